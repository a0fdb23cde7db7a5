"""Ask the scene, then edit it: a fan of rays from the camera goes into the terrace of moving_box.py (Renderer.cast_rays ->
vrt_cast_rays), and on the face each ray hit -- cell + normal of its record -- a glowing voxel is placed (set_voxel, then
Renderer.update_voxels).  Headless; new code, not one of the reference's scripts.  Run from the repo root:

    VRT_RES=640x360 VRT_SPP=16 VRT_SKY_RES=512 VRT_FAN=24x12 python examples/pick_and_place.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scene import Scene, save_image  # noqa: E402

spp = int(os.environ.get("VRT_SPP", 16))
fan_u, fan_v = (int(x) for x in os.environ.get("VRT_FAN", "24x12").split("x"))

scene = Scene(voxel_edges=0.0, exposure=2.0)
scene.set_floor(-0.85, (1.0, 1.0, 1.0))
scene.set_directional_light((1, 1, -1), 0.025, (1.3, 1.23, 1.22))
scene.set_use_physical_sky(True)
scene.set_use_clouds(True)
r = scene.renderer

for x in range(-48, 49):                     # the terrace with its low wall
    for z in range(-48, 49):
        edge = max(abs(x), abs(z)) == 48
        for y in range(-40, -36 if edge else -38):
            scene.set_voxel((x, y, z), 11, (0.55, 0.5, 0.45) if (x // 8 + z // 8) % 2 else (0.7, 0.65, 0.6))

r.prepare_data()
for _ in range(8):
    r.accumulate_clouds(8)
for s in range(8):
    r.compute_atmosphere(s, 8)

# one ray through every (W / fan_u, H / fan_v)-th pixel
W, H = r.image_res
pixels = [(int((i + 0.5) * W / fan_u), int((j + 0.5) * H / fan_v)) for j in range(fan_v) for i in range(fan_u)]
rays = [r.pick_ray(u, v) for u, v in pixels]
hits = r.cast_rays(np.array([o for o, _ in rays]), np.array([d for _, d in rays]))
half = r.voxel_grid_res // 2
placed = 0
for h in hits:
    if h["kind"] != 2:                       # VRT_HIT_VOXEL: the floor and the sky take no voxel
        continue
    cell = h["cell"] + np.rint(h["normal"]).astype(int)          # the empty cell in front of the face that was hit
    if ((cell < 0) | (cell >= r.voxel_grid_res)).any():
        continue
    scene.set_voxel(tuple(int(c) - half for c in cell), 2, (1.0, 0.6, 0.2))
    placed += 1
print(f"{len(hits)} rays: {int((hits['kind'] == 2).sum())} on voxels, {int((hits['kind'] == 1).sum())} on the floor, "
      f"{int((hits['kind'] == 0).sum())} into the sky; {placed} voxels placed")
r.update_voxels()                            # the box that holds them, then a fresh accumulation
r.accumulate(spp)
out = os.environ.get("VRT_OUT", os.path.join("screenshot", "pick_and_place.png"))
if out:
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    save_image(r.fetch_image(), out)
    print(f"Image has been saved to {out}")
