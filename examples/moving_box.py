"""A glowing box drifts across a sky-lit terrace while the frames render: the scene is prepared once (voxels, occupancy pyramid, sky
tables) and every frame only sends the box of voxels that changed (Renderer.update_voxels -> vrt_update_voxels), so the cloud and
atmosphere precompute survives.  New code, not one of the reference's scripts.  Run from the repo root:

    VRT_RES=640x360 VRT_FRAMES=48 VRT_SPP=4 VRT_SKY_RES=512 python examples/moving_box.py
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scene import Scene, save_image  # noqa: E402

frames = int(os.environ.get("VRT_FRAMES", 48))
spp = int(os.environ.get("VRT_SPP", 4))

scene = Scene(voxel_edges=0.0, exposure=2.0)
scene.set_floor(-0.85, (1.0, 1.0, 1.0))
scene.set_directional_light((1, 1, -1), 0.025, (1.3, 1.23, 1.22))
scene.set_use_physical_sky(True)
scene.set_use_clouds(True)
r = scene.renderer

for x in range(-48, 49):                     # a terrace with a low wall
    for z in range(-48, 49):
        edge = max(abs(x), abs(z)) == 48
        for y in range(-40, -36 if edge else -38):
            scene.set_voxel((x, y, z), 11, (0.55, 0.5, 0.45) if (x // 8 + z // 8) % 2 else (0.7, 0.65, 0.6))


def box(cx, mat, color):
    for x in range(cx - 3, cx + 4):
        for y in range(-34, -27):
            for z in range(-3, 4):
                scene.set_voxel((x, y, z), mat, color)


t0 = time.time()
r.prepare_data()
for _ in range(8):
    r.accumulate_clouds(8)
for s in range(8):
    r.compute_atmosphere(s, 8)
r.session.sync()
print(f"prepared, sky tables computed ({time.time() - t0:.1f} s)")

t0 = time.time()
prev = None
for k in range(frames):
    cx = -40 + (80 * k) // max(frames - 1, 1)
    if prev is not None:
        box(prev, 0, (0.0, 0.0, 0.0))
    box(cx, 2 if k % 8 < 4 else 54, (1.0, 0.6, 0.2))
    prev = cx
    r.update_voxels()                        # the box that changed, then a fresh accumulation
    r.accumulate(spp)
r.session.sync()
dt = time.time() - t0
print(f"{frames} frames of {spp} samples, one edit each: {dt:.3f} s ({dt / frames * 1e3:.2f} ms a frame)")
out = os.environ.get("VRT_OUT", os.path.join("screenshot", "moving_box.png"))
if out:
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    save_image(r.fetch_image(), out)
    print(f"Image has been saved to {out}")
