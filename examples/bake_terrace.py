"""A light map of the sky-lit terrace of examples/moving_box.py with the glowing box parked on it: no camera and no frame --
Renderer.bake_faces lists the exposed voxel faces (surface_faces) and asks the prepared scene how much light falls on each
(gather_irradiance -> vrt_gather_irradiance).  The irradiance sky_rgb + sun_rgb of the upward faces goes through the presentation curve
into a PNG, one pixel a voxel column, and the sunlit fraction and the mean sky openness are printed.  Headless.  New code, not one of the
reference's scripts.  Run from the repo root:

    VRT_SPP=64 VRT_SKY_RES=512 python examples/bake_terrace.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scene import Scene, save_image  # noqa: E402

spp = int(os.environ.get("VRT_SPP", 64))

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
for x in range(-3, 4):                       # the glowing box, parked
    for y in range(-38, -31):
        for z in range(-3, 4):
            scene.set_voxel((x, y, z), 2, (1.0, 0.6, 0.2))

t0 = time.time()
r.prepare_data()
for _ in range(8):
    r.accumulate_clouds(8)
for s in range(8):
    r.compute_atmosphere(s, 8)
r.session.sync()
print(f"prepared, sky tables computed ({time.time() - t0:.1f} s)")

t0 = time.time()
h = r.voxel_grid_res // 2
lo, hi = (h - 48, h - 40, h - 48), (h + 49, h - 30, h + 49)
cell, face, irr = r.bake_faces(lo, hi, spp)
dt = time.time() - t0
print(f"{len(cell)} faces, {spp} samples each: {dt:.3f} s ({len(cell) * spp / dt * 1e-6:.1f} M samples/s)")
top = face == 3
print(f"upward faces: {int(top.sum())}, sunlit fraction {float((irr['sun'][top] > 0.5).mean()):.3f}, mean sky openness {float(irr['sky'][top].mean()):.3f}")
light = np.zeros((hi[2] - lo[2], hi[0] - lo[0], 3), np.float32)       # one pixel a column: the topmost upward face wins
order = np.argsort(cell[top][:, 1], kind="stable")
c, e = cell[top][order], (irr["sky_rgb"] + irr["sun_rgb"])[top][order]
light[c[:, 2] - lo[2], c[:, 0] - lo[0]] = e
out = os.environ.get("VRT_OUT", os.path.join("screenshot", "bake_terrace.png"))
if out:
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    save_image(r.tone_map(light / np.float32(np.pi)), out)            # (a white diffuse surface under irradiance E shows E / pi)
    print(f"Image has been saved to {out}")
