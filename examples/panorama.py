"""A 360-degree look around from the middle of the sky-lit terrace of examples/moving_box.py: no camera, no pixel grid, no temporal
filter -- Renderer.render_panorama asks the prepared scene how much light arrives along each direction of an equirectangular image
(Renderer.trace_radiance -> vrt_trace_radiance) and the result goes through the presentation curve into a PNG.  Headless.  New code,
not one of the reference's scripts.  Run from the repo root:

    VRT_PANO=1024x512 VRT_SPP=16 VRT_SKY_RES=512 python examples/panorama.py
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scene import Scene, save_image  # noqa: E402

width, height = (int(v) for v in os.environ.get("VRT_PANO", "1024x512").split("x"))
spp = int(os.environ.get("VRT_SPP", 16))

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
for cx, mat, color in ((-20, 54, (0.8, 0.2, 0.15)), (0, 2, (1.0, 0.6, 0.2)), (22, 1, (0.2, 0.5, 0.8))):   # three boxes to look at
    for x in range(cx - 3, cx + 4):
        for y in range(-38, -31):
            for z in range(-23, -16):
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
eye = (0.0, -30.5 / 64.0, 0.0)               # a little above the terrace
pano = r.render_panorama(eye, width, height, spp)
dt = time.time() - t0
print(f"{width} x {height} directions, {spp} samples each: {dt:.3f} s ({width * height * spp / dt * 1e-6:.1f} M path-samples/s)")
out = os.environ.get("VRT_OUT", os.path.join("screenshot", "panorama.png"))
if out:
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    save_image(r.tone_map(pano)[::-1], out)  # (save_image takes row 0 at the bottom; a panorama's row 0 looks up)
    print(f"Image has been saved to {out}")
