"""An irradiance volume over the sky-lit terrace of examples/bake_terrace.py with the glowing box parked on it: no camera and no frame --
Renderer.probe_lattice lists the empty cells of a coarse lattice over the terrace and Renderer.gather_probes asks the prepared scene
for the light at each (vrt_gather_probes: nine spherical-harmonic coefficients a colour channel, the sun kept apart).  The PNG shows
one lit ball per probe, a panel per layer of the lattice (the lowest at the bottom), each seen from above and a little from the south:
every pixel of a ball has a normal, Renderer.sh_irradiance gives the irradiance on it (the sun's term with max(0, n . light_direction)),
and a grey diffuse surface of albedo 0.18 under irradiance E shows 0.18 E / pi through the presentation curve -- what a character or a
gizmo standing at that point would look like.
Headless.  New code, not one of the reference's scripts.  Run from the repo root:

    VRT_SPP=256 VRT_SKY_RES=512 python examples/probe_volume.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scene import Scene, save_image  # noqa: E402

spp = int(os.environ.get("VRT_SPP", 256))
step = int(os.environ.get("VRT_PROBE_STEP", 12))
light_direction = (1, 1, -1)

scene = Scene(voxel_edges=0.0, exposure=2.0)
scene.set_floor(-0.85, (1.0, 1.0, 1.0))
scene.set_directional_light(light_direction, 0.025, (1.3, 1.23, 1.22))
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
lo, hi = (h - 46, h - 36, h - 46), (h + 47, h - 36 + 2 * step, h + 47)       # two layers of probes above the terrace's floor
centre, cell = r.probe_lattice(lo, hi, step)
rec = r.gather_probes(centre, samples=spp)
dt = time.time() - t0
print(f"{len(centre)} probes, {spp} samples each: {dt:.3f} s ({len(centre) * spp / dt * 1e-6:.2f} M samples/s)")
print(f"mean sky openness {float(rec['sky'].mean()):.3f}, sunlit fraction {float((rec['sun'] > 0.5).mean()):.3f}")

# one ball a probe: an orthographic view from above and a little from the south (+z), north up; a panel a layer, the lowest at the bottom
R = 14                                       # a ball's radius in pixels
px = 2 * R + 6                               # pixels a lattice step
ix = (cell - np.array(lo)) // step
nx, ny, nz = (int(v) + 1 for v in ix.max(axis=0))
to_eye = np.array((0.0, 0.8, 0.6))
right, up = np.array((1.0, 0.0, 0.0)), np.array((0.0, 0.6, -0.8))           # the image's axes in the world: right x up = to_eye
panel = px * nz + px // 2
img = np.zeros((panel * ny + px // 2, px * (nx + 1), 3), np.float32)
yy, xx = np.mgrid[-R:R + 1, -R:R + 1]
inside = xx * xx + yy * yy <= R * R
a, b = xx[inside] / R, -yy[inside] / R                                      # the ball's image coordinates, b upward
normals = a[:, None] * right + b[:, None] * up + np.sqrt(np.maximum(1.0 - a * a - b * b, 0.0))[:, None] * to_eye
sun = np.array(light_direction, np.float64) / np.linalg.norm(light_direction)
for k in range(len(rec)):
    e = r.sh_irradiance(rec[k:k + 1], normals, light_direction=sun)
    cx = int(px * (ix[k, 0] + 0.5)) + px // 2
    cy = img.shape[0] - panel * int(ix[k, 1]) - int(px * (nz - 1 - ix[k, 2] + 0.5)) - px // 2
    img[cy + yy[inside], cx + xx[inside]] = 0.18 * np.maximum(e, 0.0) / np.pi
out = os.environ.get("VRT_OUT", os.path.join("screenshot", "probe_volume.png"))
if out:
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    save_image(r.tone_map(img[::-1]), out)                              # (save_image takes row 0 for the bottom row; img has it on top)
    print(f"Image has been saved to {out}")
