"""An edit, a reset, and the first frames behind it -- raw and through the g-buffer-guided filter (Renderer.fetch_denoised ->
vrt_denoise), side by side: 1, 4 and 16 samples a pixel.  The scene is prepared once; a block is put on the terrace
(Renderer.update_voxels), which starts a fresh accumulation, and the frames that follow are the noisy ones the filter is for.  The
filter's defaults are a matter of taste, not validated on images: look at the pictures.  New code, not one of the reference's scripts.
Run from the repo root:

    VRT_RES=640x360 python examples/denoise_edit.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scene import Scene, save_image  # noqa: E402

scene = Scene(voxel_edges=0.06, exposure=2.0)
scene.set_floor(-0.85, (1.0, 1.0, 1.0))
scene.set_background_color((0.5, 0.6, 0.8))
scene.set_directional_light((1, 1, -1), 0.1, (1.3, 1.23, 1.22))
r = scene.renderer

for x in range(-40, 41):                     # a chequered terrace with a wall behind it
    for z in range(-40, 41):
        for y in range(-40, -12 if z == -40 else -38):
            scene.set_voxel((x, y, z), 11, (0.75, 0.35, 0.3) if (x // 8 + z // 8 + y // 8) % 2 else (0.8, 0.78, 0.7))

r.prepare_data()
r.accumulate(64)                             # the settled frame before the edit

for x in range(-6, 7):                       # the edit: a block on the terrace
    for y in range(-38, -26):
        for z in range(-6, 7):
            scene.set_voxel((x, y, z), 11, (0.3, 0.5, 0.8))
r.update_voxels()                            # the box that changed, then reset_framebuffer(): a fresh accumulation

out_dir = os.environ.get("VRT_OUT_DIR", "screenshot")
os.makedirs(out_dir, exist_ok=True)
done = 0
for spp in (1, 4, 16):
    r.accumulate(spp - done)
    done = spp
    raw = r.tone_map(r.fetch_hdr())          # the same curve for both halves: fetch_image's without its vignette
    clean = r.fetch_denoised(ldr=True)
    path = os.path.join(out_dir, f"denoise_edit_{spp:02d}spp.png")
    save_image(np.concatenate([raw, clean], axis=1), path)
    print(f"{spp:2d} samples a pixel: raw | denoised saved to {path}")
