"""Boxes of voxels fall onto the terrace of moving_box.py and onto each other: every step each box still in the air is taken out of the
grid, swept down by its step (Renderer.sweep_boxes -> vrt_sweep_boxes), moved by t * move and written back (Renderer.update_voxels); a
box whose sweep stops at t = 0 rests.  Each sweep sees the edits before it, so boxes land on boxes.  The step is a power of two of
voxels, so every t is dyadic and a box always stops on a grid plane.  Headless; new code, not one of the reference's scripts.  Run from
the repo root:

    VRT_RES=640x360 VRT_SPP=4 VRT_SKY_RES=512 python examples/drop_boxes.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scene import Scene, save_image  # noqa: E402

STEP = 2                                     # voxels a step
# (lo, size) in voxel coordinates as set_voxel takes them, material, colour: released above the terrace, some above others
BOXES = [((-6, -4, -3), (7, 7, 7), 2, (1.0, 0.6, 0.2)), ((-3, 12, -1), (7, 5, 7), 11, (0.3, 0.6, 0.9)), ((-2, 28, 0), (5, 5, 5), 54, (0.9, 0.9, 0.3)),
         ((20, -10, 10), (5, 3, 5), 11, (0.4, 0.8, 0.4)), ((44, -6, 0), (6, 4, 6), 11, (0.8, 0.4, 0.7)), ((21, 6, 12), (3, 6, 3), 2, (1.0, 0.3, 0.2))]


def main():
    spp = int(os.environ.get("VRT_SPP", 4))
    scene = Scene(voxel_edges=0.0, exposure=2.0)
    scene.set_floor(-0.85, (1.0, 1.0, 1.0))
    scene.set_directional_light((1, 1, -1), 0.025, (1.3, 1.23, 1.22))
    scene.set_use_physical_sky(True)
    scene.set_use_clouds(True)
    r = scene.renderer
    half = r.voxel_grid_res // 2

    for x in range(-48, 49):                 # the terrace with its low wall
        for z in range(-48, 49):
            edge = max(abs(x), abs(z)) == 48
            for y in range(-40, -36 if edge else -38):
                scene.set_voxel((x, y, z), 11, (0.55, 0.5, 0.45) if (x // 8 + z // 8) % 2 else (0.7, 0.65, 0.6))

    def fill(box, mat, color):
        (x0, y0, z0), (sx, sy, sz) = box["lo"], box["size"]
        for x in range(x0, x0 + sx):
            for y in range(y0, y0 + sy):
                for z in range(z0, z0 + sz):
                    scene.set_voxel((x, y, z), mat, color)

    def world(box):                          # the box as sweep_boxes takes it: the same box update_voxels edits
        lo = np.array(box["lo"]) + half
        return r.box_of_voxels(lo, lo + np.array(box["size"]))

    boxes = [dict(lo=list(lo), size=size, mat=mat, color=color, resting=False) for lo, size, mat, color in BOXES]
    for b in boxes:
        fill(b, b["mat"], b["color"])
    r.prepare_data()
    for _ in range(8):
        r.accumulate_clouds(8)
    for s in range(8):
        r.compute_atmosphere(s, 8)

    dx = np.float32(2.0 / r.voxel_grid_res)
    move = np.array([0.0, -STEP * dx, 0.0], np.float32)
    steps = 0
    while not all(b["resting"] for b in boxes) and steps < 4 * r.voxel_grid_res:
        steps += 1
        for b in sorted((b for b in boxes if not b["resting"]), key=lambda b: b["lo"][1]):   # the lowest first: it makes room
            fill(b, 0, (0.0, 0.0, 0.0))
            r.update_voxels(reset=False)     # out of the grid, or the box would meet itself
            lo, hi = world(b)
            hit = r.sweep_boxes(lo, hi, move, t_max=1.0)[0]
            t = 1.0 if hit["kind"] == 0 else float(hit["t"])         # SWEEP_MISS: the whole step is free
            fall = t * STEP
            assert hit["kind"] != 3 and fall == int(fall), hit       # never SWEEP_START; dyadic t: whole voxels
            b["lo"][1] -= int(fall)
            b["resting"] = t == 0.0
            fill(b, b["mat"], b["color"])
            r.update_voxels(reset=False)
        r.reset_framebuffer()
        r.accumulate(spp)                    # a frame a step
    r.session.sync()
    print(f"{len(boxes)} boxes at rest after {steps} steps: " + ", ".join(f"y={b['lo'][1]}" for b in boxes))
    out = os.environ.get("VRT_OUT", os.path.join("screenshot", "drop_boxes.png"))
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        save_image(r.fetch_image(), out)
        print(f"Image has been saved to {out}")
    return r, boxes


if __name__ == "__main__":
    main()
