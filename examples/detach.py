"""A pillar on the terrace of moving_box.py is cut through, and what no longer stands falls: a slab is carved out of the pillar
(Renderer.update_voxels); the piece that now floats is FOUND, not remembered -- Renderer.floating_voxels marks the solid voxels of a box
whose connected component does not reach the box's lowest layer, Renderer.components says which component that is and gives its tight
box (both on top of Renderer.label_components -> vrt_label_components, on the device); the box is taken out of the grid, swept down
(Renderer.box_of_voxels, Renderer.sweep_boxes) and written back lower by the distance the sweep allows (two more update_voxels calls).
A frame before and a frame after.  Headless; new code, not one of the reference's scripts.  Run from the repo root:

    VRT_RES=640x360 VRT_FRAMES=16 VRT_SPP=4 VRT_SKY_RES=512 python examples/detach.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scene import Scene, save_image  # noqa: E402

PILLAR = ((-5, -38, -4), (4, -8, 5))         # [lo, hi) in voxel coordinates as set_voxel takes them: on the terrace's top
CUT = (-27, -23)                             # the slab carved out: y in [lo, hi)
REACH = 64                                   # voxels the sweep looks down: a power of two, so every t is dyadic and the fall a whole number


def main():
    spp = int(os.environ.get("VRT_SPP", 4))
    frames = int(os.environ.get("VRT_FRAMES", 16))
    scene = Scene(voxel_edges=0.0, exposure=2.0)
    scene.set_floor(-0.85, (1.0, 1.0, 1.0))
    scene.set_directional_light((1, 1, -1), 0.025, (1.3, 1.23, 1.22))
    scene.set_use_physical_sky(True)
    scene.set_use_clouds(True)
    r = scene.renderer
    g = r.voxel_grid_res
    half = g // 2

    for x in range(-48, 49):                 # the terrace with its low wall
        for z in range(-48, 49):
            edge = max(abs(x), abs(z)) == 48
            for y in range(-40, -36 if edge else -38):
                scene.set_voxel((x, y, z), 11, (0.55, 0.5, 0.45) if (x // 8 + z // 8) % 2 else (0.7, 0.65, 0.6))
    (x0, y0, z0), (x1, y1, z1) = PILLAR
    for x in range(x0, x1):                  # the pillar, banded, with a cap that overhangs
        for y in range(y0, y1):
            for z in range(z0, z1):
                scene.set_voxel((x, y, z), 54 if y % 6 < 3 else 2, (0.8, 0.35, 0.25) if y % 6 < 3 else (0.9, 0.85, 0.7))
    for x in range(x0 - 2, x1 + 2):
        for z in range(z0 - 2, z1 + 2):
            scene.set_voxel((x, y1, z), 11, (0.3, 0.4, 0.6))
    r.prepare_data()
    for _ in range(8):
        r.accumulate_clouds(8)
    for s in range(8):
        r.compute_atmosphere(s, 8)

    def render(name):
        r.reset_framebuffer()
        for _ in range(frames):
            r.accumulate(spp)
        r.session.sync()
        out = os.environ.get("VRT_OUT", os.path.join("screenshot", "detach.png"))
        if out:
            root, ext = os.path.splitext(out)
            os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
            save_image(r.fetch_image(), root + "_" + name + ext)
            print(f"Image has been saved to {root}_{name}{ext}")

    render("before")
    for x in range(x0, x1):                  # 1. the cut
        for y in range(*CUT):
            for z in range(z0, z1):
                scene.set_voxel((x, y, z), 0, (0.0, 0.0, 0.0))
    r.update_voxels(reset=False)

    # 2. what floats: the box stands on the terrace's bottom layer, so whatever is joined to the terrace stands
    lo, hi = (0, -40 + half, 0), (g, g, g)
    floating = r.floating_voxels(lo, hi)
    table = r.components(lo, hi)
    labels, record = r.label_components(lo, hi)
    roots = np.unique(labels[floating.cpu().numpy()])
    assert len(roots) == 1, roots            # one piece came loose
    row = int(np.flatnonzero(table["root"].cpu().numpy() == roots[0])[0])
    c_lo, c_hi = table["lo"][row].cpu().numpy(), table["hi"][row].cpu().numpy()   # 3. its tight box, array indices
    size = int(table["size"][row].item())
    sl = tuple(slice(int(a), int(b)) for a, b in zip(c_lo, c_hi))
    piece = labels[tuple(slice(int(a) - l, int(b) - l) for a, b, l in zip(c_lo, c_hi, lo))] == roots[0]
    mat, rgb = r.voxel_material[sl].copy(), r.voxel_color[sl].copy()
    cells = np.argwhere(piece) + c_lo
    print(f"{record['components']} components of {record['cells']} solid voxels; the piece that floats: {size} voxels in {c_lo.tolist()} .. {c_hi.tolist()}")

    def write(at, put):                      # the piece's voxels at array index `at` (its box's corner): put, or taken out
        for (i, j, k) in np.argwhere(piece):
            c = (rgb[i, j, k] + np.float32(0.5)) / np.float32(255.0)       # (set_voxel truncates c * 255: the same byte again)
            scene.set_voxel((at[0] + i - half, at[1] + j - half, at[2] + k - half), int(mat[i, j, k]) if put else 0, c if put else (0.0, 0.0, 0.0))
        r.update_voxels(reset=False)

    write(c_lo, False)                       # out of the grid, or the box would meet itself
    dx = np.float32(2.0 / g)
    hit = r.sweep_boxes(*r.box_of_voxels(c_lo, c_hi), np.array([0.0, -REACH * dx, 0.0], np.float32), t_max=1.0)[0]   # 4. the sweep
    fall = float(hit["t"]) * REACH
    assert hit["kind"] == 2 and fall == int(fall) and fall > 0, hit          # SWEEP_VOXEL: it lands on the stump; whole voxels
    new_lo = c_lo - np.array([0, int(fall), 0])
    write(new_lo, True)                      # 5. back, lower
    print(f"it falls {int(fall)} voxels and rests at {new_lo.tolist()}")
    render("after")                          # 6.
    return r, dict(cells=cells, size=size, lo=c_lo, hi=c_hi, fall=int(fall), new_lo=new_lo, new_hi=c_hi - np.array([0, int(fall), 0]), piece=piece)


if __name__ == "__main__":
    main()
