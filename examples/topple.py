"""The pillar of detach.py is cut through again, and this time the piece that comes loose is MOVED, not rewritten voxel by voxel: it is
found on the device (Renderer.label_components, floating_voxels, components), the layer under it is swept down to see how far it can fall
(Renderer.sweep_boxes), and ONE Renderer.move_voxels(select=labels, select_value=root, shift=...) puts it where it lands
(vrt_move_voxels: the voxels never visit the host).  Then it topples: a quarter turn about its lower edge with if_free=True -- the library
turns it only if no solid voxel is in the way, and says so; a piece that did tip is let fall once more, one that could not stays upright.
A frame before and a frame after, and the three counts of every move.  Headless; new code, not one of the reference's scripts.  Run from
the repo root:

    VRT_RES=640x360 VRT_FRAMES=16 VRT_SPP=4 VRT_SKY_RES=512 python examples/topple.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scene import Scene, save_image  # noqa: E402

PILLAR = ((-5, -38, -4), (4, -8, 5))         # [lo, hi) in voxel coordinates as set_voxel takes them: on the terrace's top
CUT = (-27, -23)                             # the slab carved out: y in [lo, hi)
REACH = 64                                   # voxels a sweep looks down: a power of two, so every t is dyadic and the fall a whole number


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
        out = os.environ.get("VRT_OUT", os.path.join("screenshot", "topple.png"))
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
    cut_grid = r.voxel_material.copy(), r.voxel_color.copy()

    # 2. what floats, as in detach.py: its root and its tight box
    lo, hi = (0, -40 + half, 0), (g, g, g)
    floating = r.floating_voxels(lo, hi)
    table = r.components(lo, hi)
    labels, record = r.label_components(lo, hi)
    roots = np.unique(labels[floating.cpu().numpy()])
    assert len(roots) == 1, roots            # one piece came loose
    root = int(roots[0])
    row = int(np.flatnonzero(table["root"].cpu().numpy() == root)[0])
    c_lo, c_hi = table["lo"][row].cpu().numpy(), table["hi"][row].cpu().numpy()
    print(f"{record['components']} components of {record['cells']} solid voxels; the piece that floats: {int(table['size'][row].item())} voxels in {c_lo.tolist()} .. {c_hi.tolist()}")

    def fall_of(b_lo, b_hi):                 # how far the box of array indices can fall: the layer under it swept down, plus that layer
        under_lo, under_hi = (b_lo[0], b_lo[1] - 1, b_lo[2]), (b_hi[0], b_lo[1], b_hi[2])
        dx = np.float32(2.0 / g)
        hit = r.sweep_boxes(*r.box_of_voxels(under_lo, under_hi), np.array([0.0, -REACH * dx, 0.0], np.float32), t_max=1.0)[0]
        if hit["kind"] == 3:                 # SWEEP_START: it rests on something already
            return 0
        fall = float(hit["t"]) * REACH
        assert hit["kind"] in (1, 2) and fall == int(fall), hit          # it lands on voxels or the floor, after whole voxels
        return int(fall) + 1

    steps = []

    def move(what, src_lo, src_hi, **kw):
        res = r.move_voxels(src_lo, src_hi, reset=False, **kw)
        steps.append(dict(src_lo=tuple(int(v) for v in src_lo), src_hi=tuple(int(v) for v in src_hi), kw=kw, res=res))
        print(f"{what}: written {res['written']}, blocked {res['blocked']}, erased {res['erased']}")
        return res

    # 3. it lands: ONE move, the labels select the piece out of the box it was found in
    fall = fall_of(c_lo, c_hi)
    assert fall > 0
    res = move(f"it falls {fall} voxels", lo, hi, shift=(0, -fall, 0), select=labels, select_value=root, dst_lo=lo, dst_hi=hi)
    assert res["written"] == res["erased"] and res["blocked"] == 0
    p_lo, p_hi = np.array(res["lo"]), np.array(res["hi"])                  # where the piece is now: nothing else is in this box
    # 4. it topples towards +x: a quarter turn about z through the lower edge of the pillar's side, only if nothing is in the way
    pivot = (x1 + half, int(p_lo[1]), 0)
    tip = move("it tips over", p_lo, p_hi, rotation=r.rotation_matrix("z", -90), pivot=pivot, if_free=True)
    tipped = tip["written"] > 0
    if tipped:                               # 5. and falls once more, lying down
        p_lo, p_hi = np.array(tip["lo"]), np.array(tip["hi"])
        fall2 = fall_of(p_lo, p_hi)
        if fall2:
            last = move(f"it falls {fall2} more", p_lo, p_hi, shift=(0, -fall2, 0))
            p_lo, p_hi = np.array(last["lo"]), np.array(last["hi"])
    else:
        print("the tipped pose is blocked: it stays upright")
    render("after")
    return r, dict(root=root, labels=labels, box=(lo, hi), cut_grid=cut_grid, steps=steps, tipped=tipped, lo=p_lo, hi=p_hi)


if __name__ == "__main__":
    main()
