"""Offset surfaces on the terrace of moving_box.py: the torus of fill_mesh.py filled twice, side by side, in two colours each (two clip
boxes of Renderer.fill_triangles); the left one then GROWN by 2 voxels, every new voxel inheriting colour and material of its nearest
solid voxel (Renderer.grow_voxels), the right one, its copy, SHRUNK by 1 voxel (Renderer.shrink_voxels).  Both run on the device on top
of the exact distance field of the grid (Renderer.distance_field -> vrt_distance_field).  Headless; new code, not one of the
reference's scripts.  Run from the repo root:

    VRT_RES=640x360 VRT_FRAMES=16 VRT_SPP=4 VRT_SKY_RES=512 python examples/grow_shrink.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from scene import Scene, save_image  # noqa: E402
from voxelize_mesh import torus  # noqa: E402


def main():
    spp = int(os.environ.get("VRT_SPP", 4))
    frames = int(os.environ.get("VRT_FRAMES", 16))
    scene = Scene(voxel_edges=0.0, exposure=2.0)
    scene.set_floor(-0.85, (1.0, 1.0, 1.0))
    scene.set_directional_light((1, 1, -1), 0.025, (1.3, 1.23, 1.22))
    scene.set_use_physical_sky(True)
    scene.set_use_clouds(True)
    r = scene.renderer

    for x in range(-48, 49):                 # the terrace with its low wall
        for z in range(-48, 49):
            edge = max(abs(x), abs(z)) == 48
            for y in range(-40, -36 if edge else -38):
                scene.set_voxel((x, y, z), 11, (0.55, 0.5, 0.45) if (x // 8 + z // 8) % 2 else (0.7, 0.65, 0.6))
    r.prepare_data()
    for _ in range(8):
        r.accumulate_clouds(8)
    for s in range(8):
        r.compute_atmosphere(s, 8)

    g = r.voxel_grid_res
    dx = 2.0 / g
    results = {}
    for name, cx in (("grown", -22.5), ("shrunk", 22.5)):      # the same torus twice, hovering over the terrace, each half its own colour
        tv, tf = torus((cx * dx, -24.5 * dx, 0.0), 13.3 * dx, 5.6 * dx)
        lo, hi = r.mesh_box(tv)
        mid = (int(lo[0]) + int(hi[0])) // 2
        r.fill_triangles(tv, tf, color=(230, 150, 60), mat=54, lo=lo, hi=(mid, hi[1], hi[2]), reset=False)
        r.fill_triangles(tv, tf, color=(70, 150, 230), mat=54, lo=(mid, lo[1], lo[2]), hi=hi, reset=False)
        results[name] = dict(lo=np.array(lo), hi=np.array(hi), before=int((r.voxel_material[tuple(slice(int(a), int(b)) for a, b in zip(lo, hi))] == 54).sum()))
    for name, grow in (("grown", True), ("shrunk", False)):
        res = results[name]
        lo, hi = np.maximum(res["lo"] - 2, 0), np.minimum(res["hi"] + 2, g)
        # (the terrace lies more than 2 voxels below the tori, so only the tori grow into these boxes)
        res["changed"] = r.grow_voxels(lo, hi, 2, reset=False) if grow else r.shrink_voxels(lo, hi, 1, reset=False)
        res["lo"], res["hi"] = lo, hi
        res["after"] = int((r.voxel_material[tuple(slice(int(a), int(b)) for a, b in zip(lo, hi))] == 54).sum())
        print(f"{name}: {res['before']} voxels -> {res['after']} ({res['changed']} changed) in {lo.tolist()} .. {hi.tolist()}")
    r.reset_framebuffer()
    for _ in range(frames):
        r.accumulate(spp)
    r.session.sync()
    out = os.environ.get("VRT_OUT", os.path.join("screenshot", "grow_shrink.png"))
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        save_image(r.fetch_image(), out)
        print(f"Image has been saved to {out}")
    return r, results


if __name__ == "__main__":
    main()
