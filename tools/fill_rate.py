"""What vrt_fill_triangles costs, next to the surface pass and the edit both end in: milliseconds a call on one GPU, in one process.

    python tools/fill_rate.py [--reps 9] [--warmup 3] [--out profiles/fill_rate.jsonl]

The headline scene S1, 128^3, device path throughout (triangles and box arrays stay in device memory; wall clock around the call, which
synchronises once itself).  For a 64^3 box at the grid's centre and the 128^3 box that is the whole grid, in the same run:
  (a) vrt_update_voxels of the box with its own content: the floor, because both calls end in that very work (launch_edit);
  (b) vrt_voxelize_triangles of an icosphere filling the box, subdivided 3, 6 and 8 times: 1 280, 81 920 and 1 310 720 triangles;
  (c) vrt_fill_triangles of the same mesh;
  (d) (c) with a grid-spanning slab (a triangle larger than the grid and its copy a few voxels higher: closed as far as the grid can
      see; below the 64^3 box, where its toggles cancel at the box's floor) put in front of the mesh.
Each figure is the median of --reps repetitions after --warmup, with the 10th and 90th percentile.  One JSON line per configuration is
printed and appended to --out; `ratios` lines hold (c)/(a), (c)/(b) and (d) - (c), and a last line the two claims: the fill costs the
same order as the surface pass, and the slab adds less than (a) at the full grid."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voxel_rt2_amd import _lib, host, materials, scenes  # noqa: E402
from voxel_rt2_amd._session import NativeSession  # noqa: E402
from radiance_rate import timed  # noqa: E402
from voxelize_rate import icosphere_triangles, records  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "fill_rate.jsonl"))
    a = ap.parse_args()
    import torch
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    mat, rgb, params = scenes.SCENES["s1"](0)
    G = mat.shape[0]
    s = NativeSession(_lib.load(), "vrt_", host.make_config(64, 64, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=2, grid_res=G))
    s.upload_voxels(mat, rgb)
    s.upload_materials(materials.load_table())
    s.set_scene(host.make_scene_params(**params))
    s.set_camera(host.default_camera(64, 64))
    s.prepare()
    rows = []

    def emit(**row):
        row = dict(tool="fill_rate", build=_lib.build_id(), scene="s1", grid_res=G, **row)
        line = json.dumps(row)
        print(line, flush=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
        rows.append(row)

    def ms(t):
        return dict(ms=t[0] * 1e3, p10_ms=t[1] * 1e3, p90_ms=t[2] * 1e3)
    payload = 90 | 160 << 8 | 230 << 16 | 11 << 24
    tri =lambda z: [[(-3.0, -3.0, z), (3.0, -3.0, z), (0.0, 4.0, z)]]
    slab = records(np.array(tri(-0.9) + tri(-0.8), float), payload)                 # closed as far as the grid can see: every column of it is crossed twice
    for edge in (64, 128):
        lo = ((G - edge) // 2,) * 3
        hi = tuple(l + edge for l in lo)
        bm, bc = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in s.fetch_voxels(lo, hi))
        torch.cuda.synchronize()
        t_edit = timed(lambda: s.update_voxels(lo, hi, bm.data_ptr(), bc.data_ptr(), on_device=True), s.sync, a.reps, a.warmup)
        emit(what="a_update_voxels", box=edge, **ms(t_edit))
        for sub in (3, 6, 8):
            mesh = records(icosphere_triangles((0.0, 0.0, 0.0), 0.45 * edge * 2.0 / G, sub), payload)
            t = {}
            for what, recs, call in (("b_voxelize", mesh, s.voxelize_triangles), ("c_fill", mesh, lambda d, lo, hi: s.fill_triangles(d, lo, hi, payload)),
                                     ("d_fill_with_spanning_slab", np.concatenate([slab, mesh]), lambda d, lo, hi: s.fill_triangles(d, lo, hi, payload))):
                d = torch.from_numpy(recs.view(np.uint8).reshape(-1)).cuda()
                torch.cuda.synchronize()
                res = call(d, lo, hi)
                t[what] = timed(lambda: call(d, lo, hi), s.sync, a.reps, a.warmup)
                emit(what=what, box=edge, triangles=len(recs), voxels=int(res["voxels"]), invalid=int(res["invalid"]), triangles_per_s=len(recs) / t[what][0], **ms(t[what]))
                del d
                s.update_voxels(lo, hi, bm.data_ptr(), bc.data_ptr(), on_device=True)   # the scene as it was
            emit(what="ratios", box=edge, triangles=len(mesh), c_over_a=t["c_fill"][0] / t_edit[0], c_over_b=t["c_fill"][0] / t["b_voxelize"][0],
                 d_minus_c_ms=(t["d_fill_with_spanning_slab"][0] - t["c_fill"][0]) * 1e3)
    full = next(r["ms"] for r in rows if r["what"] == "a_update_voxels" and r["box"] == G)
    ratios = [r for r in rows if r["what"] == "ratios"]
    worst = max(r["d_minus_c_ms"] for r in ratios)
    emit(what="claims", a_full_grid_ms=full, worst_d_minus_c_ms=worst, slab_adds_less_than_a=bool(worst <= full),
         c_over_b_min=min(r["c_over_b"] for r in ratios), c_over_b_max=max(r["c_over_b"] for r in ratios),
         same_order_as_surface_pass=bool(max(r["c_over_b"] for r in ratios) < 10.0 and min(r["c_over_b"] for r in ratios) > 0.1))
    s.close()


if __name__ == "__main__":
    main()
