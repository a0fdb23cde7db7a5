"""What vrt_voxelize_triangles costs, next to the edit it ends in: milliseconds a call on one GPU, in one process.

    python tools/voxelize_rate.py [--reps 9] [--warmup 3] [--out profiles/voxelize_rate.jsonl]

The headline scene S1, 128^3, device path throughout (triangles and box arrays stay in device memory; wall clock around the call, which
synchronises once itself).  For a 64^3 box at the grid's centre and the 128^3 box that is the whole grid:
  (a) vrt_update_voxels of the box with its own content: the floor, because the voxeliser ends in that very work (launch_edit);
  (b) vrt_voxelize_triangles of an icosphere filling the box, subdivided 3, 6 and 8 times: 1 280, 81 920 and 1 310 720 triangles;
  (c) (b) with one triangle spanning the grid put in front of the mesh.
Each figure is the median of --reps repetitions after --warmup, with the 10th and 90th percentile.  One JSON line per configuration is
printed and appended to --out, and a last line holds the one condition the issue sets: the lone large triangle must not serialise on
one wave -- (c) - (b) stays below (a) at the full grid."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voxel_rt2_amd import _abi, _lib, host, materials, scenes  # noqa: E402
from voxel_rt2_amd._session import NativeSession  # noqa: E402
from radiance_rate import timed  # noqa: E402


def icosphere_triangles(centre, radius, subdivisions):
    """float64 (20 * 4^s, 3, 3): an icosahedron's triangles split in four s times, every vertex pushed out to the sphere"""
    g = (1 + 5 ** 0.5) / 2
    v = np.array([(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)], float)
    f = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
                  (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)])
    t = v[f] / np.linalg.norm(v[0])
    unit = lambda p: p / np.linalg.norm(p, axis=-1, keepdims=True)
    for _ in range(subdivisions):
        a, b, c = t[:, 0], t[:, 1], t[:, 2]
        ab, bc, ca = unit(a + b), unit(b + c), unit(c + a)
        t = np.concatenate([np.stack(x, axis=1) for x in ((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca))])
    return t * radius + np.asarray(centre, float)


def records(tri, voxel):
    r = np.zeros(len(tri), _abi.TRIANGLE)
    r["v0"], r["v1"], r["v2"], r["voxel"] = tri[:, 0], tri[:, 1], tri[:, 2], voxel
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "voxelize_rate.jsonl"))
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
        row = dict(tool="voxelize_rate", build=_lib.build_id(), scene="s1", grid_res=G, **row)
        line = json.dumps(row)
        print(line, flush=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
        rows.append(row)

    def ms(t):
        return dict(ms=t[0] * 1e3, p10_ms=t[1] * 1e3, p90_ms=t[2] * 1e3)
    span = records(np.array([[(-1.5, -1.25, -1.0), (1.5, 1.0, 1.25), (1.25, -1.5, 0.75)]]), 200 | 120 << 8 | 40 << 16 | 11 << 24)
    for edge in (64, 128):
        lo = ((G - edge) // 2,) * 3
        hi = tuple(l + edge for l in lo)
        bm, bc = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in s.fetch_voxels(lo, hi))
        torch.cuda.synchronize()
        t_edit = timed(lambda: s.update_voxels(lo, hi, bm.data_ptr(), bc.data_ptr(), on_device=True), s.sync, a.reps, a.warmup)
        emit(what="a_update_voxels", box=edge, **ms(t_edit))
        for sub in (3, 6, 8):
            mesh = records(icosphere_triangles((0.0, 0.0, 0.0), 0.45 * edge * 2.0 / G, sub), 90 | 160 << 8 | 230 << 16 | 11 << 24)
            t = {}
            for what, recs in (("b_voxelize", mesh), ("c_voxelize_with_spanning_triangle", np.concatenate([span, mesh]))):
                d = torch.from_numpy(recs.view(np.uint8).reshape(-1)).cuda()
                torch.cuda.synchronize()
                res = s.voxelize_triangles(d, lo, hi)
                t[what] = timed(lambda: s.voxelize_triangles(d, lo, hi), s.sync, a.reps, a.warmup)
                emit(what=what, box=edge, triangles=len(recs), voxels=int(res["voxels"]), invalid=int(res["invalid"]), triangles_per_s=len(recs) / t[what][0],
                     **ms(t[what]))
                del d
            emit(what="ratios", box=edge, triangles=len(mesh), b_over_a=t["b_voxelize"][0] / t_edit[0],
                 c_over_b=t["c_voxelize_with_spanning_triangle"][0] / t["b_voxelize"][0],
                 c_minus_b_ms=(t["c_voxelize_with_spanning_triangle"][0] - t["b_voxelize"][0]) * 1e3)
            s.update_voxels(lo, hi, bm.data_ptr(), bc.data_ptr(), on_device=True)   # the scene as it was
    full = next(r["ms"] for r in rows if r["what"] == "a_update_voxels" and r["box"] == G)
    worst = max(r["c_minus_b_ms"] for r in rows if r["what"] == "ratios")
    emit(what="condition", a_full_grid_ms=full, worst_c_minus_b_ms=worst, holds=bool(worst <= full))
    s.close()


if __name__ == "__main__":
    main()
