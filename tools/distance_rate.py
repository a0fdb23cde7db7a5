"""What vrt_distance_field costs, next to one pass over the same box: milliseconds a call on one GPU, in one process.

    python tools/distance_rate.py [--reps 9] [--warmup 3] [--out profiles/distance_rate.jsonl]

Device path throughout (results stay in device memory; wall clock around the call and the wait for the context's stream).  On the
sparse headline scene S1 and on the half-full `dense` at 128^3, for a 64^3 box at the grid's centre and for the whole grid, with
max_d2 = 16, 256 and unbounded; and on the whole grid of `sponge256` at 256^3; all in the same run:
  (a) vrt_fetch_voxels of the box: the floor of one pass over the box (4 bytes a voxel out, as d2);
  (b) vrt_distance_field, d2 only;
  (c) vrt_distance_field, d2 and nearest.
Each figure is the median of --reps repetitions after --warmup, with the 10th and 90th percentile.  One JSON line per configuration is
printed and appended to --out; `ratios` lines hold (b)/(a) and (c)/(b), and a last line what the pruned scan pays on the sparse scene
for an unbounded field (long lines, far targets) against max_d2 = 16."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voxel_rt2_amd import _abi, _lib, host, materials, scenes  # noqa: E402
from voxel_rt2_amd._session import NativeSession  # noqa: E402
from radiance_rate import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "distance_rate.jsonl"))
    a = ap.parse_args()
    import torch
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    rows = []

    def emit(**row):
        row = dict(tool="distance_rate", build=_lib.build_id(), **row)
        line = json.dumps(row)
        print(line, flush=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
        rows.append(row)

    def ms(t):
        return dict(ms=t[0] * 1e3, p10_ms=t[1] * 1e3, p90_ms=t[2] * 1e3)
    for scene, edges in (("s1", (64, 128)), ("dense", (64, 128)), ("sponge256", (256,))):
        mat, rgb, params = scenes.SCENES[scene](0)
        G = mat.shape[0]
        s = NativeSession(_lib.load(), "vrt_", host.make_config(64, 64, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=2, grid_res=G))
        s.upload_voxels(mat, rgb)
        s.upload_materials(materials.load_table())
        s.set_scene(host.make_scene_params(**params))
        s.set_camera(host.default_camera(64, 64))
        s.prepare()
        for edge in edges:
            lo = ((G - edge) // 2,) * 3
            hi = tuple(l + edge for l in lo)
            shape = (edge,) * 3
            bm, bc = torch.empty(shape, dtype=torch.int8, device="cuda"), torch.empty(shape + (3,), dtype=torch.uint8, device="cuda")
            d2, near = (torch.empty(shape, dtype=torch.int32, device="cuda") for _ in range(2))
            torch.cuda.synchronize()
            t_a = timed(lambda: s.fetch_voxels(lo, hi, bm.data_ptr(), bc.data_ptr(), on_device=True), s.sync, a.reps, a.warmup)
            emit(what="a_fetch_voxels", scene=scene, grid_res=G, box=edge, **ms(t_a))
            for max_d2 in (16, 256, None):
                t_b = timed(lambda: s.distance_field(lo, hi, max_d2, out=d2), s.sync, a.reps, a.warmup)
                far = float((d2 == _abi.DIST_FAR).float().mean().item())
                t_c = timed(lambda: s.distance_field(lo, hi, max_d2, nearest=True, out=(d2, near)), s.sync, a.reps, a.warmup)
                label = "unbounded" if max_d2 is None else max_d2
                emit(what="b_d2", scene=scene, grid_res=G, box=edge, max_d2=label, far_share=far, voxels_per_s=edge ** 3 / t_b[0], **ms(t_b))
                emit(what="c_d2_nearest", scene=scene, grid_res=G, box=edge, max_d2=label, voxels_per_s=edge ** 3 / t_c[0], **ms(t_c))
                emit(what="ratios", scene=scene, grid_res=G, box=edge, max_d2=label, b_over_a=t_b[0] / t_a[0], c_over_b=t_c[0] / t_b[0])
            del bm, bc, d2, near
        s.close()
    pick = lambda what, max_d2, box: next(r["ms"] for r in rows if r["what"] == what and r["scene"] == "s1" and r["box"] == box and r["max_d2"] == max_d2)
    emit(what="pruned_scan_on_sparse", scene="s1", grid_res=128,
         unbounded_over_16_box64=pick("b_d2", "unbounded", 64) / pick("b_d2", 16, 64), unbounded_over_16_full=pick("b_d2", "unbounded", 128) / pick("b_d2", 16, 128),
         unbounded_over_16_full_nearest=pick("c_d2_nearest", "unbounded", 128) / pick("c_d2_nearest", 16, 128))


if __name__ == "__main__":
    main()
