"""What vrt_label_components costs, next to one pass over the same box and next to its sibling call: milliseconds a call on one GPU, in
one process.

    python tools/label_rate.py [--reps 9] [--warmup 3] [--out profiles/label_rate.jsonl]

Device path throughout (results stay in device memory; wall clock around the call and the wait for the context's stream).  On the
sparse headline scene S1 and on the half-full `dense` at 128^3, for a 64^3 box at the grid's centre and for the whole grid; and on the
whole grid of `sponge256` at 256^3; all in the same run:
  (a) vrt_fetch_voxels of the box: the floor of one pass over the box (4 bytes a voxel out, as the labels);
  (b) vrt_distance_field, d2 only, max_d2 = 16: the sibling call;
  (c) vrt_label_components at 6- and 26-connectivity, of the solid and of the empty cells.
Each figure is the median of --reps repetitions after --warmup, with the 10th and 90th percentile.  One JSON line per configuration is
printed and appended to --out; `ratios` lines hold (c)/(a) and (c)/(b), and two last lines say what one giant component costs against
many small ones (S1's empty cells against `dense`'s solid ones, whole grid) and what 256^3 costs per voxel against 128^3."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voxel_rt2_amd import _lib, host, materials, scenes  # noqa: E402
from voxel_rt2_amd._session import NativeSession  # noqa: E402
from radiance_rate import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "label_rate.jsonl"))
    a = ap.parse_args()
    import torch
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    rows = []

    def emit(**row):
        row = dict(tool="label_rate", build=_lib.build_id(), **row)
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
            d2, labels = (torch.empty(shape, dtype=torch.int32, device="cuda") for _ in range(2))
            record = torch.zeros(4, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            t_a = timed(lambda: s.fetch_voxels(lo, hi, bm.data_ptr(), bc.data_ptr(), on_device=True), s.sync, a.reps, a.warmup)
            emit(what="a_fetch_voxels", scene=scene, grid_res=G, box=edge, **ms(t_a))
            t_b = timed(lambda: s.distance_field(lo, hi, 16, out=d2), s.sync, a.reps, a.warmup)
            emit(what="b_distance_d2_16", scene=scene, grid_res=G, box=edge, **ms(t_b))
            for conn in (6, 26):
                for empty in (False, True):
                    t_c = timed(lambda: s.label_components(lo, hi, conn, empty, out=(labels, record)), s.sync, a.reps, a.warmup)
                    cells, comps = int(record[0].item()), int(record[2].item())             # (cells < 2^31: the low word)
                    emit(what="c_label", scene=scene, grid_res=G, box=edge, connectivity=conn, members="empty" if empty else "solid", cells=cells, components=comps,
                         voxels_per_s=edge ** 3 / t_c[0], **ms(t_c))
                    emit(what="ratios", scene=scene, grid_res=G, box=edge, connectivity=conn, members="empty" if empty else "solid", c_over_a=t_c[0] / t_a[0],
                         c_over_b=t_c[0] / t_b[0])
            del bm, bc, d2, labels, record
        s.close()
    pick = lambda scene, box, conn, members: next(r["ms"] for r in rows if r["what"] == "c_label" and r["scene"] == scene and r["box"] == box and
                                                  r["connectivity"] == conn and r["members"] == members)
    emit(what="one_giant_component", s1_empty_over_dense_solid_6=pick("s1", 128, 6, "empty") / pick("dense", 128, 6, "solid"),
         s1_empty_over_dense_solid_26=pick("s1", 128, 26, "empty") / pick("dense", 128, 26, "solid"))
    emit(what="per_voxel_256_over_128", sponge256_solid_6_over_dense_solid_6=pick("sponge256", 256, 6, "solid") / 8.0 / pick("dense", 128, 6, "solid"),
         sponge256_empty_6_over_s1_empty_6=pick("sponge256", 256, 6, "empty") / 8.0 / pick("s1", 128, 6, "empty"))


if __name__ == "__main__":
    main()
