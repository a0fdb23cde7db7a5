"""What an edit costs: vrt_update_voxels against the same change made through vrt_upload_voxels + vrt_prepare, on one GPU, in one process.

    python tools/edit_cost.py [--reps 40] [--warmup 5] [--out profiles/edit_cost.md]

Per case (128^3: one voxel, a 16^3 box, a 64^3 box; 256^3: a 16^3 box) three ways of reaching the same device state: the edit from host
arrays, the edit from device memory (a torch tensor), and the full path -- unchanged code, so the cost a caller paid before the entry
point existed.  Wall clock around a sync (both paths end in one), the median of --reps repetitions after --warmup, with the spread.
Every repetition really changes the grid: the box alternates between two contents.  Prints one JSON line per case and writes the table."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voxel_rt2_amd import _lib, host, materials, scenes  # noqa: E402
from voxel_rt2_amd._session import NativeSession  # noqa: E402

CASES = [(128, "one voxel", (70, 90, 70), 1), (128, "16^3 box", (61, 83, 59), 16), (128, "64^3 box", (31, 33, 29), 64), (256, "16^3 box", (121, 163, 119), 16)]


def timed(fn, sync, reps, warmup):
    out = []
    for k in range(warmup + reps):
        sync()
        t0 = time.perf_counter()
        fn(k)
        sync()
        if k >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    out.sort()
    return dict(median_ms=statistics.median(out), p10_ms=out[len(out) // 10], p90_ms=out[(9 * len(out)) // 10], n=len(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "edit_cost.md"))
    a = ap.parse_args()
    import torch
    rows = []
    sessions = {}
    for G, label, lo, n in CASES:
        if G not in sessions:
            mat, rgb, params = scenes.SCENES["s1" if G == 128 else "s1_256"](0)
            s = NativeSession(_lib.load(), "vrt_", host.make_config(64, 48, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=4, grid_res=G))
            s.upload_voxels(mat, rgb)
            s.upload_materials(materials.load_table())
            s.set_scene(host.make_scene_params(**params))
            s.set_camera(host.default_camera(64, 48))
            s.prepare()
            sessions[G] = (s, mat.copy(), rgb.copy())
        s, mat, rgb = sessions[G]
        hi = tuple(v + n for v in lo)
        rng = np.random.default_rng(n)
        contents = [((rng.random((n, n, n)) < 0.5) * 11).astype(np.int8) for _ in range(2)]
        colours = [rng.integers(0, 256, (n, n, n, 3)).astype(np.uint8) for _ in range(2)]
        dev = [(torch.from_numpy(m).cuda(), torch.from_numpy(c).cuda()) for m, c in zip(contents, colours)]
        torch.cuda.synchronize()
        box = tuple(slice(l, h) for l, h in zip(lo, hi))

        def edit_host(k):
            s.update_voxels(lo, hi, contents[k & 1], colours[k & 1])

        def edit_device(k):
            s.update_voxels(lo, hi, dev[k & 1][0].data_ptr(), dev[k & 1][1].data_ptr(), on_device=True)

        def full(k):
            mat[box], rgb[box] = contents[k & 1], colours[k & 1]
            s.upload_voxels(mat, rgb)
            s.prepare()
        row = dict(grid=G, box=label, voxels=n ** 3, host=timed(edit_host, s.sync, a.reps, a.warmup), device=timed(edit_device, s.sync, a.reps, a.warmup),
                   upload_prepare=timed(full, s.sync, a.reps, a.warmup))
        print(json.dumps(row), flush=True)
        rows.append(row)
    for s, _, _ in sessions.values():
        s.close()
    fmt = lambda t: f"{t['median_ms']:.3f} ({t['p10_ms']:.3f}-{t['p90_ms']:.3f})"
    lines = ["# Cost of a voxel edit (tools/edit_cost.py)", "",
             f"One MI355X, one process, build {_lib.build_id()}; wall clock around a sync, ms: median (10th-90th percentile) of {rows[0]['host']['n']} repetitions "
             f"after {a.warmup}.  `upload + prepare` is the same change through vrt_upload_voxels + vrt_prepare (no sky).", "",
             "| grid | box | edit, host arrays | edit, device memory | upload + prepare | full / host edit |", "|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['grid']}^3 | {r['box']} | {fmt(r['host'])} | {fmt(r['device'])} | {fmt(r['upload_prepare'])} | "
                     f"{r['upload_prepare']['median_ms'] / r['host']['median_ms']:.1f}x |")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
