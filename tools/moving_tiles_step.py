#!/usr/bin/env python3
"""Step time of the reference's moving-camera loop (scene.py:206-262: set_camera_is_moving, render scale 0.5, one sample per
accumulate call, a new pose every step) at 1080p on scene S1, 8 bounces: one whole-frame context against two row tiles of the
same frame on the same GPU with the history exchange between them (parallel.exchange_history's all-gather, played in-process
through a device tensor).  The tiles run one after the other on one GPU, so their time is the sum of two ranks' work plus the
exchange, not what two GPUs would take; the exchange part is reported alone too.
    python tools/moving_tiles_step.py [--steps N] [--warmup N]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from voxel_rt2_amd import _lib, camera, host, parallel, scenes  # noqa: E402  (the library before torch: _lib.load())
from voxel_rt2_amd._session import NativeSession  # noqa: E402

W, H, DEPTH = 1920, 1080, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import json
    import orc
    import torch
    lib = _lib.load()
    mat, rgb, params = scenes.scene_s1(0)

    def context(rows=None):
        cfg = host.make_config(W, H, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=DEPTH, seed=1, rows=rows)
        s = NativeSession(lib, "vrt_", cfg)
        orc.setup(s, mat, rgb, params)
        if rows is not None:
            parallel.enable_moving_camera(s)
        return s

    def pose(k):
        pos = (0.4 + 0.002 * k, 0.5, 2.0)
        view, proj = camera.default_matrices(W, H, pos=pos, look=(0.0, 0.001 * k, 0.0))
        return host.make_camera(view, proj, pos, jitter_index=k + 1, moving=True, render_scale=0.5, max_accum_frames=50.0)

    bounds = parallel.split_rows(H, 2)
    rows = max(b - a for a, b in bounds)
    full = torch.empty((2, rows * parallel.HISTORY_BYTES_PER_PIXEL * W), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    exch_s = [0.0]

    def exchange(tiles):
        for s in tiles:   # (the step's passes first: what follows is the exchange alone)
            s.sync()
        t0 = time.perf_counter()
        for r, s in enumerate(tiles):
            s.history_rows_io(*bounds[r], full[r].data_ptr(), False)
        for s in tiles:
            s.sync()
        for r, s in enumerate(tiles):
            s.history_rows_io(*bounds[1 - r], full[1 - r].data_ptr(), True)
        for s in tiles:
            s.sync()
        exch_s[0] += time.perf_counter() - t0

    def run(sessions, tiled):
        for s in sessions:
            s.accumulate(1)
            s.end_frame()
        if tiled:
            exchange(sessions)
        t = None
        for k in range(args.warmup + args.steps):
            if k == args.warmup:
                for s in sessions:
                    s.sync()
                exch_s[0] = 0.0
                t = time.perf_counter()
            for s in sessions:
                s.set_camera(pose(k))
                s.accumulate(1)
                s.end_frame()
            if tiled:
                exchange(sessions)   # (synchronises every step, as the all-gather of a real run does)
            else:
                sessions[0].sync()   # (the same per-step synchronisation: the reference presents every frame)
        for s in sessions:
            s.sync()
        return (time.perf_counter() - t) / args.steps * 1e3

    whole_ms = run([context()], False)
    tiles_ms = run([context(b) for b in bounds], True)
    print(json.dumps({"W": W, "H": H, "render_scale": 0.5, "steps": args.steps, "whole_frame_ms_per_step": round(whole_ms, 3),
                      "two_tiles_plus_exchange_ms_per_step": round(tiles_ms, 3),
                      "of_which_exchange_ms_per_step": round(exch_s[0] / args.steps * 1e3, 3),
                      "bytes_imported_per_tile_per_step": parallel.HISTORY_BYTES_PER_PIXEL * W * rows}))


if __name__ == "__main__":
    main()
