"""What vrt_sweep_boxes costs: boxes per second on one GPU, in one process, next to vrt_cast_rays on the same number of rays.

    python tools/sweep_rate.py [--reps 9] [--warmup 3] [--out profiles/sweep_rate.jsonl]

The headline scene S1 and the dense scene, 128^3.  The box is 7^3 voxels, its lower corner uniform over the solids' bounds grown by 8
voxels, moved by 1 voxel and by 16 voxels in a uniformly random direction (t_max = 1); batches of 1 024 and 262 144 boxes.  The device
path: records and results stay in device memory, wall clock around a sync (so a small batch's figure is the launch's and the sync's host
cost).  In the same run, vrt_cast_rays on as many rays from the boxes' centres along their moves (t_max = inf), for scale.  Each figure is
the median of --reps repetitions after --warmup, with the 10th and 90th percentile.  One JSON line per configuration is printed and
appended to --out."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voxel_rt2_amd import _abi, _lib, host, materials, scenes  # noqa: E402
from voxel_rt2_amd._session import NativeSession  # noqa: E402
from radiance_rate import timed  # noqa: E402

BOX_VOXELS = 7


def records(mat, n, move_voxels, seed):
    """(boxes, rays): n boxes of BOX_VOXELS^3 voxels around the scene's solids, each moved by move_voxels, and the rays along their moves."""
    G = mat.shape[0]
    dx = 2.0 / G
    rng = np.random.default_rng(seed)
    solid = np.argwhere(mat > 0)
    lo_b, hi_b = np.maximum(solid.min(axis=0) - 8, 0), np.minimum(solid.max(axis=0) + 9, G)
    lo = rng.uniform(lo_b, hi_b - BOX_VOXELS, (n, 3))
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    boxes = np.zeros(n, _abi.BOX_SWEEP)
    boxes["lo"], boxes["hi"], boxes["move"], boxes["t_max"] = lo * dx - 1.0, (lo + BOX_VOXELS) * dx - 1.0, d * (move_voxels * dx), 1.0
    rays = np.zeros(n, _abi.RAY)
    rays["origin"], rays["dir"], rays["t_max"] = (lo + BOX_VOXELS / 2) * dx - 1.0, d, np.inf
    return boxes, rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "sweep_rate.jsonl"))
    a = ap.parse_args()
    import torch
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    for name in ("s1", "dense"):
        mat, rgb, params = scenes.SCENES[name](0)
        s = NativeSession(_lib.load(), "vrt_", host.make_config(64, 64, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=2, grid_res=mat.shape[0]))
        s.upload_voxels(mat, rgb)
        s.upload_materials(materials.load_table())
        s.set_scene(host.make_scene_params(**params))
        s.set_camera(host.default_camera(64, 64))
        s.prepare()
        for n in (1 << 10, 1 << 18):
            for move_voxels in (1, 16):
                boxes, rays = records(mat, n, move_voxels, [7, n, move_voxels])
                t_boxes, t_rays = (torch.from_numpy(r.view(np.uint8).reshape(-1)).cuda() for r in (boxes, rays))
                t_hits = torch.zeros(n * _abi.SWEEP_HIT.itemsize, dtype=torch.uint8, device="cuda")
                t_ray_hits = torch.zeros(n * _abi.HIT.itemsize, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                sweep = timed(lambda: s.sweep_boxes(t_boxes, t_hits), s.sync, a.reps, a.warmup)
                cast = timed(lambda: s.cast_rays(t_rays, t_ray_hits), s.sync, a.reps, a.warmup)
                kinds = np.bincount(t_hits.cpu().numpy().view(_abi.SWEEP_HIT)["kind"], minlength=4)
                row = dict(tool="sweep_rate", build=_lib.build_id(), scene=name, grid_res=int(mat.shape[0]), solids=int((mat > 0).sum()), boxes=n,
                           box_voxels=BOX_VOXELS, move_voxels=move_voxels, sweep_ms=sweep[0] * 1e3, sweep_p10_ms=sweep[1] * 1e3, sweep_p90_ms=sweep[2] * 1e3,
                           boxes_per_s=n / sweep[0], cast_ms=cast[0] * 1e3, cast_p10_ms=cast[1] * 1e3, cast_p90_ms=cast[2] * 1e3, rays_per_s=n / cast[0],
                           sweep_to_cast=sweep[0] / cast[0], kinds=dict(miss=int(kinds[0]), floor=int(kinds[1]), voxel=int(kinds[2]), start=int(kinds[3])))
                line = json.dumps(row)
                print(line, flush=True)
                with open(a.out, "a") as fh:
                    fh.write(line + "\n")
        s.close()


if __name__ == "__main__":
    main()
