"""How fast vrt_trace_radiance answers, next to the render kernel that walks the same paths: path-samples/s on one GPU, in one process.

    python tools/radiance_rate.py [--reps 9] [--warmup 3] [--samples 4] [--depth 8] [--out profiles/radiance_rate.jsonl]

The 1920 x 1080 camera rays of the headline scene S1 (the reference's initial pose, no jitter: a workload, not a parity check), device
resident, `--samples` samples a ray at `--depth` bounces through the device path: wall clock around a sync, the median of --reps
repetitions after --warmup with the 10th and 90th percentile.  Next to it the same context -- created with VRT_RENDER=fused, so its frames
come from k_render, which like k_trace_radiance keeps one path per lane and refills between segments -- rendering that frame with
accumulate(samples): wall clock per call (render launch and accumulation pass), and the render kernel's own device time from
vrt_get_stats.  Prints one JSON line and appends it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["VRT_RENDER"] = "fused"                     # read when the context is created
from voxel_rt2_amd import _abi, _lib, camera as cam_mod, host, materials, scenes  # noqa: E402
from voxel_rt2_amd._session import NativeSession  # noqa: E402

W, H = 1920, 1080


def camera_rays():
    """get_cast_dir (pathtracer.py:293-312) without jitter for every pixel, row by row, stream = v * W + u."""
    view, proj = cam_mod.default_matrices(W, H)
    vi, pi = np.linalg.inv(view.astype(np.float64)), np.linalg.inv(proj.astype(np.float64))
    u, v = np.meshgrid((np.arange(W) + 0.5) / W * 2 - 1, (np.arange(H) + 0.5) / H * 2 - 1)
    p = np.stack([u, v, np.ones_like(u), np.ones_like(u)], axis=-1).reshape(-1, 4) @ pi.T
    d = p[:, :3] / p[:, 3:]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros(W * H, _abi.PATH_RAY)
    rays["origin"], rays["dir"], rays["stream"] = cam_mod.DEFAULT_POS, d @ vi[:3, :3].T, np.arange(W * H)
    return rays


def timed(fn, sync, reps, warmup):
    out = []
    for k in range(warmup + reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if k >= warmup:
            out.append(time.perf_counter() - t0)
    out.sort()
    return statistics.median(out), out[len(out) // 10], out[(9 * len(out)) // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--out", default=os.path.join("profiles", "radiance_rate.jsonl"))
    a = ap.parse_args()
    import torch
    mat, rgb, params = scenes.SCENES["s1"](0)
    s = NativeSession(_lib.load(), "vrt_", host.make_config(W, H, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=a.depth,
                                                            grid_res=mat.shape[0]))
    s.upload_voxels(mat, rgb)
    s.upload_materials(materials.load_table())
    s.set_scene(host.make_scene_params(**params))
    s.set_camera(host.default_camera(W, H))
    s.prepare()
    t_rays = torch.from_numpy(camera_rays().view(np.uint8).reshape(-1)).cuda()
    t_out = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    paths = W * H * a.samples
    q = timed(lambda: s.trace_radiance(t_rays, a.samples, 0, t_out), s.sync, a.reps, a.warmup)
    f = timed(lambda: s.accumulate(a.samples), s.sync, a.reps, a.warmup)
    st = s.stats()
    kernel_s = st["render_ms"] * 1e-3 / max(st["render_launches"], 1)
    row = dict(tool="radiance_rate", build=_lib.build_id(), scene="s1", width=W, height=H, samples=a.samples, depth=a.depth, paths=paths,
               query_ms=q[0] * 1e3, query_p10_ms=q[1] * 1e3, query_p90_ms=q[2] * 1e3, query_paths_per_s=paths / q[0],
               fused_call_ms=f[0] * 1e3, fused_call_p10_ms=f[1] * 1e3, fused_call_p90_ms=f[2] * 1e3, fused_call_paths_per_s=paths / f[0],
               fused_kernel_ms=kernel_s * 1e3, fused_kernel_paths_per_s=paths / kernel_s if kernel_s > 0 else None,
               ratio_to_fused_call=f[0] / q[0], ratio_to_fused_kernel=kernel_s / q[0] if kernel_s > 0 else None,
               mean_rgb=[float(x) for x in t_out.view(-1, 4)[:, :3].mean(dim=0).cpu()])
    s.close()
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
