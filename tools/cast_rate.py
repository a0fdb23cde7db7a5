"""How fast vrt_cast_rays answers: Mrays/s from device-resident rays, for batches of 1 to 16 M rays, on one GPU, in one process.

    python tools/cast_rate.py [--reps 15] [--warmup 3] [--max-n 16777216] [--out profiles/cast_rate.md] > lines.jsonl

Scenes s1, dense and s1_256; per scene three sets of rays -- the 1080p camera rays of the reference's initial pose (coherent), the same
rays shuffled, and random rays in and around the world box -- each as closest-hit and as any-hit rays, on both instantiations of the
kernel (coarse pyramid levels staged in LDS / everything through global memory, forced with the development build's VRT_CAST_VIEW) and,
for n up to 4096, through the host path as the shipped switch-over picks.  Wall clock around a sync, the median of --reps repetitions
after --warmup with the 10th and 90th percentile; a run's spread is what a difference has to exceed to mean something.
Prints one JSON line per measurement, then per scene the smallest n from which the staged kernel stays ahead of the global-memory one
by more than both spreads (the switch-over VRT_CAST_STAGED_MIN of vrt_plan.h is read off s1's), and writes the table."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voxel_rt2_amd import _abi, _lib, camera as cam_mod, host, materials, scenes  # noqa: E402
from voxel_rt2_amd._session import NativeSession  # noqa: E402

SCENES = ("s1", "dense", "s1_256")
NS = [1, 64, 256, 1024, 4096, 16384, 65536, 262144, 1 << 20, 1 << 22, 1 << 24]


def camera_rays(w=1920, h=1080):
    """get_cast_dir (pathtracer.py:293-312) without jitter for every pixel, row by row; not bit-exact, this is a workload."""
    view, proj = cam_mod.default_matrices(w, h)
    vi, pi = np.linalg.inv(view.astype(np.float64)), np.linalg.inv(proj.astype(np.float64))
    u, v = np.meshgrid((np.arange(w) + 0.5) / w * 2 - 1, (np.arange(h) + 0.5) / h * 2 - 1)
    p = np.stack([u, v, np.ones_like(u), np.ones_like(u)], axis=-1).reshape(-1, 4) @ pi.T
    d = p[:, :3] / p[:, 3:]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros(w * h, _abi.RAY)
    rays["origin"], rays["dir"], rays["t_max"] = cam_mod.DEFAULT_POS, d @ vi[:3, :3].T, np.inf
    return rays


def random_rays(n, seed=1):
    rng = np.random.default_rng(seed)
    rays = np.zeros(n, _abi.RAY)
    d = rng.standard_normal((n, 3)).astype(np.float32)
    rays["origin"], rays["dir"], rays["t_max"] = rng.uniform(-1.5, 1.5, (n, 3)), d / np.linalg.norm(d, axis=1, keepdims=True), np.inf
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


def session(lib, name, view):
    if view:
        os.environ["VRT_CAST_VIEW"] = view          # read when the context is created (development build only)
    else:
        os.environ.pop("VRT_CAST_VIEW", None)
    mat, rgb, params = scenes.SCENES[name](0)
    s = NativeSession(lib, "vrt_", host.make_config(64, 48, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=4, grid_res=mat.shape[0]))
    s.upload_voxels(mat, rgb)
    s.upload_materials(materials.load_table())
    s.set_scene(host.make_scene_params(**params))
    s.set_camera(host.default_camera(64, 48))
    s.prepare()
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-n", type=int, default=1 << 24)
    ap.add_argument("--out", default=os.path.join("profiles", "cast_rate.md"))
    a = ap.parse_args()
    import torch
    ns = [n for n in NS if n <= a.max_n]
    cam = camera_rays()
    sets = {"coherent": cam, "shuffled": cam[np.random.default_rng(2).permutation(len(cam))], "random": random_rays(len(cam))}
    dev = {}
    for k, r in sets.items():                          # device copies, tiled up to the largest batch
        t = torch.from_numpy(r.view(np.uint8).reshape(-1)).cuda()
        dev[k] = t.repeat(-(-ns[-1] // len(r)))[:ns[-1] * 32].contiguous()
    flagged = {k: t.clone() for k, t in dev.items()}
    for t in flagged.values():
        t.view(torch.int32)[7::8] = _abi.RAY_ANY_HIT
    hits = torch.zeros(ns[-1] * 48, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rows = []
    lib = _lib.load_dev()                              # (without VRT_CAST_VIEW it picks the view as the shipped library does)
    for name in SCENES:
        for view in ("staged", "global", ""):
            s = session(lib, name, view)
            for work in sets:
                for any_hit in (False, True):
                    src = flagged[work] if any_hit else dev[work]
                    host_rays = sets[work].copy()
                    host_rays["flags"] = int(any_hit)
                    for n in ns:
                        if view:
                            fn = lambda: s.cast_rays(src, hits, n=n)
                        elif n <= 4096:
                            fn = lambda: s.cast_rays(host_rays[:n])
                        else:
                            continue
                        med, lo, hi = timed(fn, s.sync, a.reps if n < (1 << 22) else max(5, a.reps // 3), a.warmup)
                        row = dict(scene=name, view=view or "host path", rays=work, any_hit=any_hit, n=n, median_us=med * 1e6, p10_us=lo * 1e6, p90_us=hi * 1e6,
                                   mrays_per_s=n / med * 1e-6)
                        print(json.dumps(row), flush=True)
                        rows.append(row)
            s.close()
    os.environ.pop("VRT_CAST_VIEW", None)
    get = {(r["scene"], r["view"], r["rays"], r["any_hit"], r["n"]): r for r in rows}
    crossing = {}
    for name in SCENES:
        for work in sets:
            ahead = [n for n in ns if get[name, "staged", work, False, n]["p90_us"] < get[name, "global", work, False, n]["p10_us"]]
            tail = next((n for i, n in enumerate(ns) if all(m in ahead for m in ns[i:])), None)
            crossing[f"{name}/{work}"] = tail
    print(json.dumps(dict(staged_ahead_from=crossing)), flush=True)
    lines = ["# vrt_cast_rays: rays per second (tools/cast_rate.py)", "",
             f"One MI355X, one process, build {_lib.build_id()}; device-resident rays, wall clock around a sync, Mrays/s from the median of {a.reps} repetitions "
             f"(a third of that from 4 M rays on) after {a.warmup}; in brackets the 10th-90th percentile of the time as a share of the median.  "
             "`LDS` / `global`: the two instantiations of k_cast_rays; `host` the host path (staging and copies included).", "",
             "Smallest n from which the staged kernel stays ahead by more than both spreads, closest hit: " +
             ", ".join(f"{k}: {v}" for k, v in crossing.items()) + ".", ""]
    for name in SCENES:
        lines += [f"## {name}", "", "| n | " + " | ".join(f"{w} {'any' if ah else 'closest'}: LDS / global / host" for w in sets for ah in (False, True)) + " |",
                  "|---|" + "---|" * (2 * len(sets))]
        for n in ns:
            cells = []
            for w in sets:
                for ah in (False, True):
                    part = []
                    for view in ("staged", "global", "host path"):
                        r = get.get((name, view, w, ah, n))
                        part.append("-" if r is None else f"{r['mrays_per_s']:.3g} ({(r['p90_us'] - r['p10_us']) / r['median_us'] * 100:.0f} %)")
                    cells.append(" / ".join(part))
            lines.append(f"| {n} | " + " | ".join(cells) + " |")
        lines.append("")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
