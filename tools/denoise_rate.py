"""What vrt_denoise costs, next to the frame it cleans: milliseconds of one call and of one vrt_accumulate(4) step on the same context, on
one GPU, in one process.

    python tools/denoise_rate.py [--reps 9] [--warmup 3] [--width 1920] [--height 1080] [--iterations 5] [--out profiles/denoise_rate.jsonl]

The headline scene S1 at --width x --height, a static camera.  The device path: the result stays in device memory, wall clock around a
sync (so a call's figure holds its launches' and the sync's host cost, some tens of microseconds).  The two are ALTERNATED -- a step, a
denoise, a step, a denoise -- and each figure is the median of --reps repetitions after --warmup, with the 10th and 90th percentile.  The
rendering code behind vrt_accumulate is the yardstick: a denoiser that costs more than the frame it cleans is of little use.

As a floor, the bytes one iteration must move, from the plane sizes (voxel_rt2_amd/csrc/vrt_denoise.h): it reads a pixel's guide record
(16), material word (4) and two signals (16 each) and writes two signals (16 each) -- 84 bytes a pixel; the last iteration reads step 1's
signals too and writes the result (12) instead: 96.  Step 1 reads 52 and writes 52.  At 6.3 TB/s that is `floor_ms`; an iteration's own
time is taken as the difference between calls of k and of k - 1 iterations (the first holds step 1), and `floor_share` is floor / time.
Prints one JSON line and appends it to --out."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voxel_rt2_amd import _abi, _lib, host, materials, scenes  # noqa: E402
from voxel_rt2_amd._session import NativeSession  # noqa: E402
from radiance_rate import timed  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def floor_bytes(pixels, iterations):
    """[step 1, iteration 0, .., iteration n - 1]: the bytes each must move at least."""
    return [pixels * (52 + 52)] + [pixels * (96 if i == iterations - 1 else 84) for i in range(iterations)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "denoise_rate.jsonl"))
    a = ap.parse_args()
    import torch
    mat, rgb, params = scenes.SCENES["s1"](0)
    w, h = a.width, a.height
    s = NativeSession(_lib.load(), "vrt_", host.make_config(w, h, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=8, grid_res=mat.shape[0]))
    s.upload_voxels(mat, rgb)
    s.upload_materials(materials.load_table())
    s.set_scene(host.make_scene_params(**params))
    s.set_camera(host.default_camera(w, h))
    s.prepare()
    out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p = _abi.VrtDenoiseParams(iterations=a.iterations)
    steps, calls = [], []

    def both():                                        # a step, a denoise: alternated, each timed by itself
        steps.append(timed(lambda: s.accumulate(4), s.sync, 1, 0)[0])
        calls.append(timed(lambda: s.denoise(p, out), s.sync, 1, 0)[0])

    for _ in range(a.warmup + a.reps):
        both()
    steps, calls = sorted(steps[a.warmup:]), sorted(calls[a.warmup:])
    pick = lambda v: (v[len(v) // 2], v[len(v) // 10], v[(9 * len(v)) // 10])
    by_k = [timed(lambda k=k: s.denoise(_abi.VrtDenoiseParams(iterations=k), out), s.sync, a.reps, a.warmup)[0] for k in range(1, a.iterations + 1)]
    # an iteration as the LAST of its call does step 3 as well; what a call of k iterations adds to one of k - 1 is iteration k - 1 in full
    parts_ms = [by_k[0] * 1e3] + [(by_k[k] - by_k[k - 1]) * 1e3 for k in range(1, a.iterations)]
    fb = floor_bytes(w * h, a.iterations)
    floor_ms = [b / HBM_BYTES_PER_S * 1e3 for b in fb]
    result = out.cpu().numpy()
    row = dict(tool="denoise_rate", build=_lib.build_id(), scene="s1", width=w, height=h, iterations=a.iterations,
               denoise_ms=pick(calls)[0] * 1e3, denoise_p10_ms=pick(calls)[1] * 1e3, denoise_p90_ms=pick(calls)[2] * 1e3,
               step_ms=pick(steps)[0] * 1e3, step_p10_ms=pick(steps)[1] * 1e3, step_p90_ms=pick(steps)[2] * 1e3,
               denoise_to_step=pick(calls)[0] / pick(steps)[0],
               calls_of_k_iterations_ms=[t * 1e3 for t in by_k],
               first_iteration_with_step1_ms=parts_ms[0], later_iterations_ms=parts_ms[1:],
               floor_bytes=fb, floor_ms=floor_ms, floor_total_ms=sum(floor_ms),
               floor_share_first_with_step1=(floor_ms[0] + floor_ms[1]) / parts_ms[0] if parts_ms[0] > 0 else None,
               floor_share_later=[floor_ms[1 + k] / parts_ms[k] if parts_ms[k] > 0 else None for k in range(1, a.iterations)],
               floor_share_call=sum(floor_ms) / (pick(calls)[0] * 1e3),
               mean_rgb=[float(x) for x in result.reshape(-1, 3).mean(axis=0)], finite=bool((result == result).all()))
    s.close()
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
