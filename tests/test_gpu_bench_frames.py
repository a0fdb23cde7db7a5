"""The frames bench.py times, against the CPU oracle bit for bit.

The other GPU-vs-oracle tests at these frame sizes render one call on a fresh context; the benchmark makes many calls with the
launch pipeline in flight (buffer sets in rotation, timed launches one in eight, camera rays shared by fused samples, running
means over every call).  Here the frames of those schedules -- bench.py's own plain run and its two-rank rehearsal, configs 4
and 5 replayed the way bench.py --full runs them (in both indexing modes), and the Scene API's one-sample loop -- are compared
with oracle row bands (tests/bands.py; tests/test_oracle_bands.py pins that a band is the whole frame's rows).  Every
comparison has a negative control: the same band after one call fewer and one call more must differ."""
import json
import os
import re
import socket
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import bands
import orc
from voxel_rt2_amd import _abi, _lib, host, scenes
from voxel_rt2_amd._session import NativeSession

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH_SETUP_CALLS = 4   # ShardedRun.timed / run_secondary: calls before the warm-up


def run_bench(args, timeout, ranks=1, **env_extra):
    """bench.py in a child process (it sets GPU_MAX_HW_QUEUES at import: never imported here).  Returns (the JSON line, stderr)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(env_extra)
    bench_py = os.path.join(ROOT, "bench.py")
    if ranks == 1:
        cmd = [sys.executable, bench_py, "--gpus", "1", *args]
    else:
        sock = socket.socket()
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
        sock.close()
        env["MASTER_ADDR"] = "127.0.0.1"
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
               "--master-port", str(port), bench_py, "--gpus", str(ranks), *args]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), r.stderr


def check_bands(frame, scene, calls, band_rows, what, *, depth, seed, grid=128, ref_indexing=False, bufs=None, extra_call=None):
    """frame: the GPU's whole HDR frame after `calls` (tests/bands.py's call list).  Every band of rows equals the oracle's after
    the same calls; the bands together differ from the oracle's after one call fewer and after one call more (`extra_call`, by
    default the last call again).  bufs: {buffer id: the GPU's whole buffer}, compared on the same rows after the same calls.
    Returns {band: the oracle's HDR rows}."""
    H, W = frame.shape[:2]
    n = len(calls)
    script = list(calls) + [extra_call if extra_call is not None else calls[-1]]
    got, fewer, more, out = [], [], [], {}
    for rows in band_rows:
        assert 0 <= rows[0] < rows[1] <= H, rows
        ref = bands.oracle_band(scene, W, H, rows, script, [n - 1, n, n + 1], depth=depth, seed=seed, grid=grid,
                                ref_indexing=ref_indexing, bufs=tuple(bufs or ()), bufs_at=n)
        band = frame[rows[0]:rows[1]]
        bands.assert_rows_equal(band, ref[n][0], rows[0], f"{what}: HDR rows {rows} after {n} calls")
        for b, whole in (bufs or {}).items():
            bands.assert_rows_equal(whole[rows[0]:rows[1]], ref[n][1][b], rows[0], f"{what}: buffer {b}, rows {rows}")
        got.append(band)
        fewer.append(ref[n - 1][0])
        more.append(ref[n + 1][0])
        out[rows] = ref[n][0]
    bands.assert_rows_differ(np.concatenate(got), np.concatenate(fewer), f"{what}: after {n - 1} calls")
    bands.assert_rows_differ(np.concatenate(got), np.concatenate(more), f"{what}: after {n + 1} calls")
    return out


def s1_scene():
    return scenes.scene_s1(0)


# ---- a. the headline: bench.py's plain run ---------------------------------------------------------------------------------------
def test_headline_bench_frame_matches_oracle(tmp_path):
    """bench.py --gpus 1 with 4 + 2 + 12 calls of 4 samples: every buffer set of the launch pipeline comes round several times and
    at least two launches carry timers (one in eight).  Bands: the first and the last rows, one across row 540, one through S1's horizon, one off the
    8x8 wave-tile grid inside the voxels."""
    steps, warmup = 12, 2
    out, _ = run_bench(["--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path)], timeout=600)
    cfg = out["config"]
    W, H, spp, depth, seed = cfg["width"], cfg["height"], cfg["spp_per_step"], cfg["max_depth"], cfg["seed"]
    assert cfg["launch_pipeline"]["overlapped"] is True, cfg["launch_pipeline"]
    assert out["steps"] == steps and out["warmup"] == warmup
    n = BENCH_SETUP_CALLS + warmup + steps
    assert n >= 16
    hdr = np.load(tmp_path / "hdr.npy")
    assert hdr.shape == (H, W, 3) and np.isfinite(hdr).all()
    mid = H // 2
    band_rows = [(0, 8), (H - 8, H), (mid - 4, mid + 4), (H * 748 // 1080, H * 748 // 1080 + 16), (H * 613 // 1080, H * 613 // 1080 + 9)]
    check_bands(hdr, s1_scene(), [spp] * n, band_rows, "bench.py headline", depth=depth, seed=seed)


# ---- b. the two-rank rehearsal: the HDR-target ring and the gather, against the oracle ------------------------------------------
@pytest.mark.parametrize("stripes", [0, 32])
def test_two_rank_rehearsal_frame_matches_oracle(tmp_path, stripes):
    """VRT_BENCH_REHEARSE=1, two ranks on one GPU: the frame rank 0 assembles from the last gathered tiles (written by the
    temporal pass into the ring of vrt_set_hdr_targets).  Contiguous tiles: a band across the balanced boundary and the last rows.
    32-row stripes: bands across stripe edges, and the short last stripe (1080 = 33 x 32 + 24).  4 + 2 + 5 calls: the ring of
    eight HDR targets comes round."""
    steps, warmup = 5, 2
    out, err = run_bench(["--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path)], timeout=600, ranks=2,
                         VRT_BENCH_REHEARSE="1", VRT_BENCH_STRIPES=str(stripes))
    assert "[rehearsal] config 2: gathered frame == unsharded frame: True" in err, err[-3000:]
    cfg = out["config"]
    W, H, spp, depth, seed = cfg["width"], cfg["height"], cfg["spp_per_step"], cfg["max_depth"], cfg["seed"]
    assert out["n_gpus"] == 2
    tile_rows = [int(x) for x in re.search(r"tile rows \[([0-9, ]+)\]", cfg["sharding"]).group(1).split(",")]
    assert sum(tile_rows) == H and len(tile_rows) == 2
    if stripes:
        assert f"interleaved {stripes}-row stripes" in cfg["sharding"]
        last = (H // stripes) * stripes
        assert 0 < H - last < stripes
        band_rows = [(stripes - 4, stripes + 4), (3 * stripes - 4, 3 * stripes + 5), (last - 4, last + 4), (H - 8, H)]
    else:
        b = tile_rows[0]
        assert 8 <= b <= H - 8
        band_rows = [(b - 4, b + 4), (H - 8, H)]
    hdr = np.load(tmp_path / "hdr.npy")
    assert hdr.shape == (H, W, 3) and np.isfinite(hdr).all()
    n = BENCH_SETUP_CALLS + warmup + steps
    check_bands(hdr, s1_scene(), [spp] * n, band_rows, f"two-rank rehearsal, stripes {stripes}", depth=depth, seed=seed)


# ---- c. configs 4 and 5 in their one-GPU form, both indexing modes ---------------------------------------------------------------
def secondary_cases():
    """bench.SECONDARY and bench.SEED, read in a child process (importing bench.py sets GPU_MAX_HW_QUEUES)."""
    code = (f"import json, sys; sys.path[:0] = [{ROOT!r}]; import bench; "
            "print(json.dumps(dict(cases=bench.SECONDARY, seed=bench.SEED)))")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


GBUF = (_abi.BUF_GBUF_DEPTH, _abi.BUF_GBUF_NORMAL, _abi.BUF_GBUF_POSITION, _abi.BUF_GBUF_MAT)
HIST = (_abi.BUF_HISTORY_DIFFUSE, _abi.BUF_HISTORY_SPECULAR)


@pytest.mark.parametrize("prefix", ["config4", "config5"])
def test_secondary_4k_config_matches_oracle(prefix):
    """run_secondary's flow through the library on the whole 3840x2160 frame: its scene and seed, the sky off, 4 set-up calls and
    `steps` calls of accumulate(spp) -- once in the default mode and once with vrt_set_reference_indexing.  HDR, both histories
    (w = the sample count) and the g-buffer on the first, a middle and the last rows.  The oracle's two modes differ inside
    these bands, so the reference-mode comparison cannot pass on a library that ignores the mode."""
    info = secondary_cases()
    case = next(c for c in info["cases"] if c["name"].startswith(prefix))
    W, H, spp, depth, grid = case["W"], case["H"], case["spp"], case["depth"], case.get("grid", 128)
    assert not case.get("sky_res") and not case.get("restir")
    mat, rgb, params = scenes.SCENES[case["scene"]](12345 if case["scene"].startswith("dense") else 0)
    params = dict(params, use_physical_sky=0, use_clouds=0)
    scene = (mat, rgb, params)
    n = BENCH_SETUP_CALLS + case["steps"]
    band_rows = [(0, 8), (H // 2 + 8, H // 2 + 16), (H - 8, H)]
    oracle = {}
    for ref in (False, True):
        cfg = host.make_config(W, H, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=depth, seed=info["seed"],
                               grid_res=grid)
        g = NativeSession(_lib.load(), "vrt_", cfg)
        orc.setup(g, mat, rgb, params, cam=host.default_camera(W, H, jitter_index=1))
        if ref:
            g.set_reference_indexing(True)
        for _ in range(n):
            g.accumulate(spp)
        g.sync()
        hdr = g.fetch_hdr()
        bufs = {b: g.fetch_buffer(b) for b in GBUF + HIST}
        g.close()
        assert np.isfinite(hdr).all()
        for b in HIST:
            assert (bufs[b][..., 3] == n * spp).all(), f"buffer {b}: history weight is not the sample count {n * spp}"
        oracle[ref] = check_bands(hdr, scene, [spp] * n, band_rows, f"{case['name']}, reference indexing {ref}", depth=depth,
                                  seed=info["seed"], grid=grid, ref_indexing=ref, bufs=bufs)
    for rows in band_rows:
        assert bands.first_difference(oracle[True][rows], oracle[False][rows]) is not None, \
            f"{case['name']}: the indexing modes do not differ on rows {rows}"


# ---- d. the Scene API's loop shape: one sample per call, a new jitter every frame ------------------------------------------------
SCENE_API_W, SCENE_API_H, SCENE_API_CALLS = 1920, 1080, 20


def scene_api_calls(n):
    """bench.py's scene_api_default: frame k sets the camera of jitter index k % 16 + 1, one sample, end_frame."""
    cams = [host.default_camera(SCENE_API_W, SCENE_API_H, jitter_index=k + 1) for k in range(16)]
    return [(1, cams[k % 16]) for k in range(n)]


def _render_scene_api_loop(out_path):
    """The body of test_scene_api_loop_matches_oracle's child process: the frame and the pipeline flags."""
    mat, rgb, params = s1_scene()
    cfg = host.make_config(SCENE_API_W, SCENE_API_H, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=8, seed=0)
    s = NativeSession(_lib.load(), "vrt_", cfg)
    orc.setup(s, mat, rgb, params, cam=host.default_camera(SCENE_API_W, SCENE_API_H, jitter_index=1))
    bands.play(s, scene_api_calls(SCENE_API_CALLS))
    s.sync()
    np.save(out_path, s.fetch_hdr())
    flags = s.stats()["pipeline_flags"]
    s.close()
    print(json.dumps(dict(flags=flags, queues=os.environ.get("GPU_MAX_HW_QUEUES"))))


def test_scene_api_loop_matches_oracle(tmp_path):
    """20 one-sample calls on S1 at 1080p, cycling through the 16 jittered cameras with end_frame after each: in a child process
    started without GPU_MAX_HW_QUEUES, so that the library asks for sixteen queues and one-sample launches run eight deep on a
    quarter of the workgroup slots each -- the pipeline scene_api_default times."""
    out_path = tmp_path / "hdr.npy"
    code = textwrap.dedent("""
        import os, sys
        sys.path[:0] = [%r, os.path.join(%r, "tests")]
        import test_gpu_bench_frames
        test_gpu_bench_frames._render_scene_api_loop(%r)
    """) % (ROOT, ROOT, str(out_path))
    env = {k: v for k, v in os.environ.items() if k not in ("GPU_MAX_HW_QUEUES", "VRT_OVERLAP", "VRT_RENDER")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    info = json.loads(r.stdout.strip().splitlines()[-1])
    flags = info["flags"]
    assert info["queues"] == "16", info
    assert flags & 1 == 1 and (flags >> 2) & 7 == 4 and (flags >> 5) & 7 == 4, f"not eight launches of a quarter in flight: {flags:#x}"
    hdr = np.load(out_path)
    H = SCENE_API_H
    calls = scene_api_calls(SCENE_API_CALLS + 1)
    check_bands(hdr, s1_scene(), calls[:-1], [(H // 2 - 4, H // 2 + 4), (H * 613 // 1080, H * 613 // 1080 + 9), (H - 8, H)],
                "Scene API loop", depth=8, seed=0, extra_call=calls[-1])
