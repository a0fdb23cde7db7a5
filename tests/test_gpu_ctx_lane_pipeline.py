"""The pipeline shape a runtime with four hardware queues runs (csrc/vrt_plan.h, PipelineShape::ctx_lane): launches of half the
workgroup slots take turns over the library's two render streams AND the context's stream, the dispatch gate holds launch k until
launch k - 2 starts to drain, the grouped accumulation pass runs on the lane of its group's last launch, and the context's stream
is made to wait for the other lanes only where somebody looks at it or queues work on it.  Every variant of it -- the shape as
selected, switched off, with either pass placement, on a caller's stream that changes in mid-run, at 1080p -- renders what
isolated launches (VRT_OVERLAP=0) render, bit for bit: the HDR frame, both histories, g-buffer depth, normal, material, position.

Every GPU step is a process of its own under `timeout -k 10 300`, the steps of a run chained with `&&`, on the development build:
the switches are read when a context is created, the queue count when the runtime starts."""
import os
import shlex
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FRAMES = {"small": (320, 200, 6), "1080p": (1920, 1080, 8)}   # (small: 64 000 pixels -- at four queues the deep shape, the eight-deep one needs sixteen)
CALLS_A, CALLS_B, CALLS_C, CALLS_D = (4, 4, 1, 4, 4), (4, 4, 4), (4, 1, 4), (4, 4, 4, 4, 4)
FAIL_AT = len(CALLS_A) + len(CALLS_B) + len(CALLS_C)   # the launch after them (a call of up to four samples is one launch)
KNOBS = ("VRT_OVERLAP", "VRT_STREAMS", "VRT_PASS_STREAM", "VRT_GRID_DIV", "VRT_DEFER", "VRT_CTX_LANE", "VRT_TEST_FAIL_LAUNCH", "VRT_DEEP_ITEMS",
         "VRT_DEEPER_ITEMS", "VRT_DRAIN_GATE")
# the switches of each variant (development build): as selected; the lane off; the lane with the pass on the lane of the group's
# last launch; with every pass on the context's stream
VARIANTS = {
    "as_selected": {},
    "lane_off": {"VRT_CTX_LANE": "0"},
    "pass_on_last_lane": {"VRT_CTX_LANE": "1", "VRT_PASS_STREAM": "1"},
    "pass_on_context_stream": {"VRT_CTX_LANE": "1", "VRT_PASS_STREAM": "0"},
}


def _session(lib, W, H, depth):
    import orc
    from voxel_rt2_amd import host, scenes
    from voxel_rt2_amd._session import NativeSession
    mat, rgb, params = scenes.scene_s1(0)
    cfg = host.make_config(W, H, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=depth, seed=3)
    s = NativeSession(lib, "vrt_", cfg)
    orc.setup(s, mat, rgb, params)
    return s


def _state(s):
    from voxel_rt2_amd import _abi
    out = {"hdr": s.fetch_hdr()}
    for name, b in (("hist_d", _abi.BUF_HISTORY_DIFFUSE), ("hist_s", _abi.BUF_HISTORY_SPECULAR), ("depth", _abi.BUF_GBUF_DEPTH),
                    ("normal", _abi.BUF_GBUF_NORMAL), ("mat", _abi.BUF_GBUF_MAT), ("pos", _abi.BUF_GBUF_POSITION)):
        out[name] = s.fetch_buffer(b)
    return out


def _child_scenario(frame, out_path, inject):
    """One run of the scenario in this process (the environment carries the switches); the state goes to out_path."""
    import ctypes as C
    from voxel_rt2_amd import _lib
    W, H, depth = FRAMES[frame]
    lib = _lib.load_dev()
    if inject:
        os.environ["VRT_TEST_FAIL_LAUNCH"] = str(FAIL_AT)   # (read when the context is created)
    s = _session(lib, W, H, depth)
    os.environ.pop("VRT_TEST_FAIL_LAUNCH", None)
    for n in CALLS_A:
        s.accumulate(n)
    s.sync()
    for n in CALLS_B:
        s.accumulate(n)
    mid = s.fetch_hdr()
    for n in CALLS_C:
        s.accumulate(n)
    if inject:
        assert lib.vrt_accumulate(C.c_void_p(s._ctx), 4) == -2 and b"injected" in lib.vrt_last_error()
    for n in CALLS_D:
        s.accumulate(n)
    st = s.stats()
    out = _state(s)
    s.close()
    np.savez(out_path, mid=mid, flags=np.uint32(st["pipeline_flags"]), **out)
    print("scenario: ok")


def _child_caller_stream(out_path, overlapped):
    """The caller's stream as a lane: a copy of the frame and a kernel of the caller's behind six calls, five more calls, another
    stream of the caller's in mid-run, five more calls and a copy and a kernel on that one."""
    import torch
    from voxel_rt2_amd import _lib
    W, H, depth = FRAMES["small"]
    s = _session(_lib.load_dev(), W, H, depth)
    got = {}
    if overlapped:
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        bufs = [torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        s.set_stream(streams[0].cuda_stream)
        with torch.cuda.stream(streams[0]):
            for _ in range(6):       # a group of four launches and two launches still pending
                s.accumulate(4)
            s.fetch_hdr_device_async(bufs[0].data_ptr())
            got["after_6"] = bufs[0] * 1.0   # the caller's kernel, queued behind the library's work on this stream
            for _ in range(5):       # ... and the passes that write that frame's buffer again come behind the copy
                s.accumulate(4)
        s.set_stream(streams[1].cuda_stream)   # in mid-run: launches and a pass in flight on the stream that is given up
        with torch.cuda.stream(streams[1]):
            for _ in range(5):
                s.accumulate(4)
            s.fetch_hdr_device_async(bufs[1].data_ptr())
            got["after_16"] = bufs[1] * 1.0
        for st in streams:
            st.synchronize()
        got = {k: v.cpu().numpy() for k, v in got.items()}
        flags = s.stats()["pipeline_flags"]
    else:
        for done in range(1, 17):
            s.accumulate(4)
            if done in (6, 16):
                got[f"after_{done}"] = s.fetch_hdr()
        flags = s.stats()["pipeline_flags"]
    got.update(_state(s))
    s.close()
    np.savez(out_path, flags=np.uint32(flags), **got)
    print("caller stream: ok")


def _step(call, **env):
    """`timeout -k 10 300 python -c <call>` with four hardware queues and the switches in front: one GPU step."""
    code = f"import os, sys; sys.path[:0] = [{ROOT!r}, os.path.join({ROOT!r}, 'tests')]; import test_gpu_ctx_lane_pipeline as t; t.{call}"
    sets = " ".join(f"{k}={shlex.quote(v)}" for k, v in dict(env, GPU_MAX_HW_QUEUES="4").items())
    return f"env {sets} timeout -k 10 300 {shlex.quote(sys.executable)} -c {shlex.quote(code)}"


def _run(steps):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run(["bash", "-c", " && ".join(steps)], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]


def _same(a, b, what):
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        if k != "flags":
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


def _flags(run):
    f = int(run["flags"])
    return {"overlapped": f & 1, "depth": (f >> 2) & 7, "share": (f >> 5) & 7, "ctx_lane": (f >> 24) & 1}


@pytest.fixture(scope="module")
def isolated_small(tmp_path_factory):
    """The scenario with isolated launches (no launch fails in it): what every variant is compared with."""
    ref = str(tmp_path_factory.mktemp("ctx_lane_ref") / "ref.npz")
    _run([_step(f"_child_scenario('small', {ref!r}, False)", VRT_OVERLAP="0")])
    a = np.load(ref)
    assert _flags(a)["overlapped"] == 0
    # (the reference run is a picture, and one that moved on after the fetch in the middle)
    assert np.isfinite(a["hdr"]).all() and a["hdr"].mean() > 0.0 and not np.array_equal(a["mid"], a["hdr"])
    return a


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_variant_renders_what_isolated_launches_render(variant, isolated_small, tmp_path):
    got = str(tmp_path / "got.npz")
    _run([_step(f"_child_scenario('small', {got!r}, True)", **VARIANTS[variant])])
    b = np.load(got)
    f = _flags(b)
    print(variant, f)
    assert f["overlapped"] == 1 and f["depth"] == 1 and f["share"] == 2, "two streams of the pipeline's own, launches of half the slots"
    assert f["ctx_lane"] == (0 if variant == "lane_off" else 1), "bit 24: the context's stream is a render lane"
    _same(isolated_small, b, variant)


def test_the_callers_stream_is_the_lane_and_may_change_in_mid_run(tmp_path):
    ref, got = str(tmp_path / "ref.npz"), str(tmp_path / "got.npz")
    _run([_step(f"_child_caller_stream({ref!r}, False)", VRT_OVERLAP="0"),
          _step(f"_child_caller_stream({got!r}, True)")])
    a, b = np.load(ref), np.load(got)
    assert _flags(a)["overlapped"] == 0 and _flags(b)["overlapped"] == 1 and _flags(b)["ctx_lane"] == 1
    assert {"after_6", "after_16", "hdr"} <= set(a.files) and not np.array_equal(a["after_6"], a["after_16"])
    _same(a, b, "caller's stream")


def test_the_headline_frame(tmp_path):
    """1920 x 1080, 8 bounces: the launches of bench.py, through the same scenario."""
    ref, got = str(tmp_path / "ref.npz"), str(tmp_path / "got.npz")
    _run([_step(f"_child_scenario('1080p', {ref!r}, False)", VRT_OVERLAP="0"),
          _step(f"_child_scenario('1080p', {got!r}, True)")])
    a, b = np.load(ref), np.load(got)
    f = _flags(b)
    assert f["overlapped"] == 1 and f["depth"] == 1 and f["share"] == 2 and f["ctx_lane"] == 1
    _same(a, b, "1080p")
