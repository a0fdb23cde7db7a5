"""The shapes of the pipeline of half-size launches (csrc/vrt_plan.h, plan_pipeline_shape): four render streams with the grouped
accumulation pass on the context's stream (what runs where the runtime has six hardware queues or more), two render streams
without the dispatch gate's stream wait (what runs where it has fewer), and the shapes the development build can force beside
them: three render streams, the pass on the render stream of the group's last launch.  Every shape renders
what isolated launches (VRT_OVERLAP=0) render, bit for bit, through a run that mixes four-sample and one-sample calls, a
synchronisation, a fetch in the middle and a launch that fails to queue; and work a caller queues on its own stream after
vrt_accumulate still finds the finished frame.

Every GPU step is a process of its own under `timeout -k 10`, the steps of a test chained with `&&`: the switches are read when a
context is created, the queue count when the runtime starts."""
import os
import shlex
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# VRT_STREAMS, VRT_PASS_STREAM of the development build (read_knobs)
SHAPES = {
    "four_streams_pass_on_context_stream": ("4", "0"),
    "four_streams_pass_on_render_stream": ("4", "1"),
    "three_streams_pass_on_render_stream": ("3", "1"),
    "two_streams_pass_on_context_stream": ("2", "0"),
    "two_streams_pass_on_render_stream": ("2", "1"),
}
FRAMES = {"small": (320, 200, 6), "1080p": (1920, 1080, 8)}
CALLS_A, CALLS_B, CALLS_C, CALLS_D = (4, 4, 1, 4, 4), (4, 4, 4), (4, 1, 4), (4, 4, 4, 4, 4)
FAIL_AT = len(CALLS_A) + len(CALLS_B) + len(CALLS_C)   # the launch after them (a call of up to four samples is one launch)


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
    """The caller's stream: a copy of the frame and a kernel of the caller's behind vrt_accumulate, then more calls at once."""
    import torch
    from voxel_rt2_amd import _lib
    W, H, depth = FRAMES["1080p"]
    s = _session(_lib.load_dev(), W, H, depth)
    got = {}
    if overlapped:
        stream = torch.cuda.Stream()
        s.set_stream(stream.cuda_stream)
        bufs = [torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            done = 0
            for k, upto in enumerate((4, 10)):   # a whole group of four launches, then a group and two launches still pending
                while done < upto:
                    s.accumulate(4)
                    done += 1
                s.fetch_hdr_device_async(bufs[k].data_ptr())
                got[f"after_{upto}"] = bufs[k] * 1.0   # the caller's kernel, queued behind the library's work on this stream
            for _ in range(5):                      # ... and the passes that write that frame's buffer again come behind the copy
                s.accumulate(4)
        stream.synchronize()
        got = {k: v.cpu().numpy() for k, v in got.items()}
        got["final"] = s.fetch_hdr()
    else:
        for done in range(1, 16):
            s.accumulate(4)
            if done in (4, 10):
                got[f"after_{done}"] = s.fetch_hdr()
        got["final"] = s.fetch_hdr()
    s.close()
    np.savez(out_path, **got)
    print("caller stream: ok")


def _step(call, seconds, **env):
    """`timeout -k 10 <seconds> python -c <call>` with the switches in front: one GPU step."""
    code = f"import os, sys; sys.path[:0] = [{ROOT!r}, os.path.join({ROOT!r}, 'tests')]; import test_gpu_queue_lean_pipeline as t; t.{call}"
    sets = " ".join(f"{k}={shlex.quote(v)}" for k, v in env.items())
    return f"env {sets} timeout -k 10 {seconds} {shlex.quote(sys.executable)} -c {shlex.quote(code)}"


def _run(steps):
    knobs = ("VRT_OVERLAP", "VRT_STREAMS", "VRT_PASS_STREAM", "VRT_GRID_DIV", "VRT_DEFER", "VRT_TEST_FAIL_LAUNCH")
    env = {k: v for k, v in os.environ.items() if k not in knobs}
    r = subprocess.run(["bash", "-c", " && ".join(steps)], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]


def _same(a, b, what):
    for k in a.files:
        if k != "flags":
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


@pytest.mark.parametrize("frame", sorted(FRAMES))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_shape_renders_what_isolated_launches_render(shape, frame, tmp_path):
    streams, pass_stream = SHAPES[shape]
    ref, got = str(tmp_path / "ref.npz"), str(tmp_path / "got.npz")
    _run([_step(f"_child_scenario({frame!r}, {ref!r}, False)", 300, VRT_OVERLAP="0"),
          _step(f"_child_scenario({frame!r}, {got!r}, True)", 300, VRT_STREAMS=streams, VRT_PASS_STREAM=pass_stream)])
    a, b = np.load(ref), np.load(got)
    assert int(a["flags"]) & 1 == 0 and int(b["flags"]) & 1 == 1
    assert (int(b["flags"]) >> 5) & 7 == 2, "launches of half the workgroup slots"
    assert (int(b["flags"]) >> 2) & 7 == (1 if streams == "2" else 2)
    # (the reference run is a picture, and one that moved on after the fetch in the middle: S1 is dark, its mean is below 0.01)
    assert np.isfinite(a["hdr"]).all() and a["hdr"].mean() > 0.0 and not np.array_equal(a["mid"], a["hdr"])
    _same(a, b, shape)


@pytest.mark.parametrize("queues", ["4", "16"])
def test_shape_selected_from_the_queue_count(queues, tmp_path):
    """The development build without a forced shape, in a runtime started with four and with sixteen hardware queues."""
    ref, got = str(tmp_path / "ref.npz"), str(tmp_path / "got.npz")
    _run([_step(f"_child_scenario('1080p', {ref!r}, False)", 300, VRT_OVERLAP="0", GPU_MAX_HW_QUEUES=queues),
          _step(f"_child_scenario('1080p', {got!r}, True)", 300, GPU_MAX_HW_QUEUES=queues)])
    a, b = np.load(ref), np.load(got)
    assert int(b["flags"]) & 1 == 1 and (int(b["flags"]) >> 5) & 7 == 2
    assert (int(b["flags"]) >> 2) & 7 == (1 if queues == "4" else 2), "two render streams on four queues, four on sixteen"
    _same(a, b, queues)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_callers_work_behind_accumulate_reads_the_finished_frame(shape, tmp_path):
    streams, pass_stream = SHAPES[shape]
    ref, got = str(tmp_path / "ref.npz"), str(tmp_path / "got.npz")
    _run([_step(f"_child_caller_stream({ref!r}, False)", 300, VRT_OVERLAP="0"),
          _step(f"_child_caller_stream({got!r}, True)", 300, VRT_STREAMS=streams, VRT_PASS_STREAM=pass_stream)])
    a, b = np.load(ref), np.load(got)
    assert sorted(a.files) == ["after_10", "after_4", "final"]
    _same(a, b, shape)
