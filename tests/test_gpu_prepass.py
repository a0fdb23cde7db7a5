"""The camera-ray pre-pass (k_primary_records, queued on a launch's lane ahead of it: csrc/vrt_plan.h plan_prepass, csrc/vrt_pipeline.hip)
changes no bit of what a context renders: the HDR frame, both histories and g-buffer depth / normal / material / position of every
case are those of the same calls rendered with VRT_PREPASS=0 -- with the pre-pass on (1) and with it queued but the launch not told
(2), at four hardware queues (the queue-lean shape with the context's stream as a lane) and at sixteen.  At sixteen queues frames
this small would take the eight-deep pipeline, which has no pre-pass, so those runs carry VRT_DEEPER_ITEMS=0: the four-deep pipeline,
the shape the headline runs in there.

Whether a launch finds the pipeline nearly empty, takes every slot and so has no pre-pass depends on the host's timing; every run
here carries VRT_FULL_BELOW=0 (no overlapped launch takes every slot), so which launches have a pre-pass is fixed: all nine fused
launches of a case, none of the one-sample call -- three per lane on the three lanes of four queues, two or three on the four streams
of sixteen, across two grouped passes -- and the test asserts that count and the shape the run reports for every case of every run.

Every GPU run is a process of its own under `timeout`, on the development build (the switches are read when a context is created,
the queue count when the runtime starts); a run renders every case, one context after the other."""
import os
import re
import shlex
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CALLS = (4, 4, 1, 4, 4, 4, 4, 4, 4, 4)   # nine fused launches and a one-sample call: every lane serves two pre-passes at least, two grouped passes are crossed
FUSED = sum(1 for n in CALLS if n > 1)
# name: (scene, width, height, depth, rows or None, a new jitter index before every call, row stripes (rows, parts, part) or None)
CASES = {
    "s1_320x200": ("s1", 320, 200, 6, None, False, None),
    "s1_320x200_new_jitter_every_call": ("s1", 320, 200, 6, None, True, None),
    "s1_324x203_partial_tiles": ("s1", 324, 203, 6, None, False, None),
    "s1_rows_37_131": ("s1", 320, 200, 6, (37, 131), False, None),      # a row tile whose first row is no multiple of 8
    "sunlit_80x48": ("sunlit", 80, 48, 6, None, False, None),           # the emitting-sun instantiation
    "s1_256_96x56": ("s1_256", 96, 56, 4, None, False, None),
    # one rank's interleaved stripes of a two-way split (vrt_set_row_stripes): the launch's rows through launch_tile_row / launch_renders_row;
    # such a context does not defer its accumulation, so on four queues it runs two lanes, not three
    "s1_320x200_stripes_16_part_1_of_2": ("s1", 320, 200, 6, None, False, (16, 2, 1)),
}
RUNS = {"on_q4": ("1", 4), "untold_q4": ("2", 4), "on_q16": ("1", 16), "untold_q16": ("2", 16)}
KNOBS = ("VRT_OVERLAP", "VRT_STREAMS", "VRT_PASS_STREAM", "VRT_GRID_DIV", "VRT_DEFER", "VRT_CTX_LANE", "VRT_TEST_FAIL_LAUNCH", "VRT_DEEP_ITEMS",
         "VRT_DEEPER_ITEMS", "VRT_DRAIN_GATE", "VRT_PREPASS", "VRT_PREPASS_REPORT", "VRT_FULL_BELOW")
BUFFERS = ("hist_d", "hist_s", "depth", "normal", "mat", "pos")


def _child(out_dir):
    """Every case in this process (the environment carries the switches); the state of each goes to out_dir/<case>.npz."""
    import orc
    from voxel_rt2_amd import _abi, _lib, host, scenes
    from voxel_rt2_amd._session import NativeSession
    lib = _lib.load_dev()
    which = dict(zip(BUFFERS, (_abi.BUF_HISTORY_DIFFUSE, _abi.BUF_HISTORY_SPECULAR, _abi.BUF_GBUF_DEPTH, _abi.BUF_GBUF_NORMAL, _abi.BUF_GBUF_MAT,
                               _abi.BUF_GBUF_POSITION)))
    for name, (scene, W, H, depth, rows, rejitter, stripes) in CASES.items():
        mat, rgb, params = scenes.SCENES[scene](0)
        cfg = host.make_config(W, H, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=depth, seed=3, grid_res=mat.shape[0])
        if rows:
            cfg.row_begin, cfg.row_end = rows
        s = NativeSession(lib, "vrt_", cfg)
        orc.setup(s, mat, rgb, params)
        if stripes:
            s.set_row_stripes(*stripes)
        for k, n in enumerate(CALLS):
            if rejitter:
                s.set_camera(host.default_camera(W, H, jitter_index=k + 1))
            s.accumulate(n)
        out = {"hdr": s.fetch_hdr(), "flags": np.uint32(s.stats()["pipeline_flags"])}
        for key, b in which.items():
            out[key] = s.fetch_buffer(b)
        print(f"case {name}:", flush=True)
        sys.stderr.flush()
        s.close()   # (the development build reports the context's pre-passes here, on stderr)
        np.savez(os.path.join(out_dir, name + ".npz"), **out)
    print("prepass child: ok")


def _run(out_dir, prepass, queues):
    code = f"import os, sys; sys.path[:0] = [{ROOT!r}, os.path.join({ROOT!r}, 'tests')]; import test_gpu_prepass as t; t._child({str(out_dir)!r})"
    sets = {"VRT_PREPASS": prepass, "VRT_PREPASS_REPORT": "1", "VRT_FULL_BELOW": "0", "GPU_MAX_HW_QUEUES": str(queues)}
    if queues >= 16:
        sets["VRT_DEEPER_ITEMS"] = "0"
    cmd = "env " + " ".join(f"{k}={shlex.quote(v)}" for k, v in sets.items()) + f" timeout -k 10 300 {shlex.quote(sys.executable)} -c {shlex.quote(code)}"
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run(["bash", "-c", cmd + " 2>&1"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0 and "prepass child: ok" in r.stdout, r.stdout[-4000:]
    # "case NAME:" is printed before the context is closed, the report when it is
    reports = {}
    for name, tail in re.findall(r"case (\S+):\n((?:(?!case ).*\n)*)", r.stdout):
        m = re.search(r"pre-passes queued (\d+) told (\d+) of (\d+) render launches", tail)
        assert m, (name, tail)
        reports[name] = tuple(int(x) for x in m.groups())
    return reports


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    d = tmp_path_factory.mktemp("prepass_off")
    reports = _run(d, "0", 4)
    assert set(reports) == set(CASES) and all(r[:2] == (0, 0) and r[2] == len(CALLS) for r in reports.values()), reports
    ref = {name: np.load(str(d / (name + ".npz"))) for name in CASES}
    for name, a in ref.items():   # pictures, not black frames
        assert np.isfinite(a["hdr"]).all() and a["hdr"].mean() > 0.0, name
    return ref


@pytest.fixture(scope="module", params=sorted(RUNS))
def run(request, tmp_path_factory):
    prepass, queues = RUNS[request.param]
    d = tmp_path_factory.mktemp("prepass_" + request.param)
    reports = _run(d, prepass, queues)
    return request.param, reports, {name: np.load(str(d / (name + ".npz"))) for name in CASES}


@pytest.mark.parametrize("case", sorted(CASES))
def test_renders_what_it_renders_without_the_pre_pass(case, run, reference):
    which, reports, got = run
    a, b = reference[case], got[case]
    queued, told, launches = reports[case]
    print(f"{which} {case}: pre-passes queued {queued}, told {told}, of {launches} launches; flags {int(b['flags']):#x}")
    assert launches == len(CALLS)
    assert queued == FUSED, "every fused launch has a pre-pass, the one-sample call has none"
    assert told == (queued if RUNS[which][0] == "1" else 0)
    # the shape the run took: overlapped, launches of half the slots; four queues: two streams of the pipeline's own and, where the
    # context defers its accumulation, the context's stream as the third lane; sixteen: four streams
    f = int(b["flags"])
    overlapped, depth, share, ctx_lane = f & 1, (f >> 2) & 7, (f >> 5) & 7, (f >> 24) & 1
    assert overlapped == 1 and share == 2, hex(f)
    if RUNS[which][1] == 4:
        assert depth == 1 and ctx_lane == (0 if CASES[case][6] else 1), hex(f)
    else:
        assert depth == 2, hex(f)
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        if k != "flags":
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (which, case, k)


def test_pre_passes_are_queued(run):
    """Not a comparison of two runs without one: every case of the run reports its nine pre-passes."""
    which, reports, _ = run
    print(which, reports)
    assert set(reports) == set(CASES) and all(r[0] == FUSED for r in reports.values())
