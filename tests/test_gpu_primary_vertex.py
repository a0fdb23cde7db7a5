"""Shading the primary vertices ahead of the pooled launch (k_primary_vertex, queued on a launch's lane behind its pre-pass: csrc/vrt_primary.h,
csrc/vrt_plan.h plan_primary, csrc/vrt_pipeline.hip) changes no bit of what a context renders: the HDR frame, both histories and g-buffer
depth / normal / material / position of every case are those of the same calls rendered with VRT_PRIMARY=0 -- at four hardware queues (the
queue-lean shape with the context's stream as a lane) and at sixteen (VRT_DEEPER_ITEMS=0: the four-deep pipeline, as in test_gpu_prepass.py),
and at four queues with the queue's continuation records bounded to 64 (VRT_PRIMARY_CAP: eight a head), where nearly every path that goes on
takes the overflow route and is begun by the pool from depth 0.

Every run carries VRT_FULL_BELOW=0 (no overlapped launch takes every slot), so which launches are served is fixed: all nine fused launches of a
case, none of the one-sample call.  The development build reports per context the launches served, the paths k_primary_vertex finished and
the paths it sent on; the test asserts the first, that both of the others are non-zero on s1 at depth 6, and that nothing is sent on at
max_depth 1 (every path ends at its primary vertex).

Every GPU run is a process of its own under `timeout`, on the development build; a run renders every case, one context after the other."""
import os
import re
import shlex
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CALLS = (4, 4, 1, 4, 2, 3, 4, 4, 4, 4)   # nine fused launches of four, two and three samples and a one-sample call
FUSED = sum(1 for n in CALLS if n > 1)
# name: (scene, width, height, depth, rows or None, a new jitter index before every call, row stripes (rows, parts, part) or None)
CASES = {
    "s1_320x200": ("s1", 320, 200, 6, None, False, None),
    "s1_324x203_partial_tiles": ("s1", 324, 203, 6, None, False, None),
    "s1_rows_37_131": ("s1", 320, 200, 6, (37, 131), False, None),
    "s1_320x200_new_jitter_every_call": ("s1", 320, 200, 6, None, True, None),
    "sunlit_80x48": ("sunlit", 80, 48, 6, None, False, None),           # the emitting sun: the depth-0 light sample and its inline shadow ray
    "s1_256_96x56": ("s1_256", 96, 56, 4, None, False, None),
    "s1_320x200_stripes_16_part_1_of_2": ("s1", 320, 200, 6, None, False, (16, 2, 1)),
    "s1_96x56_max_depth_1": ("s1", 96, 56, 1, None, False, None),      # every path ends in the new kernel
    "s1_96x56_max_depth_2": ("s1", 96, 56, 2, None, False, None),      # ... or one bounce later
}
# name: (hardware queues, VRT_PRIMARY_CAP or None)
RUNS = {"on_q4": (4, None), "on_q16": (16, None), "cap64_q4": (4, "64")}
KNOBS = ("VRT_OVERLAP", "VRT_STREAMS", "VRT_PASS_STREAM", "VRT_GRID_DIV", "VRT_DEFER", "VRT_CTX_LANE", "VRT_TEST_FAIL_LAUNCH", "VRT_DEEP_ITEMS",
         "VRT_DEEPER_ITEMS", "VRT_DRAIN_GATE", "VRT_PREPASS", "VRT_PREPASS_REPORT", "VRT_FULL_BELOW", "VRT_PRIMARY", "VRT_PRIMARY_CAP", "VRT_PRIMARY_REPORT")
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
        s.close()   # (the development build reports the context's served launches and path counts here, on stderr)
        np.savez(os.path.join(out_dir, name + ".npz"), **out)
    print("primary vertex child: ok")


def _run(out_dir, primary, queues, cap=None):
    code = f"import os, sys; sys.path[:0] = [{ROOT!r}, os.path.join({ROOT!r}, 'tests')]; import test_gpu_primary_vertex as t; t._child({str(out_dir)!r})"
    sets = {"VRT_PRIMARY": primary, "VRT_PRIMARY_REPORT": "1", "VRT_FULL_BELOW": "0", "GPU_MAX_HW_QUEUES": str(queues)}
    if queues >= 16:
        sets["VRT_DEEPER_ITEMS"] = "0"
    if cap:
        sets["VRT_PRIMARY_CAP"] = cap
    cmd = "env " + " ".join(f"{k}={shlex.quote(v)}" for k, v in sets.items()) + f" timeout -k 10 300 {shlex.quote(sys.executable)} -c {shlex.quote(code)}"
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run(["bash", "-c", cmd + " 2>&1"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0 and "primary vertex child: ok" in r.stdout, r.stdout[-4000:]
    reports = {}
    for name, tail in re.findall(r"case (\S+):\n((?:(?!case ).*\n)*)", r.stdout):
        m = re.search(r"primary vertices served (\d+) of (\d+) render launches, paths finished (\d+) sent on (\d+)", tail)
        assert m, (name, tail)
        reports[name] = tuple(int(x) for x in m.groups())
    return reports


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    d = tmp_path_factory.mktemp("primary_off")
    reports = _run(d, "0", 4)
    assert set(reports) == set(CASES) and all(r == (0, len(CALLS), 0, 0) for r in reports.values()), reports
    ref = {name: np.load(str(d / (name + ".npz"))) for name in CASES}
    for name, a in ref.items():   # pictures, not black frames
        assert np.isfinite(a["hdr"]).all() and a["hdr"].mean() > 0.0, name
    return ref


@pytest.fixture(scope="module", params=sorted(RUNS))
def run(request, tmp_path_factory):
    queues, cap = RUNS[request.param]
    d = tmp_path_factory.mktemp("primary_" + request.param)
    reports = _run(d, "1", queues, cap)
    return request.param, reports, {name: np.load(str(d / (name + ".npz"))) for name in CASES}


@pytest.mark.parametrize("case", sorted(CASES))
def test_renders_what_it_renders_without_the_primary_vertex_kernel(case, run, reference):
    which, reports, got = run
    a, b = reference[case], got[case]
    served, launches, finished, sent_on = reports[case]
    print(f"{which} {case}: served {served} of {launches} launches; paths finished {finished}, sent on {sent_on}; flags {int(b['flags']):#x}")
    assert launches == len(CALLS)
    assert served == FUSED, "every fused launch is served, the one-sample call is not"
    scene, W, H, depth = CASES[case][:4]
    if scene == "s1" and depth == 6:
        assert finished > 0 and sent_on > 0
    if depth == 1:
        assert finished > 0 and sent_on == 0
    f = int(b["flags"])
    overlapped, pdepth, share, ctx_lane = f & 1, (f >> 2) & 7, (f >> 5) & 7, (f >> 24) & 1
    assert overlapped == 1 and share == 2, hex(f)
    if RUNS[which][0] == 4:
        assert pdepth == 1 and ctx_lane == (0 if CASES[case][6] else 1), hex(f)
    else:
        assert pdepth == 2, hex(f)
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        if k != "flags":
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (which, case, k)
