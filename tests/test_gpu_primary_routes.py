"""The routes of the primary-vertex queue (k_primary_vertex and the QUEUED / SERVED instantiations of the pooled kernel: csrc/vrt_kernels.hip,
csrc/vrt_primary.h, csrc/vrt_pipeline.hip) that tests/test_gpu_primary_vertex.py cannot reach, each held to the bits of the same calls rendered
with VRT_PRIMARY=0 VRT_PREPASS=0 -- HDR frame, both histories, g-buffer depth / normal / material / position, byte for byte, no pixel masked:

  1. records that fail their check.  The development build's hook VRT_TEST_SPOIL_RECORDS=N (k_spoil_primary_records) inverts bit 0 of the
     check word of every live pixel's record whose table index is the launch's number mod N (mod N), behind the pre-pass and ahead of every
     reader.  `spoil11` / `spoil11_q16` / `spoil11_cap64`: k_primary_vertex makes every sample of such a pixel a leftover and the QUEUED BEGIN
     takes its `!known` arm (pool_begin, the record store of sample 0, the pool writes the g-buffer); `spoil1`: every path of every launch;
     `prepass_spoil11` (VRT_PRIMARY=0 VRT_PREPASS=1): the `!known` arm for sample 0 of the SERVED instantiation.
  2. a queue that has to grow (lane_primary_queue): CALLS puts a two-sample launch before a three-sample one before a four-sample one on every
     lane, `sun_on` changes the records from 16 to 24 words and the kernel to k_primary_vertex_sun between launches.  The development build
     reports how often each lane's queue was reallocated.
  3. fewer tiles than work heads, and uneven heads: frames of 1, 3, 6 and 9 tiles.
  4. a context that changes between SERVED launches (every run carries VRT_FULL_BELOW=0, so which launches are served does not depend on the
     host's timing): voxel edits on the host and the device path, the sun switched on and off, instrumented launches in between, reserved CUs,
     a reset with launches in flight, a new jitter before every call.

Two things are not as the issue that asked for this test put them, because the library does not allow them:
  - `restripe` (vrt_set_row_stripes between launches): the call is refused with VRT_E_STATE once a context has accumulated
    (vrt_api.hip: "set the stripes before the first vrt_accumulate"), so a context's tile count cannot change.  The case asserts the refusal,
    resets and goes on full-frame.
  - a 72x24 context of rows (8, 16) renders its two halo rows either side: rows 6..17, two tile rows, 18 tiles (heads 0 and 1 hold three, the
    others two).  The case stays; `s1_72x8_9_tiles` is the frame with nine tiles in one tile row, head 0 holding two.
`reset_between` takes no snapshot before the reset: a fetch would wait for the launches that are meant to be in flight.

The chain ends in an independent reference: the reference run's HDR frame is compared bit for bit with the CPU oracle's after the same
calls (scene changes, resets and jitters included; the oracle knows no stripes: the owned rows are compared).  The two `edit` cases are
compared with the reference run only -- the oracle has no vrt_update_voxels, and without a reset the frame mixes two scenes.

The counts.  A run's child prints per context the launches served, the paths k_primary_vertex finished and sent on, the pre-passes the
launches were told of and the reallocations per lane; the test asserts the served count the plan gives (every fused launch that is not
instrumented; no one-sample call), `finished == sent_on == 0` under spoil1, and under spoil11 -- with VRT_PRIMARY_CAP above the item
count, so that no path overflows into a leftover -- `finished + sent_on == sum over served launches of samples x (live - spoiled pixels)`,
worked out here from the hook's rule and the launch numbers (a context's k-th vrt_accumulate call of at most four samples is launch k).

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

CALLS = (2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 1, 4)   # on two, three or four lanes: 2 before 3 before 4 samples on every lane; the one-sample call is not served
SPOIL = 11
# name: (scene, width, height, depth, rows or None, row stripes (rows, parts, part) or None)
STATIC = {
    "s1_96x56": ("s1", 96, 56, 4, None, None),
    "sunlit_80x48": ("sunlit", 80, 48, 6, None, None),                # 24-word records, k_primary_vertex_sun
    "s1_256_96x56": ("s1_256", 96, 56, 4, None, None),
    "s1_24x8_3_tiles": ("s1", 24, 8, 4, None, None),                  # heads 3..7 empty
    "s1_8x8_1_tile": ("s1", 8, 8, 4, None, None),
    "s1_72x24_rows_8_16": ("s1", 72, 24, 4, (8, 16), None),           # 18 tiles in two tile rows (see above)
    "s1_72x8_9_tiles": ("s1", 72, 8, 4, None, None),                  # one tile row: head 0 holds two
    "sunlit_20x12_6_tiles": ("sunlit", 20, 12, 4, None, None),        # partial in both directions, emitting sun
    "s1_320x200_stripes_16_part_1_of_2": ("s1", 320, 200, 4, None, (16, 2, 1)),
}
# The state cases, 96x56 at depth 4: (scene, operations).  ("acc", n): vrt_accumulate(n); ("snap",): all seven buffers; ("edit", device path);
# ("sun", on): vrt_set_scene with an emitting / a black light_color; ("stripes", rows, parts, part): expected to be refused
A4 = (("acc", 4),) * 4
STATE = {
    "edit_host": ("s1", A4 + (("snap",), ("edit", False)) + A4 + (("snap",),)),
    "edit_device": ("s1", A4 + (("snap",), ("edit", True)) + A4 + (("snap",),)),
    "sun_on": ("s1", A4 + (("snap",), ("sun", True), ("reset",)) + A4 + (("snap",),)),
    "sun_off": ("sunlit", A4 + (("snap",), ("sun", False), ("reset",)) + A4 + (("snap",),)),
    "restripe": ("s1", A4 + (("snap",), ("stripes", 16, 2, 1), ("reset",)) + A4 + (("snap",), ("stripes", 8, 2, 0), ("reset",), ("acc", 4), ("acc", 4), ("snap",))),
    "instr_between": ("s1", (("instr", 1),) + A4 + (("snap",), ("instr", 0)) + A4 + (("snap",),)),
    "reserve_between": ("sunlit", A4 + (("snap",), ("reserve", 32)) + A4 + (("snap",),)),
    "reset_between": ("s1", A4 + (("reset",),) + A4 + (("snap",),)),
    "rejitter": ("s1", tuple(op for k in range(8) for op in (("jitter", k + 1), ("acc", 4))) + (("snap",),)),
}
SW, SH, SDEPTH = 96, 56, 4
CASES = sorted(STATIC) + sorted(STATE)
# name: (VRT_PRIMARY, VRT_PREPASS or None, VRT_TEST_SPOIL_RECORDS or None, VRT_PRIMARY_CAP or None, hardware queues)
# (spoil11 carries a cap above the item count, so that its path counts are exact; spoil11_q16 is the same switches under the rule's own cap)
BIG_CAP = str(8 * 320 * 200 * 4)   # eight heads x every item of the largest launch: plan_primary_caps clamps it to the leftover capacity
RUNS = {
    "prepass_spoil11": ("0", "1", str(SPOIL), None, 4),
    "on": ("1", None, None, None, 4),
    "spoil11": ("1", None, str(SPOIL), BIG_CAP, 4),
    "spoil11_cap64": ("1", None, str(SPOIL), "64", 4),
    "spoil1": ("1", None, "1", None, 4),
    "spoil11_q16": ("1", None, str(SPOIL), None, 16),
}
KNOBS = ("VRT_OVERLAP", "VRT_STREAMS", "VRT_PASS_STREAM", "VRT_GRID_DIV", "VRT_DEFER", "VRT_CTX_LANE", "VRT_TEST_FAIL_LAUNCH", "VRT_DEEP_ITEMS",
         "VRT_DEEPER_ITEMS", "VRT_DRAIN_GATE", "VRT_PREPASS", "VRT_PREPASS_REPORT", "VRT_FULL_BELOW", "VRT_PRIMARY", "VRT_PRIMARY_CAP", "VRT_PRIMARY_REPORT",
         "VRT_TEST_SPOIL_RECORDS", "VRT_RENDER", "VRT_FUSE", "VRT_OVERLAP_SINGLE")
BUFFERS = ("hist_d", "hist_s", "depth", "normal", "mat", "pos")
EDIT_LO, EDIT_HI = (82, 64, 82), (94, 76, 94)   # a box on s1's slab in the middle of the default view


def edit_box():
    """The box's new voxels: the slab's cells under it become material 11, a block of material 21 stands on them, the towers around it go."""
    shape = tuple(h - l for l, h in zip(EDIT_LO, EDIT_HI))
    bmat, brgb = np.zeros(shape, np.int8), np.zeros(shape + (3,), np.uint8)
    bmat[:, 0, :] = 11
    brgb[:, 0, :] = (50, 200, 80)
    bmat[2:10, 1:9, 2:10] = 21
    brgb[2:10, 1:9, 2:10] = (230, 180, 40)
    return bmat, brgb


def ops_of(case):
    return tuple(("acc", n) for n in CALLS) + (("snap",),) if case in STATIC else STATE[case][1]


def geometry(case):
    """(scene, W, H, depth, rows, stripes) of any case."""
    return STATIC[case] if case in STATIC else (STATE[case][0], SW, SH, SDEPTH, None, None)


def light_on(params, on):
    return dict(params, light_color=(1.0, 1.0, 1.0) if on else (0.0, 0.0, 0.0))


def drive(s, case, scene_of, snap, product):
    """The case's operations on session `s` (the product's or the oracle's, which ignores what it does not know); snap(s) at every ("snap",)."""
    from voxel_rt2_amd import host
    scene, W, H = geometry(case)[:3]
    params = scene_of(scene)[2]
    keep = []
    refused = 0
    for op in ops_of(case):
        if op[0] == "acc":
            s.accumulate(op[1])
        elif op[0] == "snap":
            snap(s)
        elif op[0] == "reset":
            s.reset()
        elif op[0] == "jitter":
            s.set_camera(host.default_camera(W, H, jitter_index=op[1]))
        elif op[0] == "sun":
            s.set_scene(host.make_scene_params(**light_on(params, op[1])))
        elif not product:
            continue
        elif op[0] == "edit":
            bmat, brgb = edit_box()
            if op[1]:
                import torch
                tm, tr = torch.from_numpy(bmat).cuda(), torch.from_numpy(brgb).cuda()
                torch.cuda.synchronize()   # (written on torch's stream, read on the context's)
                keep += [tm, tr]
                s.update_voxels(EDIT_LO, EDIT_HI, tm.data_ptr(), tr.data_ptr(), on_device=True)
            else:
                s.update_voxels(EDIT_LO, EDIT_HI, bmat, brgb)
        elif op[0] == "stripes":
            from voxel_rt2_amd._session import NativeError
            try:
                s.set_row_stripes(*op[1:])
            except NativeError:
                refused += 1
        elif op[0] == "instr":
            import ctypes as C
            assert s._lib.vrt_set_instrumented(C.c_void_p(s._ctx), int(op[1])) == 0
        elif op[0] == "reserve":
            s.reserve_cus(op[1])
    return refused, keep


def _child(out_dir):
    """Every case in this process (the environment carries the switches); the snapshots of each go to out_dir/<case>.npz."""
    import functools
    import orc
    from voxel_rt2_amd import _abi, _lib, host, scenes
    from voxel_rt2_amd._session import NativeSession
    lib = _lib.load_dev()
    which = dict(zip(BUFFERS, (_abi.BUF_HISTORY_DIFFUSE, _abi.BUF_HISTORY_SPECULAR, _abi.BUF_GBUF_DEPTH, _abi.BUF_GBUF_NORMAL, _abi.BUF_GBUF_MAT,
                               _abi.BUF_GBUF_POSITION)))
    scene_of = functools.lru_cache(maxsize=None)(lambda name: scenes.SCENES[name](0))
    for name in CASES:
        scene, W, H, depth, rows, stripes = geometry(name)
        mat, rgb, params = scene_of(scene)
        cfg = host.make_config(W, H, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=depth, seed=3, grid_res=mat.shape[0])
        if rows:
            cfg.row_begin, cfg.row_end = rows
        s = NativeSession(lib, "vrt_", cfg)
        orc.setup(s, mat, rgb, params)
        if stripes:
            s.set_row_stripes(*stripes)
        out = {}

        def snap(s):
            k = sum(1 for key in out if key.endswith("_hdr"))
            out[f"snap{k}_hdr"] = s.fetch_hdr()
            for key, b in which.items():
                out[f"snap{k}_{key}"] = s.fetch_buffer(b)
        refused, keep = drive(s, name, scene_of, snap, True)
        out["flags"] = np.uint32(s.stats()["pipeline_flags"])
        out["refused"] = np.uint32(refused)
        print(f"case {name}:", flush=True)
        sys.stderr.flush()
        s.close()   # (the development build reports the context's served launches, path counts and reallocations here, on stderr)
        del keep
        np.savez(os.path.join(out_dir, name + ".npz"), **out)
    print("primary routes child: ok")


def _run(out_dir, which):
    primary, prepass, spoil, cap, queues = which
    code = f"import os, sys; sys.path[:0] = [{ROOT!r}, os.path.join({ROOT!r}, 'tests')]; import test_gpu_primary_routes as t; t._child({str(out_dir)!r})"
    sets = {"VRT_PRIMARY": primary, "VRT_PRIMARY_REPORT": "1", "VRT_PREPASS_REPORT": "1", "VRT_FULL_BELOW": "0", "GPU_MAX_HW_QUEUES": str(queues)}
    if queues >= 16:
        sets["VRT_DEEPER_ITEMS"] = "0"
    for k, v in (("VRT_PREPASS", prepass), ("VRT_TEST_SPOIL_RECORDS", spoil), ("VRT_PRIMARY_CAP", cap)):
        if v is not None:
            sets[k] = v
    cmd = "env " + " ".join(f"{k}={shlex.quote(v)}" for k, v in sets.items()) + f" timeout -k 10 300 {shlex.quote(sys.executable)} -c {shlex.quote(code)}"
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run(["bash", "-c", cmd + " 2>&1"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0 and "primary routes child: ok" in r.stdout, r.stdout[-4000:]
    reports = {}
    for name, tail in re.findall(r"case (\S+):\n((?:(?!case ).*\n)*)", r.stdout):
        m = re.search(r"primary vertices served (\d+) of (\d+) render launches, paths finished (\d+) sent on (\d+), queues regrown \[([\d,]*)\]", tail)
        p = re.search(r"pre-passes queued (\d+) told (\d+) of (\d+) render launches", tail)
        assert m and p, (name, tail)
        reports[name] = dict(served=int(m.group(1)), launches=int(m.group(2)), finished=int(m.group(3)), sent_on=int(m.group(4)),
                             regrown=[int(x) for x in m.group(5).split(",") if x], told=int(p.group(2)))
    return reports


def _load(d):
    return {name: np.load(str(d / (name + ".npz"))) for name in CASES}


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    d = tmp_path_factory.mktemp("routes_reference")
    reports = _run(d, ("0", "0", None, None, 4))
    assert set(reports) == set(CASES), reports
    for name, r in reports.items():
        assert r["served"] == 0 and r["told"] == 0 and r["launches"] == len(launches_of(name)), (name, r)
    ref = _load(d)
    for name, a in ref.items():   # pictures, not black frames
        for k in a.files:
            if k.endswith("_hdr"):
                assert np.isfinite(a[k]).all() and a[k].mean() > 0.0, (name, k)
    return ref


@pytest.fixture(scope="module", params=sorted(RUNS))
def run(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("routes_" + request.param)
    reports = _run(d, RUNS[request.param])
    return request.param, reports, _load(d)


# ---- what the plan and the hook's rule say of a case -------------------------------------------------------------------------------------
def launches_of(case):
    """[(samples, served)] per render launch, in launch-number order: a call of at most four samples is one launch; served: fused and not
    instrumented (plan_prepass, plan_primary with VRT_FULL_BELOW=0)."""
    out, instr = [], False
    for op in ops_of(case):
        if op[0] == "instr":
            instr = bool(op[1])
        elif op[0] == "acc":
            assert 1 <= op[1] <= 4
            out.append((op[1], op[1] > 1 and not instr))
    return out


def live_indices(case):
    """The record-table index (v - row0) * W + u of every pixel a launch of the case renders: k_primary_records' gating over its tiles
    (launch_tile_row, launch_renders_row of csrc/vrt_types.h; outside_render_area is never true at render scale 1)."""
    _, W, H, _, rows, stripes = geometry(case)
    row0, row1 = (max(rows[0] - 2, 0), min(rows[1] + 2, H)) if rows else (0, H)   # a tile's two halo rows either side
    if stripes:
        srows, parts, part = stripes
        period, first = srows * parts, part * srows
        per = srows // 8 + 2
        starts = [k * period + first - 8 + j * 8 for k in range(len(range(first, H, period))) for j in range(per)]
        renders = lambda v: v >= row0 and (v - first + 2 + period) % period < srows + 4
    else:
        starts = [row0 + t * 8 for t in range((row1 - row0 + 7) >> 3)]
        renders = lambda v: True
    vs = [v for t in starts for v in range(t, t + 8) if v < row1 and renders(v)]
    assert len(vs) == len(set(vs))   # (every row once: tests/test_emul_parity.py)
    v = np.array(sorted(vs))
    return ((v[:, None] - row0) * W + np.arange(W)[None, :]).ravel()


def lanes_of(case, which):
    """Render lanes of the run's pipeline: sixteen queues: four streams; four: two streams and, where the context defers its accumulation
    (no row stripes), its own stream as the third (plan_pipeline_shape)."""
    return 4 if RUNS[which][4] >= 16 else 2 if geometry(case)[5] else 3


def expected_unspoiled(case, n):
    idx = live_indices(case)
    return sum(g * int((idx % n != k % n).sum()) for k, (g, served) in enumerate(launches_of(case)) if served)


# ---- the tests ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_renders_what_it_renders_without_the_queue(case, run, reference):
    which, reports, got = run
    a, b, r = reference[case], got[case], reports[case]
    primary, prepass, spoil, cap, queues = RUNS[which]
    plan = launches_of(case)
    want_served = sum(1 for _, served in plan if served)
    print(f"{which} {case}: served {r['served']} (told {r['told']}) of {r['launches']} launches, plan {want_served}; paths finished {r['finished']}, "
          f"sent on {r['sent_on']}; queues regrown {r['regrown']}; flags {int(b['flags']):#x}")
    assert r["launches"] == len(plan)
    assert r["told"] == want_served, "every fused launch that is not instrumented has a pre-pass it is told of; a one-sample call has none"
    assert r["served"] == (want_served if primary == "1" else 0)
    scene, W, H, depth, rows, stripes = geometry(case)
    if case == "restripe":
        assert int(b["refused"]) == 2 and int(a["refused"]) == 2, "vrt_set_row_stripes is refused once a context has accumulated"
    if which == "on":
        if scene == "s1" and depth >= 4 and ((W + 7) // 8) * ((H + 7) // 8) >= 60:
            assert r["finished"] > 0 and r["sent_on"] > 0
        if case == "sun_on":   # 16-word records, then 24-word ones: every lane of the second half grows its queue once
            assert len(r["regrown"]) == 3 and all(n >= 1 for n in r["regrown"]), r["regrown"]
    if primary == "1" and case in STATIC:   # 2, then 3, then 4 samples on every lane
        assert len(r["regrown"]) == lanes_of(case, which) and all(n >= 2 for n in r["regrown"]), r["regrown"]
    if which == "spoil1":
        assert r["finished"] == 0 and r["sent_on"] == 0, "every path went the leftover route"
    if which == "spoil11":   # (no head overflows: VRT_PRIMARY_CAP)
        want = expected_unspoiled(case, SPOIL)
        print(f"    paths of unspoiled records, from the hook's rule: {want}")
        assert r["finished"] + r["sent_on"] == want
    f = int(b["flags"])
    assert f & 1 == 1 and (f >> 2) & 7 == (2 if queues >= 16 else 1), hex(f)   # overlapped; four streams or the queue-lean shape
    assert sorted(a.files) == sorted(b.files) and sum(1 for k in a.files if k.endswith("_hdr")) == sum(1 for op in ops_of(case) if op[0] == "snap")
    for k in a.files:
        if k.startswith("snap"):
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (which, case, k)


@pytest.mark.parametrize("case", ["edit_host", "edit_device"])
def test_the_edit_is_in_view(case, reference):
    """What the edit cases rest on: the box changes what some camera rays hit and the material under others."""
    a = reference[case]
    assert (a["snap0_mat"] != a["snap1_mat"]).any() and (a["snap0_depth"] != a["snap1_depth"]).any()
    assert all(np.array_equal(a[k].view(np.uint8), reference["edit_device" if case == "edit_host" else "edit_host"][k].view(np.uint8)) for k in a.files if k.startswith("snap"))


@pytest.mark.parametrize("case", [c for c in CASES if not c.startswith("edit_")])
def test_reference_run_matches_the_oracle(case, reference):
    """The last snapshot's HDR frame of the reference run against the CPU oracle after the same operations, bit for bit (owned rows)."""
    import orc
    from voxel_rt2_amd import host
    scene, W, H, depth, rows, stripes = geometry(case)
    mat, rgb, params = _scene(scene)
    cfg = host.make_config(W, H, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=depth, seed=3, grid_res=mat.shape[0])
    if rows:
        cfg.row_begin, cfg.row_end = rows
    o = orc.Oracle(cfg)
    orc.setup(o, mat, rgb, params)
    frames = []
    drive(o, case, _scene, lambda s: frames.append(s.fetch_hdr()), False)
    o.close()
    a = reference[case]
    got = a[f"snap{len(frames) - 1}_hdr"]
    own = np.zeros(H, bool)
    if stripes:
        srows, parts, part = stripes
        for s0 in range(part * srows, H, srows * parts):
            own[s0:s0 + srows] = True
        assert not got[~own].any()
    else:
        own[:] = True
    assert got[own].any()
    assert np.array_equal(got[own].view(np.uint32), frames[-1][own].view(np.uint32)), f"{(got[own] != frames[-1][own]).sum()} values differ"


_SCENES = {}


def _scene(name):
    from voxel_rt2_amd import scenes
    if name not in _SCENES:
        _SCENES[name] = scenes.SCENES[name](0)
    return _SCENES[name]
