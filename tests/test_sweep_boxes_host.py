"""vrt_sweep_boxes on the host: the functions of voxel_rt2_amd/csrc/vrt_sweep.h compiled with g++ (tests/emul/sweep_emul.cpp runs the
loop of k_sweep_boxes, the 64 lanes of a box one after the other) against the numpy brute force of tests/sweep.py over every solid voxel
-- every box family on every scene; the same bytes with one lane and with 64, with pruning on and off, with the scene's culling box and
the open one; the candidate region against the cells the brute force accepted; the validity gate on literal boxes; the launch decisions
at their boundaries; the boundary (export, binding, record sizes, NULL-context code); the census of the expected records; and a
stand-alone program over one family built with -fsanitize=address,undefined (no sanitizer runs on code loaded into Python)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import sweep as W
from voxel_rt2_amd import _abi, _lib


@pytest.fixture(scope="module")
def host_scene():
    live = {}

    def get(name, open_box=False):
        if (name, open_box) not in live:
            live[name, open_box] = W.HostScene(name, open_box)
        return live[name, open_box]
    return get


def test_families_are_what_they_claim():
    W.check_census()


@pytest.mark.parametrize("scene,fam", W.cases())
def test_host_build_equals_brute_force(host_scene, scene, fam):
    boxes, want, _ = W.family(scene, fam)
    W.check(host_scene(scene).sweep(boxes), boxes, want, f"{scene}/{fam}")


@pytest.mark.parametrize("scene,fam", W.cases())
def test_lane_count_pruning_and_culling_box_change_no_byte(host_scene, scene, fam):
    boxes, want, _ = W.family(scene, fam)
    ref = host_scene(scene).sweep(boxes, 64, True)
    for lanes, prune, open_box in ((1, True, False), (64, False, False), (1, False, False), (64, True, True), (7, False, True)):
        got = host_scene(scene, open_box).sweep(boxes, lanes, prune)
        assert got.tobytes() == ref.tobytes(), f"{scene}/{fam} lanes={lanes} prune={prune} open_box={open_box}: {W.mismatches(got, ref).size} records differ"


@pytest.mark.parametrize("scene,fam", W.cases())
def test_candidate_region_holds_every_accepted_cell(host_scene, scene, fam):
    """Directly: the bounds of every cell the brute force accepted (start overlaps and contacts before t_max, not the winner alone) lie
    inside sweep_region's cells, with the scene's culling box and with the open one."""
    boxes, want, info = W.family(scene, fam)
    some = info["acc_hi"][:, 0] >= 0
    for open_box in (False, True):
        reg = host_scene(scene, open_box).regions(boxes)
        assert not reg[some, 6].any(), f"{scene}/{fam}: an empty region for a box that meets a cell"
        assert (reg[some, 0:3] <= info["acc_lo"][some]).all() and (reg[some, 3:6] >= info["acc_hi"][some]).all(), f"{scene}/{fam} open_box={open_box}"
        G = W.scene(scene)[0].shape[0]
        full = reg[reg[:, 6] == 0]
        assert (full[:, 0:3] >= 0).all() and (full[:, 3:6] <= G - 1).all() and (full[:, 0:3] <= full[:, 3:6]).all()
    if scene == "empty":
        assert host_scene(scene).regions(boxes)[:, 6].all()                  # nothing is read in a grid without solids


def box(lo=(0.0, 0.5, 0.0), hi=(0.1, 0.6, 0.1), move=(0.0, -1.0, 0.0), t_max=1.0, flags=0, reserved=0):
    b = np.zeros(1, W.BOX)
    with np.errstate(invalid="ignore"):
        b["lo"], b["hi"], b["move"], b["t_max"], b["flags"], b["reserved"] = lo, hi, move, t_max, flags, reserved
    return b


def test_validity_gate_on_literal_boxes():
    ok = lambda b: bool(W.lib().sweep_emul_valid(b.ctypes.data_as(C.c_void_p)))
    nan, inf = np.nan, np.inf
    assert ok(box()) and ok(box(t_max=inf)) and ok(box(t_max=1e-40)) and ok(box(flags=1)) and ok(box(flags=0xFFFFFFFF))
    assert ok(box(move=(0.0, -0.0, 0.0))) and ok(box(move=(1e-40, -1e30, 3e38))) and ok(box(lo=(0.0, 0.5, 0.0), hi=(0.0, 0.5, 0.0)))
    assert ok(box(lo=(-64.0, -64.0, -64.0), hi=(64.0, 64.0, 64.0)))
    for bad in (nan, inf, -inf):
        for axis in range(3):
            v = [0.25, 0.5, -0.75]
            v[axis] = bad
            assert not ok(box(lo=v, hi=(1.0, 1.0, 1.0))) and not ok(box(lo=(-1.0, -1.0, -1.0), hi=v)) and not ok(box(move=v)), (bad, axis)
    assert not ok(box(lo=(0.2, 0.5, 0.0))) and not ok(box(hi=(0.1, 0.6, -0.1)))                                  # lo > hi
    up, down = float(np.nextafter(np.float32(64), np.float32(inf))), float(np.nextafter(np.float32(-64), np.float32(-inf)))
    assert not ok(box(hi=(0.1, up, 0.1))) and not ok(box(lo=(down, 0.5, 0.0))) and not ok(box(lo=(70.0, 70.0, 70.0), hi=(71.0, 71.0, 71.0)))
    for t in (nan, 0.0, -0.0, -1e-40, -1.0, -inf):
        assert not ok(box(t_max=t)), t
    assert not ok(box(reserved=1)) and not ok(box(reserved=0x80000000))
    assert (W.valid(np.concatenate([box(), box(t_max=nan), box(reserved=1), box(hi=(0.1, up, 0.1))])) == [True, False, False, False]).all()
    # what an invalid box gets, and a valid one that meets nothing before t_max: the miss record of include/vrt_api.h
    h = W.HostScene("empty")
    for b in (box(t_max=nan), box(reserved=1), box(move=(0.0, 1.0, 0.0)), box(t_max=1e-3)):
        assert h.sweep(b)[0].tobytes() == W.miss_record(1)[0].tobytes(), b


def test_known_contacts_on_tie():
    """Literal boxes on the tie scene: the voxel (37, 48, 37) stands on the floor plane p(48) with nothing above it and nothing at
    (38, 48, 37); its top face is p(49)."""
    h = W.HostScene("tie")
    p = lambda k: k / 64 - 1
    mat = W.scene("tie")[0]
    assert mat[37, 48, 37] > 0 and mat[37, 49, 37] <= 0 and mat[38, 48, 37] <= 0 and not (mat[:36] > 0).any()
    down = h.sweep(box(lo=(p(37.25), p(52), p(37.25)), hi=(p(37.75), p(53), p(37.75)), move=(0.0, -1 / 64, 0.0), t_max=np.inf))[0]
    assert down["kind"] == _abi.SWEEP_VOXEL and down["t"] == 3.0 and down["cell"].tolist() == [37, 48, 37] and down["normal"].tolist() == [0.0, 1.0, 0.0]
    # resting on the top face: stopped at once going down, free going sideways (touching is not overlapping), START once it sinks in
    rest = dict(lo=(p(37.25), p(49), p(37.25)), hi=(p(37.75), p(50), p(37.75)))
    at0 = h.sweep(box(move=(0.0, -1.0, 0.0), **rest))[0]
    assert at0["kind"] == _abi.SWEEP_VOXEL and at0["t"] == 0.0 and not np.signbit(at0["t"]) and at0["normal"].tolist() == [0.0, 1.0, 0.0]
    assert h.sweep(box(move=(1 / 64, 0.0, 0.0), flags=1, **rest))[0]["kind"] == _abi.SWEEP_MISS
    assert h.sweep(box(move=(0.0, 0.0, 0.0), **rest))[0]["kind"] == _abi.SWEEP_MISS
    sunk = h.sweep(box(lo=(p(37.25), p(48.5), p(37.25)), hi=(p(37.75), p(50), p(37.75)), move=(0.0, 0.0, 0.0)))[0]
    assert sunk["kind"] == _abi.SWEEP_START and sunk["t"] == 0.0 and sunk["cell"].tolist() == [37, 48, 37] and sunk["normal"].tolist() == [0.0, 0.0, 0.0]
    # the floor: beside the voxels, falling two cells onto p(48); without the floor a miss; below it a start overlap with cell -1
    fall = dict(lo=(p(10), p(50), p(10)), hi=(p(12), p(52), p(12)), move=(0.0, -1 / 64, 0.0), t_max=np.inf)
    f = h.sweep(box(**fall))[0]
    assert f["kind"] == _abi.SWEEP_FLOOR and f["t"] == 2.0 and f["cell"].tolist() == [-1, -1, -1] and f["normal"].tolist() == [0.0, 1.0, 0.0]
    assert h.sweep(box(flags=1, **fall))[0].tobytes() == W.miss_record(1)[0].tobytes()
    under = h.sweep(box(lo=(p(10), p(47.5), p(10)), hi=(p(12), p(52), p(12))))[0]
    assert under["kind"] == _abi.SWEEP_START and under["cell"].tolist() == [-1, -1, -1] and under["t"] == 0.0
    # the floor is a plane, not the render's disc: far outside radius 10 it still stops the box
    far = h.sweep(box(lo=(40.0, p(50), 40.0), hi=(41.0, p(52), 41.0), move=(0.0, -1 / 64, 0.0), t_max=np.inf))[0]
    assert far["kind"] == _abi.SWEEP_FLOOR and far["t"] == 2.0


def test_plan_sweep_at_its_boundaries():
    lib = W.lib()
    assert lib.sweep_emul_chunk() >= 256 and lib.sweep_emul_chunk() * 80 <= 1 << 26
    blocks = lib.sweep_emul_blocks
    assert blocks(1, 256, 4) == 1 and blocks(4, 256, 4) == 1 and blocks(5, 256, 4) == 2 and blocks(8, 256, 4) == 2 and blocks(9, 256, 4) == 3
    assert blocks(4 * 1024, 256, 4) == 1024 and blocks(4 * 1024 + 1, 256, 4) == 1024 and blocks(4 * 1023 + 1, 256, 4) == 1024 and blocks(4 * 1023, 256, 4) == 1023
    assert blocks(1 << 40, 256, 7) == 1792 and blocks(1 << 24, 256, 0) == 256 and blocks(1 << 24, 256, -3) == 256


def test_export_binding_and_record_sizes():
    assert "vrt_sweep_boxes" in set(_lib.exported_symbols())
    assert _abi.BOX_SWEEP.itemsize == 48 and _abi.SWEEP_HIT.itemsize == 32
    assert W.lib().sweep_emul_sizes(0) == 48 and W.lib().sweep_emul_sizes(1) == 32
    assert [_abi.BOX_SWEEP.fields[k][1] for k in ("lo", "flags", "hi", "reserved", "move", "t_max")] == [0, 12, 16, 28, 32, 44]
    assert [_abi.SWEEP_HIT.fields[k][1] for k in ("t", "kind", "cell", "normal")] == [0, 4, 8, 20]
    assert (_abi.SWEEP_MISS, _abi.SWEEP_FLOOR, _abi.SWEEP_VOXEL, _abi.SWEEP_START, _abi.SWEEP_NO_FLOOR, _abi.SWEEP_MAX_COORD) == (0, 1, 2, 3, 1, 64.0)
    lib = _lib.load()
    sweep = lib.vrt_sweep_boxes
    assert sweep.restype is C.c_int and len(sweep.argtypes) == 5 and sweep.argtypes[1] is C.c_int64
    b, h = np.zeros(1, _abi.BOX_SWEEP), np.zeros(1, _abi.SWEEP_HIT)
    assert sweep(None, 1, b.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p), 0) == _abi.VRT_E_INVALID
    assert b"null" in lib.vrt_last_error()
    from voxel_rt2_amd.renderer import Renderer
    assert all(callable(getattr(Renderer, name)) for name in ("sweep_boxes", "overlap_boxes", "box_of_voxels"))


def test_standalone_program_under_sanitizers(tmp_path):
    """The host row function over one family of boxes, as a program of its own (-DSWEEP_EMUL_MAIN: its own main, a scene built in C++),
    with AddressSanitizer and UndefinedBehaviorSanitizer: it must run clean and the four ways of running a box must agree."""
    exe = str(tmp_path / "sweep_emul_main")
    src, _ = W.sources()
    flags = [f for f in W.GXX if f not in ("-fPIC", "-O2")] + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                                 "-static-libasan", "-static-libubsan", "-DSWEEP_EMUL_MAIN"]
    subprocess.run(flags + ["-o", exe, src], check=True, capture_output=True)   # (the runtimes linked in: the program needs nothing preloaded)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), (run.returncode, run.stdout[-500:], run.stderr[-2000:])
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-2000:]
