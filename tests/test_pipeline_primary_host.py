"""The primary-vertex stage in the launch plan (csrc/vrt_plan.h), without a GPU: plan_primary names exactly the launches that have a
pre-pass and are told of it; plan_primary_caps sizes a queue in which a leftover can always be written; plan_lane_ops puts the lane's
queue operations in the order the stage depends on -- the pre-pass, the wait for the pass that last read the copy, the zeroing of the
queue's counts, the kernel, and the dispatch gate last.  tests/emul/plan_primary_emul.cpp is vrt_plan.h behind ctypes."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_SO = os.path.join(HERE, "emul", "_plan_primary_emul.so")
PREPASS, WAIT_PASS, ZERO_QUEUE, PRIMARY_VERTEX, WAIT_GATE = range(5)


@pytest.fixture(scope="module")
def emul():
    src = os.path.join(HERE, "emul", "plan_primary_emul.cpp")
    deps = [src, os.path.join(ROOT, "voxel_rt2_amd", "csrc", "vrt_plan.h")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-Wno-unused-function", "-o", _SO, src],
                       check=True, capture_output=True)
    lib = C.CDLL(_SO)
    lib.primary_decision.argtypes = [C.POINTER(C.c_int)]
    lib.primary_caps.argtypes = [C.c_uint, C.c_int, C.c_longlong, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    lib.primary_lane_ops.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)]
    return lib


def decision(lib, width=1920, height=1080, max_depth=8, knob_render=-1, knob_cull=-1, use_restir=False, instrumented=False, count_as_timed=False,
             ref_oob=False, cull_active=True, dense_grid=False, light_emits=False, fused=4, overlapped=True, lone=False, grid_div=2, prepass=1, primary=1):
    """(pre-pass queued, told, primary).  The defaults are a launch of bench.py: S1 at 1080p, 8 bounces, 4 fused samples, overlapped, half the slots."""
    args = (C.c_int * 18)(width, height, max_depth, knob_render, knob_cull, int(use_restir), int(instrumented), int(count_as_timed), int(ref_oob),
                          int(cull_active), int(dense_grid), int(light_emits), fused, int(overlapped), int(lone), grid_div, prepass, primary)
    bits = lib.primary_decision(args)
    return bool(bits & 1), bool(bits & 2), bool(bits & 4)


def test_the_headline_launch_is_served(emul):
    assert decision(emul) == (True, True, True)
    assert decision(emul, light_emits=True) == (True, True, True), "the sun-lit scene: the emitting-sun instantiation"
    assert decision(emul, cull_active=False) == (True, True, True)
    assert decision(emul, fused=2) == (True, True, True)


EXCLUDED = {
    "lone launch (every slot)": dict(lone=True),
    "not overlapped": dict(overlapped=False),
    "two-deep 4K mode": dict(width=3840, height=2160, grid_div=1),
    "eight-deep small-launch mode": dict(width=1920, height=135, grid_div=4),
    "ReSTIR": dict(use_restir=True, overlapped=False),
    "ReSTIR, were it overlapped": dict(use_restir=True),
    "one-sample call": dict(fused=1),
    "dense12 variant": dict(dense_grid=True, light_emits=True),
    "instrumented (reference counters)": dict(instrumented=True),
    "instrumented (timed counters)": dict(instrumented=True, count_as_timed=True),
    "reference indexing": dict(ref_oob=True),
    "fused schedule": dict(knob_render=0),
    "no pre-pass": dict(prepass=0),
    "pre-pass queued, launch not told": dict(prepass=2),
    "switched off": dict(primary=0),
}


@pytest.mark.parametrize("case", sorted(EXCLUDED))
def test_every_other_launch_is_queued_as_before(emul, case):
    assert decision(emul, **EXCLUDED[case])[2] is False


def test_only_told_launches_are_served(emul):
    """Over every combination of the switches and modes above: primary implies a pre-pass that the launch is told of."""
    for use_restir, instrumented, dense, emits, fused, overlapped, lone, grid_div, prepass, primary in itertools.product(
            (False, True), (False, True), (False, True), (False, True), (1, 4), (False, True), (False, True), (1, 2, 4), (0, 1, 2), (0, 1)):
        q, t, p = decision(emul, use_restir=use_restir, instrumented=instrumented, dense_grid=dense, light_emits=emits, fused=fused, overlapped=overlapped,
                           lone=lone, grid_div=grid_div, prepass=prepass, primary=primary)
        assert p == (q and t and primary == 1)


def test_the_shipped_default(emul):
    assert emul.primary_default_knob() == 1


def caps(lib, tiles, n, knob=0):
    a, b = C.c_uint(), C.c_uint()
    lib.primary_caps(tiles, n, knob, C.byref(a), C.byref(b))
    return a.value, b.value


@pytest.mark.parametrize("tiles,n", [(1, 2), (7, 4), (8, 4), (9, 3), (240 * 135, 4), (41 * 26, 2)])
def test_a_leftover_can_always_be_written(emul, tiles, n):
    """Tile t appends to head t % 8: a head has at most ceil(tiles / 8) tiles of 64 pixels and n samples, and holds that many leftovers."""
    cap, left = caps(emul, tiles, n)
    assert left == -(-tiles // 8) * 64 * n
    assert 0 < cap <= left and cap == (3 * left + 7) // 8, "three eighths of the head's items, rounded up"
    forced, left2 = caps(emul, tiles, n, 64)
    assert forced == min(8, left) and left2 == left


def lane_ops(lib, pre_queue, pre_tell, primary, wait_pass, wait_gate):
    ops = (C.c_int * 5)()
    n = lib.primary_lane_ops(int(pre_queue), int(pre_tell), int(primary), int(wait_pass), int(wait_gate), ops)
    return list(ops[:n])


def test_the_order_of_a_served_launch(emul):
    assert lane_ops(emul, True, True, True, True, True) == [PREPASS, WAIT_PASS, ZERO_QUEUE, PRIMARY_VERTEX, WAIT_GATE]
    assert lane_ops(emul, True, True, True, False, False) == [PREPASS, ZERO_QUEUE, PRIMARY_VERTEX]


def test_the_order_in_every_combination(emul):
    for q, t, p, wp, wg in itertools.product((False, True), repeat=5):
        ops = lane_ops(emul, q, t, p, wp, wg)
        assert ops == sorted(ops) and len(set(ops)) == len(ops), "the order is fixed and nothing is queued twice"
        assert (PREPASS in ops) == q and (WAIT_PASS in ops) == wp and (WAIT_GATE in ops) == wg
        served = q and t and p
        assert (ZERO_QUEUE in ops) == served and (PRIMARY_VERTEX in ops) == served
        if served:   # the counts are zeroed right in front of the kernel, which is behind the pre-pass and the pass, in front of the gate
            assert ops.index(PRIMARY_VERTEX) == ops.index(ZERO_QUEUE) + 1
    # without the stage the lane's operations are the ones it had
    assert lane_ops(emul, True, True, False, True, True) == [PREPASS, WAIT_PASS, WAIT_GATE]
    assert lane_ops(emul, False, False, True, True, True) == [WAIT_PASS, WAIT_GATE]
