"""The launch pipeline's decisions (voxel_rt2_amd/csrc/vrt_plan.h: shape, deferral depth, fused sample count, timer period, dispatch
gate, workgroups, set and lane of a launch) as plain functions, compiled for the host (tests/emul/plan_emul.cpp).  The expected
values are literals: what the library decided before the decisions were lifted out of vrt_accumulate.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_SO = os.path.join(HERE, "emul", "_plan_emul.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(HERE, "emul", "plan_emul.cpp")
        deps = [src, os.path.join(ROOT, "voxel_rt2_amd", "csrc", "vrt_plan.h")]
        if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
            subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-Wno-unused-function", "-o", _SO, src],
                           check=True, capture_output=True)
        _lib = C.CDLL(_SO)
        _lib.plan_shape.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _lib.plan_period.argtypes = [C.c_int, C.c_int, C.c_longlong]
        _lib.plan_period.restype = C.c_uint
        _lib.plan_deep_items.restype = C.c_longlong
        _lib.plan_target.argtypes = [C.c_uint, C.c_int, C.c_int, C.c_int, C.c_uint]
        _lib.plan_target.restype = C.c_uint
        _lib.plan_wait.argtypes = [C.c_uint, C.c_uint, C.c_int, C.c_int]
        _lib.plan_set.argtypes = _lib.plan_lane.argtypes = [C.c_uint, C.c_int]
    return _lib


def shape(items, queues, heavy=False, can_defer=True, streams=None, grid_div=None, pass_stream=None, defer4=None, defer8=None):
    """((n_streams, grid_div), defer_k, pass_on_render)"""
    knobs = (C.c_int * 5)(*[-100 if v is None else v for v in (streams, grid_div, pass_stream, defer4, defer8)])
    out = (C.c_int * 4)()
    lib().plan_shape(items, int(heavy), queues, int(can_defer), knobs, out)
    return (out[0], out[1]), out[3], bool(out[2])


P1080 = 1920 * 1080
DEEP = 12 << 20

# (items, heavy, queues) -> (n_streams, grid_div), defer_k (None: the issue's table states no K for the case)
SHAPES = [
    (P1080 * 4, False, 4, (2, 2), 4),      # the queue-lean shape
    (P1080 * 4, False, 6, (4, 2), 4),
    (P1080 * 4, False, 16, (4, 2), 4),
    (P1080 * 4, False, 5, (2, 2), None),   # lean
    (P1080, False, 16, (8, 4), 1),
    (P1080, False, 15, (4, 2), None),
    (P1080, False, 4, (2, 2), 4),
    (P1080, True, 16, (8, 4), None),       # heavy: 4 147 200 <= 9 * 2^19
    (2400000, True, 16, (4, 2), None),
    (DEEP, False, 16, (4, 2), None),       # exactly the deep limit
    (DEEP + 1, False, 16, (2, 1), 1),
    (3840 * 2160 * 4, False, 16, (2, 1), 1),
]


@pytest.mark.parametrize("items,heavy,queues,want,want_k", SHAPES)
def test_pipeline_shape(items, heavy, queues, want, want_k):
    assert P1080 * 4 == 8294400 and P1080 == 2073600
    got, k, pass_on_render = shape(items, queues, heavy=heavy)
    assert got == want
    assert not pass_on_render
    if want_k is not None:
        assert k == want_k
    # a context whose launches are never deferred pays for no copies, whatever the shape
    assert shape(items, queues, heavy=heavy, can_defer=False) == (want, 1, False)


def test_development_overrides():
    assert lib().plan_max_sets() == 12
    assert shape(P1080 * 4, 4, streams=3, defer4=4)[:2] == ((3, 2), 4)
    assert shape(P1080 * 4, 4, streams=2, grid_div=1, defer4=4)[:2] == ((2, 1), 1)
    assert shape(P1080 * 4, 16, pass_stream=1)[2] is True
    assert shape(P1080 * 4, 16, pass_stream=0)[2] is False
    assert shape(P1080 * 4, 16)[2] is False
    # VRT_DEFER=8: K 8 at four streams, clamped to VRT_MAX_SETS - n_streams = 12 - 8 at eight, 8 at two streams of half-size launches
    assert shape(P1080 * 4, 16, defer4=8, defer8=8)[:2] == ((4, 2), 8)
    assert shape(P1080, 16, defer4=8, defer8=8)[:2] == ((8, 4), 4)
    assert shape(P1080 * 4, 4, defer4=8, defer8=8)[:2] == ((2, 2), 8)
    assert shape(P1080 * 4, 16, streams=2, grid_div=2, defer4=8, defer8=8)[:2] == ((2, 2), 8)


def test_dispatch_gate():
    L = lib()
    # four streams of half-size launches: launch 10 takes the slots of launch 8, which raises the word to 9
    assert L.plan_target(10, 0, 2, 0, 0) == 9
    assert L.plan_wait(9, 7, 1, 1) == 1      # the lane's last launch was number 6: the wait is queued
    # two streams in steady state: the lane's last launch IS number 8 -- stream order says what the wait would
    assert L.plan_wait(9, 9, 1, 1) == 0
    assert L.plan_target(10, 1, 2, 0, 0) == 10   # the previous launch took every slot: its own drain
    assert L.plan_target(10, 1, 4, 3, 0) == 10
    assert L.plan_target(10, 0, 2, 0, 10) == 10  # never for a launch older than the last full one
    assert L.plan_target(10, 0, 4, 0, 8) == 8
    assert L.plan_target(10, 0, 4, 0, 0) == 7
    assert L.plan_target(10, 0, 2, 1, 0) == 8    # VRT_GATE_EXTRA=1
    assert L.plan_target(0, 1, 2, 0, 0) == 0 and L.plan_wait(0, 0, 1, 1) == 0   # the first launch waits for nothing
    assert L.plan_target(1, 0, 2, 0, 0) == 0
    assert L.plan_wait(9, 7, 0, 1) == 0      # no gate
    assert L.plan_wait(9, 7, 1, 0) == 0      # the most recent launch was not given the signal
    assert L.plan_wait(9, 8, 1, 1) == 1 and L.plan_wait(9, 0, 1, 1) == 1 and L.plan_wait(9, 10, 1, 1) == 0


def test_workgroups_of_a_partial_launch():
    L = lib()
    assert L.plan_blocks(512, 2) == 256
    assert L.plan_blocks(520, 2) == 264
    assert L.plan_blocks(520, 4) == 136
    assert L.plan_blocks(520, 1) == 520 and L.plan_blocks(516, 1) == 520   # whole rounds of the 8 XCDs


def test_timer_period():
    L = lib()
    assert L.plan_deep_items() == DEEP
    assert L.plan_period(0, 0, P1080 * 4) == 8
    assert L.plan_period(0, 0, DEEP) == 8
    assert L.plan_period(0, 0, DEEP + 1) == 1
    assert L.plan_period(0, 1, P1080) == 1       # ReSTIR
    assert L.plan_period(5, 0, P1080) == 5 and L.plan_period(5, 1, DEEP + 1) == 5


def test_fused_sample_count():
    L = lib()
    assert L.plan_fused(9, 1, 4) == 4
    assert L.plan_fused(1, 1, 4) == 1
    assert L.plan_fused(3, 0, 4) == 1
    assert L.plan_fused(3, 1, 4) == 3
    assert L.plan_fused(4, 1, 4) == 4 and L.plan_fused(5, 1, 2) == 2 and L.plan_fused(2, 1, 1) == 1


def test_set_and_lane_take_turns():
    L = lib()
    # two streams, K = 4: six copies; four streams, K = 4: eight
    assert [L.plan_set(q, 6) for q in range(8)] == [0, 1, 2, 3, 4, 5, 0, 1]
    assert [L.plan_lane(q, 2) for q in range(5)] == [0, 1, 0, 1, 0]
    assert (L.plan_set(13, 8), L.plan_lane(13, 4)) == (5, 1)
    assert (L.plan_set(2**32 - 1, 12), L.plan_lane(2**32 - 1, 8)) == (3, 7)
