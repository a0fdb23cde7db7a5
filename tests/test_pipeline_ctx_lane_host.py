"""The pipeline shape whose third render lane is the context's stream (csrc/vrt_plan.h, PipelineShape::ctx_lane), without a GPU:
where plan_pipeline_shape selects it, how launches rotate over its three lanes and seven copies, and what the dispatch gate makes
each launch wait for.  tests/emul/plan_ctx_lane_emul.cpp is vrt_plan.h behind ctypes."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_SO = os.path.join(HERE, "emul", "_plan_ctx_lane_emul.so")
HEADLINE = 1920 * 1080 * 4   # work items of a launch of bench.py: 8.3 M


@pytest.fixture(scope="module")
def emul():
    src = os.path.join(HERE, "emul", "plan_ctx_lane_emul.cpp")
    deps = [src, os.path.join(ROOT, "voxel_rt2_amd", "csrc", "vrt_plan.h")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-Wno-unused-function", "-o", _SO, src],
                       check=True, capture_output=True)
    lib = C.CDLL(_SO)
    lib.ctx_lane_shape.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.ctx_lane_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint)]
    return lib


FIELDS = ("n_streams", "grid_div", "pass_on_render", "defer_k", "ctx_lane", "pass_on_last", "lanes", "n_sets")


def shape(lib, items=HEADLINE, queues=4, heavy=False, can_defer=True, streams=None, grid_div=None, pass_stream=None, ctx_lane=None, defer4=None):
    knobs = (C.c_int * 5)(*[-100 if v is None else v for v in (streams, grid_div, pass_stream, ctx_lane, defer4)])
    out = (C.c_int * 8)()
    lib.ctx_lane_shape(items, int(heavy), queues, int(can_defer), knobs, out)
    return dict(zip(FIELDS, out))


@pytest.mark.parametrize("queues", [4, 5])
def test_the_headline_launch_takes_the_contexts_stream_as_a_lane(emul, queues):
    sh = shape(emul, queues=queues)
    assert sh["ctx_lane"] == 1 and sh["pass_on_last"] == 1
    # what the shape was before stays: two streams of the pipeline's own, half the slots, four launches a pass, pass_on_render off
    assert (sh["n_streams"], sh["grid_div"], sh["defer_k"], sh["pass_on_render"]) == (2, 2, 4, 0)
    assert (sh["lanes"], sh["n_sets"]) == (3, 7)


@pytest.mark.parametrize("case", [dict(queues=6), dict(queues=16), dict(can_defer=False), dict(items=(12 << 20) + 1),
                                  dict(streams=2), dict(streams=3), dict(streams=4), dict(grid_div=2), dict(pass_stream=0), dict(pass_stream=1)],
                         ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_no_other_launch_does(emul, case):
    sh = shape(emul, **case)
    assert sh["ctx_lane"] == 0 and sh["lanes"] == sh["n_streams"] and sh["n_sets"] == sh["n_streams"] + sh["defer_k"]
    assert sh["pass_on_last"] == sh["pass_on_render"]


def test_the_other_fields_are_what_they_were(emul):
    """n_streams, grid_div, defer_k and pass_on_render with the lane and without it (VRT_CTX_LANE=0), for launches of every size
    and both queue counts."""
    for items in (1 << 20, 4 << 20, HEADLINE, 12 << 20, 33 << 20):
        for queues in (4, 5, 6, 16):
            for can_defer in (True, False):
                a, b = shape(emul, items, queues, can_defer=can_defer), shape(emul, items, queues, can_defer=can_defer, ctx_lane=0)
                assert b["ctx_lane"] == 0
                assert all(a[f] == b[f] for f in ("n_streams", "grid_div", "defer_k", "pass_on_render")), (items, queues, can_defer, a, b)


def test_the_switch_overrides_the_choice(emul):
    assert shape(emul, ctx_lane=0)["ctx_lane"] == 0
    assert shape(emul, queues=16, streams=2, ctx_lane=1)["ctx_lane"] == 1
    # the two pass placements of the A/B runs: on the lane of the group's last launch, always on the context's stream
    assert shape(emul, pass_stream=1, ctx_lane=1)["pass_on_last"] == 1
    on_ctx = shape(emul, pass_stream=0, ctx_lane=1)
    assert on_ctx["ctx_lane"] == 1 and on_ctx["pass_on_last"] == 0
    # never where launches cannot be deferred, or are not (a pass per launch belongs on the context's stream, in front of nothing)
    assert shape(emul, can_defer=False, ctx_lane=1)["ctx_lane"] == 0
    assert shape(emul, defer4=1, ctx_lane=1)["ctx_lane"] == 0


def test_rotation_and_gate_of_the_three_lane_shape(emul):
    sh = shape(emul)
    out = (C.c_uint * 40)()
    emul.ctx_lane_run(10, sh["lanes"], sh["n_sets"], sh["grid_div"], out)
    rows = [tuple(out[4 * k:4 * k + 4]) for k in range(10)]
    #        lane set target wait      launch k goes to lane k mod 3 (lane 2: the context's stream) and copy k mod 7; it is dispatched
    want = [(0, 0, 0, 0),            # when launch k - 2 starts to drain, i.e. at the value k - 1 of the drain signal; its lane last held
            (1, 1, 0, 0),            # launch k - 3, which is older than that: the stream wait is queued from launch 2 on
            (2, 2, 1, 1),
            (0, 3, 2, 1),
            (1, 4, 3, 1),
            (2, 5, 4, 1),
            (0, 6, 5, 1),
            (1, 0, 6, 1),
            (2, 1, 7, 1),
            (0, 2, 8, 1)]
    assert rows == want
