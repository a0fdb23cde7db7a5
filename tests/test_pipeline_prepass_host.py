"""The camera-ray pre-pass in the launch plan (csrc/vrt_plan.h), without a GPU: plan_prepass names the launches that get one -- the
overlapped launches of half the workgroup slots whose fused samples share the record table, i.e. the headline's -- and every other
mode keeps its launches as they were; LaunchSeq never hands a tag that a pre-pass carries to any other launch, whether the
pre-pass's own launch was queued or not.  tests/emul/plan_prepass_emul.cpp is vrt_plan.h behind ctypes."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_SO = os.path.join(HERE, "emul", "_plan_prepass_emul.so")
HEADLINE = 1920 * 1080 * 4


@pytest.fixture(scope="module")
def emul():
    src = os.path.join(HERE, "emul", "plan_prepass_emul.cpp")
    deps = [src, os.path.join(ROOT, "voxel_rt2_amd", "csrc", "vrt_plan.h")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-Wno-unused-function", "-o", _SO, src],
                       check=True, capture_output=True)
    lib = C.CDLL(_SO)
    lib.prepass_decision.argtypes = [C.POINTER(C.c_int)]
    lib.prepass_grid_div.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_int]
    lib.prepass_run.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    return lib


def decision(lib, width=1920, height=1080, max_depth=8, knob_render=-1, knob_cull=-1, use_restir=False, instrumented=False, count_as_timed=False,
             ref_oob=False, cull_active=True, dense_grid=False, light_emits=False, fused=4, overlapped=True, lone=False, grid_div=2, knob=1):
    """(queued, told).  The defaults are a launch of bench.py: S1 at 1080p, 8 bounces, 4 fused samples, overlapped, half the slots."""
    args = (C.c_int * 17)(width, height, max_depth, knob_render, knob_cull, int(use_restir), int(instrumented), int(count_as_timed), int(ref_oob),
                          int(cull_active), int(dense_grid), int(light_emits), fused, int(overlapped), int(lone), grid_div, knob)
    bits = lib.prepass_decision(args)
    return bool(bits & 1), bool(bits & 2)


@pytest.mark.parametrize("queues", [4, 16])
def test_the_headline_launch_has_a_pre_pass(emul, queues):
    """With four hardware queues (the queue-lean shape with the context's stream as a lane) and with sixteen (four streams)."""
    assert emul.prepass_grid_div(HEADLINE, 0, queues, 1) == 2
    assert decision(emul) == (True, True)
    assert decision(emul, light_emits=True) == (True, True), "the sun-lit scene: the emitting-sun instantiation"
    assert decision(emul, cull_active=False) == (True, True), "a scene without a culling box"
    assert decision(emul, fused=2) == (True, True)


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
    "switched off": dict(knob=0),
}


@pytest.mark.parametrize("case", sorted(EXCLUDED))
def test_every_other_mode_keeps_its_launches(emul, case):
    assert decision(emul, **EXCLUDED[case]) == (False, False)


def test_the_shapes_that_exclude_are_the_shapes_those_modes_run_in(emul):
    """grid_div of the excluded frame sizes above, from plan_pipeline_shape itself."""
    assert emul.prepass_grid_div(3840 * 2160 * 4, 0, 16, 1) == 1 and emul.prepass_grid_div(3840 * 2160 * 4, 0, 4, 1) == 1
    assert emul.prepass_grid_div(1920 * 135 * 4, 0, 16, 1) == 4
    assert emul.prepass_grid_div(HEADLINE // 2, 0, 16, 1) == 4      # half a frame, sixteen queues: eight-deep
    assert emul.prepass_grid_div(HEADLINE // 2, 0, 4, 1) == 2       # ... four queues: the headline's shape


def test_mode_2_queues_and_does_not_tell(emul):
    assert decision(emul, knob=2) == (True, False)
    for case in EXCLUDED.values():
        if "knob" not in case:
            assert decision(emul, **dict(case, knob=2)) == (False, False)


def test_the_shipped_default(emul):
    assert emul.prepass_default_knob() == 1


def _run(lib, events):
    ev = (C.c_int * len(events))(*events)
    pre, launch = (C.c_uint * len(events))(), (C.c_uint * len(events))()
    lib.prepass_run(len(events), ev, pre, launch)
    return list(pre), list(launch)


def test_tags_are_unique_across_a_queued_then_aborted_launch(emul):
    #          a launch, three with a pre-pass, a pre-pass whose launch fails, then the run goes on
    events = [0, 1, 1, 1, 2, 1, 0, 1]
    pre, launch = _run(emul, events)
    assert launch == [1, 2, 3, 4, 0, 6, 7, 8] and pre == [0, 2, 3, 4, 5, 6, 0, 8]
    for k, e in enumerate(events):
        if e == 1:
            assert pre[k] == launch[k] != 0, "a pre-pass carries exactly its launch's tag"
    assert 5 not in launch, "the tag of the pre-pass whose launch never came is burnt"


def test_tags_are_unique_in_every_short_history(emul):
    """Every sequence of six events: no tag is handed to two launches, nor to a pre-pass and another event's launch, and none is 0."""
    for events in itertools.product(range(4), repeat=6):
        pre, launch = _run(emul, list(events))
        owners = {}
        for k, (p, l) in enumerate(zip(pre, launch)):
            for tag in {p, l} - {0}:
                assert owners.setdefault(tag, k) == k, (events, pre, launch)
            assert (p != 0) == (events[k] in (1, 2)) and (l != 0) == (events[k] != 2)
            if p and l:
                assert p == l
