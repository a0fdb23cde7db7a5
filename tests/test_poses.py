"""Whole frames from a matrix of camera poses: the host build of the device code (tests/emul) against the oracle under the four
schedules of test_emul_parity.py -- camera inside the grid, inside a block, below the floor, on the grid's faces and corner, looking
away, narrow and wide fields of view -- and render scales 0.75 and 0.3.  tests/poses.py holds the poses and the rules;
tests/test_gpu_poses.py runs the same matrix on the device."""
import pytest

import emu
import poses as P


@pytest.fixture(autouse=True, params=["fused", "pool", "fused+cull", "pool+cull"])
def render_schedule(request, monkeypatch):
    for var, on in (("VRT_EMU_POOL", request.param.startswith("pool")), ("VRT_EMU_CULL", request.param.endswith("+cull"))):
        if on:
            monkeypatch.setenv(var, "1")
        else:
            monkeypatch.delenv(var, raising=False)
    return request.param


def test_oracle_frames_show_the_scene(render_schedule):
    if render_schedule == "fused":    # the oracle's frames alone: once
        P.check_guards()


@pytest.mark.parametrize("case", range(len(P.CASES)), ids=P.IDS)
def test_emulated_frames_equal_oracle(case):
    P.check_matrix(emu.Emulated, case)


@pytest.mark.parametrize("case", range(len(P.SCALED)), ids=["64x40-scale0.75", "100x60-scale0.3"])
def test_emulated_render_scale_sequences_equal_oracle(case):
    P.check_scaled(emu.Emulated, case)
