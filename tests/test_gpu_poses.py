"""Whole frames from a matrix of camera poses ON THE DEVICE against the oracle, bit for bit, under both render schedules: camera
inside the grid, inside a block, below the floor, on the grid's faces and corner, looking away (every camera ray culled), narrow
and wide fields of view; ReSTIR on three of them; render scales 0.75 and 0.3.  This is where the device-only parts meet other
poses than the default one: the approximate reciprocal of cull_ray, the pyramid in LDS, the pooled kernel's suspended walks, the
twelve-wave dense kernel, the camera rays the fused samples share.  tests/poses.py holds the poses and the rules;
tests/test_poses.py runs the same matrix on the host build of the device code."""
import pytest

import poses as P
from voxel_rt2_amd import _lib
from voxel_rt2_amd._session import NativeSession

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["pool", "fused"])
def render_schedule(request, monkeypatch):
    monkeypatch.setenv("VRT_RENDER", request.param)
    return request.param


def gpu_session(cfg):
    return NativeSession(_lib.load(), "vrt_", cfg)


def test_oracle_frames_show_the_scene(render_schedule):
    if render_schedule == "pool":     # the oracle's frames alone: once
        P.check_guards()


@pytest.mark.parametrize("case", range(len(P.CASES)), ids=P.IDS)
def test_device_frames_equal_oracle(case):
    P.check_matrix(gpu_session, case)


@pytest.mark.parametrize("case", range(len(P.SCALED)), ids=["64x40-scale0.75", "100x60-scale0.3"])
def test_device_render_scale_sequences_equal_oracle(case):
    P.check_scaled(gpu_session, case)
