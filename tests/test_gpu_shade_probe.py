"""Single shading functions ON THE DEVICE (vrt_shade_probe, include/vrt_api.h; k_shade_probe runs the row function of
vrt_shade_probe.h that tests/test_shade_probe.py runs on the host): every row of functions.npz and functions_edges.npz as the reference's
own source computed it, the random rows of tests/shading.py against the oracle, the shift_is_constant property and the hook's guards.
Bit for bit; the BSDF rows in all three formulations.  One 16x8 context on the sun-lit scene for the whole module."""
import ctypes as C

import numpy as np
import pytest

import orc
import shading
from voxel_rt2_amd import host, scenes

pytestmark = pytest.mark.gpu


def _session(prepare=True):
    from voxel_rt2_amd import _lib
    from voxel_rt2_amd._session import NativeSession
    mat, rgb, params = scenes.scene_sunlit(0)
    g = NativeSession(_lib.load(), "vrt_", host.make_config(16, 8, max_depth=2))
    if prepare:
        orc.setup(g, mat, rgb, params)
    return g


@pytest.fixture(scope="module")
def session():
    g = _session()
    yield g
    g.close()


@pytest.fixture(scope="module")
def run(session):
    from voxel_rt2_amd import _lib
    lib = _lib.load()

    def run(op, rows, n_out):
        rows = np.ascontiguousarray(rows, np.float32)
        out = np.zeros((len(rows), n_out), np.float32)
        rc = lib.vrt_shade_probe(C.c_void_p(session._ctx), int(op), len(rows), orc.fptr(rows), rows.shape[1], orc.fptr(out), n_out)
        assert rc == 0, lib.vrt_last_error()
        return out
    return run


def test_gpu_shading_equals_reference_source(run):
    shading.check_reference(run)


def test_gpu_shading_equals_oracle(run):
    shading.check_oracle_rows(run)


def test_gpu_guards(session):
    from voxel_rt2_amd import _lib
    lib = _lib.load()

    def call_on(s):
        def call(op, rows, in_stride, out_stride):
            n = 1 if rows is None else len(rows)
            out = np.zeros((n, max(out_stride, 1)), np.float32)
            return lib.vrt_shade_probe(C.c_void_p(s._ctx), int(op), n, None if rows is None else orc.fptr(rows), int(in_stride), orc.fptr(out), int(out_stride))
        return call
    cold = _session(prepare=False)
    shading.check_guards(call_on(session), call_on(cold))
    cold.close()
