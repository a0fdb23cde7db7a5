"""Single rays through the closest-hit walk ON THE DEVICE (vrt_trace_probe, include/vrt_api.h) against the oracle's raytrace, bit for
bit: the three walk variants, with the culling box off and on.  cull_ray (vrt_trace.h) divides with the approximate reciprocal on
the device only, so this is where its 8-voxel margin is put to the test: rays aimed at the faces, edges and corners of the grown
box from either side.  tests/rays.py holds the scenes, the ray families and the rules; tests/test_ray_probe.py runs the same cases
on the host build of the same code."""
import ctypes as C

import numpy as np
import pytest

import orc
import rays as R
from voxel_rt2_amd import _lib
from voxel_rt2_amd._session import NativeSession

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    """device(scene, reference_indexing=False): one prepared context per scene, closed (its device memory released) when the
    module is done."""
    live = {}

    def get(name, reference_indexing=False):
        if (name, reference_indexing) not in live:
            g = NativeSession(_lib.load(), "vrt_", R.config(name))
            mat, rgb, params = R.scene(name)
            orc.setup(g, mat, rgb, params)
            if reference_indexing:
                g.set_reference_indexing(True)
            live[name, reference_indexing] = g
        return live[name, reference_indexing]
    yield get
    for g in live.values():
        g.close()


def probe_of(session):
    def probe(mode, rays):
        out = np.zeros(len(rays), R.REC)
        rc = _lib.load().vrt_trace_probe(C.c_void_p(session._ctx), int(mode), len(rays), orc.fptr(rays), orc.fptr(out))
        assert rc == 0, _lib.load().vrt_last_error()
        return out
    return probe


def test_families_are_what_they_claim():
    R.check_guards()


@pytest.mark.parametrize("scene,fam", R.cases())
def test_device_walks_equal_oracle(device, scene, fam):
    rays, want = R.family(scene, fam)
    culled = R.check_probe(probe_of(device(scene)), rays, want, label=f"{scene}/{fam}",
                           culls=R.scene(scene)[0].shape[0] if fam == "box" and scene in R.CULLING else None)
    if culled:
        print(f"culling {scene}: {culled[0]} of {len(rays)} box-aimed rays culled whole, steps {culled[1]} -> {culled[2]}")


@pytest.mark.parametrize("reference_indexing", [False, True])
def test_device_walks_equal_reference_source_rays(device, reference_indexing):
    """The 600 recorded rays: the reference's own values are the expectation, in both indexing modes (with the reference's indexing
    cell and normal are compared on every ray, and nothing is culled: the box-on modes then walk every ray too)."""
    rays, want = R.recorded()
    R.check_probe(probe_of(device("sunlit", reference_indexing)), rays, want, cells="all" if reference_indexing else "finite",
                  label=f"recorded, reference_indexing={reference_indexing}")


def test_probe_needs_prepare_and_a_known_mode(device):
    lib = _lib.load()
    g = NativeSession(lib, "vrt_", R.config("sunlit"))
    ray = np.array([[66.5, 100.0, 66.25, 0.0, -1.0, 0.0]], np.float32)
    out = np.zeros(1, R.REC)
    assert lib.vrt_trace_probe(C.c_void_p(g._ctx), 0, 1, orc.fptr(ray), orc.fptr(out)) == -3      # VRT_E_STATE: before vrt_prepare
    g.close()
    g = device("sunlit")
    for mode in (3, 7, 8, -1):
        assert lib.vrt_trace_probe(C.c_void_p(g._ctx), mode, 1, orc.fptr(ray), orc.fptr(out)) == -1  # VRT_E_INVALID
    want = R.oracle_trace("sunlit", ray)
    for mode in (0, 1, 2):
        assert probe_of(g)(mode, ray).tobytes() == want.tobytes()
    # a ray inside the grid that stays clear of the grown box: walked without the box, culled with it -- the record vrt_api.h states
    clear = np.array([[5.0, 120.0, 5.0, 1.0, 0.01, 0.02]], np.float32)
    walked = R.oracle_trace("sunlit", clear)
    assert np.isinf(walked["dist"][0]) and walked["iters"][0] > 0
    for mode in (0, 1, 2):
        assert probe_of(g)(mode, clear).tobytes() == walked.tobytes(), mode
        got = probe_of(g)(mode | R.BOX, clear)[0]
        assert np.isinf(got["dist"]) and got["cell"].tolist() == [-1, -1, -1] and got["normal"].tolist() == [0.0, 0.0, 0.0] and got["iters"] == 0, (mode, got)
