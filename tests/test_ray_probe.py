"""Single rays through the device code's closest-hit walk, compiled for the host (emu_trace_probe, tests/emul/emul.cpp: the function
vrt_trace_probe runs on the device, vrt_probe.h) against the oracle's raytrace -- the hook's record layout and modes, the three
walk variants, and the culling box with exact division.  tests/rays.py holds the scenes, the ray families and the rules;
tests/test_gpu_ray_probe.py runs the same cases on the device, where cull_ray divides with the approximate reciprocal."""
import ctypes as C

import numpy as np
import pytest

import emu
import orc
import rays as R


@pytest.fixture(scope="module")
def emulated():
    """emulated(scene, reference_indexing=False): one prepared session per scene, closed when the module is done."""
    live = {}

    def get(name, reference_indexing=False):
        if (name, reference_indexing) not in live:
            e = emu.Emulated(R.config(name))
            mat, rgb, params = R.scene(name)
            orc.setup(e, mat, rgb, params)
            if reference_indexing:
                e.set_reference_indexing(True)
            live[name, reference_indexing] = e
        return live[name, reference_indexing]
    yield get
    for e in live.values():
        e.close()


def probe_of(session):
    def probe(mode, rays):
        out = np.zeros(len(rays), R.REC)
        assert emu.lib().emu_trace_probe(C.c_void_p(session._ctx), int(mode), len(rays), orc.fptr(rays), orc.fptr(out)) == 0
        return out
    return probe


def test_families_are_what_they_claim():
    R.check_guards()


@pytest.mark.parametrize("scene,fam", R.cases())
def test_emulated_walks_equal_oracle(emulated, scene, fam):
    rays, want = R.family(scene, fam)
    culled = R.check_probe(probe_of(emulated(scene)), rays, want, label=f"{scene}/{fam}",
                           culls=R.scene(scene)[0].shape[0] if fam == "box" and scene in R.CULLING else None)
    if culled:
        print(f"culling {scene}: {culled[0]} of {len(rays)} box-aimed rays culled whole, steps {culled[1]} -> {culled[2]}")


@pytest.mark.parametrize("reference_indexing", [False, True])
def test_emulated_walks_equal_reference_source_rays(emulated, reference_indexing):
    """The 600 recorded rays: the reference's own values are the expectation, in both indexing modes (with the reference's indexing
    cell and normal are compared on every ray, and nothing is culled: the box-on modes then walk every ray too)."""
    rays, want = R.recorded()
    R.check_probe(probe_of(emulated("sunlit", reference_indexing)), rays, want, cells="all" if reference_indexing else "finite",
                  label=f"recorded, reference_indexing={reference_indexing}")


def test_probe_layout_and_modes(emulated):
    """One known ray: straight down onto the top of a sunlit block; every mode gives the same 32-byte record.  Bad modes are refused."""
    e = emulated("sunlit")
    ray = np.array([[66.5, 100.0, 66.25, 0.0, -1.0, 0.0]], np.float32)
    want = R.oracle_trace("sunlit", ray)
    assert np.isfinite(want["dist"][0]) and want["cell"][0].tolist()[0::2] == [66, 66] and want["normal"][0].tolist() == [0.0, 1.0, 0.0]
    for mode in (0, 1, 2, 4, 5, 6):
        got = probe_of(e)(mode, ray)
        assert got.tobytes() == want.tobytes() or mode >= 4 and got[["dist", "cell", "normal"]].tobytes() == want[["dist", "cell", "normal"]].tobytes(), mode
    # a ray inside the grid that stays clear of the grown box: walked without the box, culled with it -- the record vrt_api.h states
    clear = np.array([[5.0, 120.0, 5.0, 1.0, 0.01, 0.02]], np.float32)
    walked = R.oracle_trace("sunlit", clear)
    assert np.isinf(walked["dist"][0]) and walked["iters"][0] > 0
    for mode in (0, 1, 2):
        assert probe_of(e)(mode, clear).tobytes() == walked.tobytes(), mode
        got = probe_of(e)(mode | R.BOX, clear)[0]
        assert np.isinf(got["dist"]) and got["cell"].tolist() == [-1, -1, -1] and got["normal"].tolist() == [0.0, 0.0, 0.0] and got["iters"] == 0, (mode, got)
    out = np.zeros(1, R.REC)
    for mode in (3, 7, 8, -1):
        assert emu.lib().emu_trace_probe(C.c_void_p(e._ctx), mode, 1, orc.fptr(ray), orc.fptr(out)) != 0
