"""vrt_distance_field WITHOUT a GPU: the host build of voxel_rt2_amd/csrc/vrt_distance.h (tests/emul/distance_emul.cpp: the kernels' loops,
the entry point's checks, plan_distance_layout's scratch) against two numpy brute forces that know nothing of a separable transform
(tests/distance.py).  Byte for byte, on d2 and on nearest, over every cell of every box:
  - every case family of tests/distance.py at 128^3 and one at 256^3: an empty and a full grid under both flags, single solids in the grid's
    corners, ties along each axis and across the axes (the smallest linear index wins), max_d2 = 0 / exactly D / D - 1 / the largest
    allowed, targets only outside the box (inside the grown box, and just outside it), boxes on every grid face, a cell, lines, a box
    that is no multiple of any tile, a half-full grid under both flags, a grid after an emulated edit;
  - the two brute forces agree where both are affordable;
  - a request without `nearest` gives the same d2 bytes and touches less scratch; the plan's byte count bounds what is touched (a guard
    behind it comes back untouched on every call above);
  - the grown box; export, ctypes binding, constants, the error codes that need no device;
  - a stand-alone program built from distance_emul.cpp with -fsanitize=address,undefined runs three families clean."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import distance as D
import edit as E
import rays as R
from voxel_rt2_amd import _abi, _lib


@pytest.mark.parametrize("name", D.NAMES_128 + D.HOST_256)
def test_emulation_equals_brute_force(name):
    c = D.CASES[name]
    rc, d2, near = D.emul_call(D.grid(c["grid"]), c["lo"], c["hi"], c["max_d2"], c["to_empty"])
    assert rc == _abi.VRT_OK
    D.check(d2, near, D.expected(name), name)


def test_the_cases_are_what_they_claim():
    far = lambda n: D.expected(n)[0] == D.FAR
    assert far("empty").all() and far("full_to_empty").all() and (D.expected("empty")[1] == -1).all()
    assert (D.expected("full")[0] == 0).all() and (D.expected("empty_to_empty")[0] == 0).all()
    d2, near = D.expected("twelve")
    G, c = 128, D.C0
    at = tuple(10 for _ in range(3))                                                           # the centre cell of the box
    first = min((c[0] + s * o[0]) * G * G + (c[1] + s * o[1]) * G + c[2] + s * o[2] for o in D.TWELVE for s in (-1, 1))
    assert d2[at] == 25 and near[at] == first == ((c[0] - 5) * G + c[1]) * G + c[2]
    for a in range(3):                                                                         # -k wins over +k on every axis
        d2, near = D.expected("tie_" + "xyz"[a])
        lo = [c[k] - (D.TIE_K if k == a else 0) for k in range(3)]
        assert d2[at] == D.TIE_K ** 2 and near[at] == (lo[0] * G + lo[1]) * G + lo[2]
    assert (D.expected("maxd2_exact")[0] != D.FAR).sum() == 1 and D.expected("maxd2_exact")[0][0, 0, 0] == 25
    assert far("maxd2_minus").all() and far("outside_out").all() and (D.expected("outside_in")[0] == 16).sum() == 1
    z = D.expected("maxd2_0")[0]
    assert set(np.unique(z).tolist()) == {0, D.FAR}
    assert D.CASES["s1_unbounded"]["max_d2"] == _abi.DIST_MAX_D2 and not far("s1_unbounded").any()


def test_the_two_brute_forces_agree():
    for name in ("twelve_25", "maxd2_0", "odd_box", "s1_edit"):
        c = D.CASES[name]
        m = D.grid(c["grid"])
        assert all(D.affordable(m, c["lo"], c["hi"], c["max_d2"], c["to_empty"])), name
        a = D.brute_targets(m, c["lo"], c["hi"], c["max_d2"], c["to_empty"])
        b = D.brute_offsets(m, c["lo"], c["hi"], c["max_d2"], c["to_empty"])
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), name


def test_after_an_emulated_edit():
    """the edit goes through edit_emul.cpp's loops into a HostGrid; the field is then asked of its materials"""
    g = E.HostGrid(*R.scene("s1")[:2])
    c = D.CASES["s1_edit"]
    before = D.emul_call(g.mat, c["lo"], c["hi"], c["max_d2"])
    g.apply(*D.S1_EDIT)
    assert g.mat.tobytes() == D.grid("s1_edit").tobytes()
    rc, d2, near = D.emul_call(g.mat, c["lo"], c["hi"], c["max_d2"])
    D.check(d2, near, D.expected("s1_edit"), "s1 after an edit")
    assert before[1].tobytes() != d2.tobytes()


@pytest.mark.parametrize("name", ["twelve", "s1_unbounded", "dense_9_to_empty", "face_x0", "cell_d0", "corners_256"])
def test_without_nearest_the_same_d2_and_less_scratch(name):
    c = D.CASES[name]
    m = D.grid(c["grid"])
    rc, d2, near = D.emul_call(m, c["lo"], c["hi"], c["max_d2"], c["to_empty"], nearest=False)
    assert rc == _abi.VRT_OK and near is None and d2.tobytes() == D.expected(name)[0].tobytes()
    G = m.shape[0]
    (glo, ghi), b = D.emul_grown(G, c["lo"], c["hi"], c["max_d2"]), [h - l for l, h in zip(c["lo"], c["hi"])]
    g = [h - l for l, h in zip(glo, ghi)]
    values = 4 * g[0] * g[1] * b[2] + 4 * g[0] * b[1] * b[2]
    coords = g[0] * g[1] * b[2] + g[0] * b[1] * b[2]
    slack = 5 * 256 + 256                                                                      # every part rounded up to 256 bytes
    with_n, without = D.emul_plan(G, c["lo"], c["hi"], c["max_d2"]), D.emul_plan(G, c["lo"], c["hi"], c["max_d2"], nearest=False)
    assert values <= without <= values + slack and values + coords <= with_n <= values + coords + slack
    assert with_n <= 10 * g[0] * g[1] * g[2] + slack                                           # "a few bytes per voxel of the grown box"


def test_grown_box():
    G = 128
    assert D.emul_grown(G, (10, 20, 30), (11, 22, 33), 16) == ([6, 16, 26], [15, 26, 37])
    assert D.emul_grown(G, (10, 20, 30), (11, 22, 33), 15) == ([7, 17, 27], [14, 25, 36])       # floor(sqrt(15)) = 3
    assert D.emul_grown(G, (10, 20, 30), (11, 22, 33), 0) == ([10, 20, 30], [11, 22, 33])
    assert D.emul_grown(G, (2, 20, 125), (11, 22, 128), 25) == ([0, 15, 120], [16, 27, 128])    # cut by the grid on one side of two axes
    assert D.emul_grown(G, (60, 60, 60), (61, 61, 61), 3 * 127 * 127) == ([0, 0, 0], [128, 128, 128])
    assert D.emul_grown(256, (60, 60, 60), (61, 61, 61), _abi.DIST_MAX_D2) == ([0, 0, 0], [256, 256, 256])


def test_export_binding_constants_and_error_codes():
    assert "vrt_distance_field" in _lib.exported_symbols()
    hdr = open(D.ROOT + "/include/vrt_api.h").read()
    assert int(re.search(r"#define VRT_DIST_FAR\s+(\w+)", hdr).group(1), 16) == _abi.DIST_FAR == 0x7FFFFFFF
    assert int(re.search(r"#define VRT_DIST_MAX_D2\s+(\d+)", hdr).group(1)) == _abi.DIST_MAX_D2 == 3 * 255 * 255
    assert int(re.search(r"VRT_DIST_TO_EMPTY = (\d+)", hdr).group(1)) == _abi.DIST_TO_EMPTY == 1
    hip = _lib.load()
    _abi.declare(hip, "vrt_")
    fn = hip.vrt_distance_field
    assert fn.restype is C.c_int and len(fn.argtypes) == 8 and fn.argtypes[3] is C.c_int32 and fn.argtypes[4] is C.c_uint32
    out = np.zeros(1, np.int32)
    assert fn(None, (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(1, 1, 1), 0, 0, out.ctypes.data_as(C.c_void_p), None, 0) == _abi.VRT_E_INVALID
    # the entry point's checks, as the emulation repeats them
    m = D.grid("lone")
    call = lambda lo=(1, 1, 1), hi=(2, 2, 2), max_d2=4, flags=0: D.emul_call(m, lo, hi, max_d2, flags=flags)[0]
    assert call() == _abi.VRT_OK
    assert call(max_d2=-1) == call(max_d2=_abi.DIST_MAX_D2 + 1) == call(flags=2) == call(flags=0x80000001) == _abi.VRT_E_INVALID
    for lo, hi in (((2, 1, 1), (1, 2, 2)), ((-1, 0, 0), (0, 1, 1)), ((127, 127, 127), (128, 128, 129))):
        assert call(lo, hi) == _abi.VRT_E_INVALID, (lo, hi)
    rc, d2, near = D.emul_call(m, (5, 5, 5), (5, 9, 9), 4)                                     # an empty box: OK, nothing written
    assert rc == _abi.VRT_OK and d2.shape == (0, 4, 4)
    assert call(max_d2=_abi.DIST_MAX_D2) == call(max_d2=0) == _abi.VRT_OK


def test_standalone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "distance_emul_asan")
    build = subprocess.run(D.GCC[:1] + ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DDISTANCE_EMUL_MAIN",
                                        "-Wno-unknown-pragmas", "-o", exe, D._SRC], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    for family in ("sparse", "dense", "ties"):
        run = subprocess.run([exe, family], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-3000:]
        assert run.stdout.rstrip().endswith("ok") and family in run.stdout
