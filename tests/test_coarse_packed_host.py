"""The packed coarse entry of the pooled render kernels' staged 128^3 view, on the host: voxel_rt2_amd/csrc/vrt_trace.h compiled with g++
(tests/emul/coarse_packed_emul.cpp).  A host pyramid type that declares `coarse_packed`, with its table of {l1 word, coarse_pack()} filled
by the loop render_pool_body stages it with, is walked through descend_flat() for EVERY cell of the grid and EVERY start level 0..6, and
the level it returns, `solid` and `nq` must equal what the branchy descend() returns on GlobalPyramid -- exactly, no query left out.  And
coarse_pack() itself against the expressions it folds (descend_flat()'s unpacked ones and cell_occupied()'s), for all 512 l1 cells.
The levels come from the numpy rebuild of tests/edit.py, the compacted fine level from numpy here: nothing of the code under test builds
its own input."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import edit as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_SO = os.path.join(HERE, "emul", "_coarse_packed_emul.so")
G = 128


@functools.lru_cache(maxsize=None)
def lib():
    src = os.path.join(HERE, "emul", "coarse_packed_emul.cpp")
    csrc = os.path.join(ROOT, "voxel_rt2_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("vrt_trace.h", "vrt_types.h")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-o", _SO, src], check=True, capture_output=True)
    so = C.CDLL(_SO)
    so.cp_compare_descents.restype = C.c_longlong
    so.cp_compare_descents.argtypes = [C.c_void_p] * 7
    so.cp_check_pack.restype = C.c_int
    so.cp_check_pack.argtypes = [C.c_void_p] * 6
    return so


def corners():
    mat = np.zeros((G, G, G), np.int8)
    for x in (0, G - 1):
        for y in (0, G - 1):
            for z in (0, G - 1):
                mat[x, y, z] = 1
    return mat


def one_voxel():
    mat = np.zeros((G, G, G), np.int8)
    mat[77, 5, 126] = 1
    return mat


def random_fill(p, seed):
    return (np.random.default_rng([20250701, seed]).random((G, G, G)) < p).astype(np.int8)


GRIDS = {
    "empty": lambda: np.zeros((G, G, G), np.int8),
    "one_voxel": one_voxel,
    "corners": corners,
    "p0.001": lambda: random_fill(0.001, 1),
    "p0.05": lambda: random_fill(0.05, 2),
    "p0.5": lambda: random_fill(0.5, 3),
    "full": lambda: np.ones((G, G, G), np.int8),
}


def levels(mat):
    """l0, l1, l2 (tests/edit.py: numpy, from scratch) and the compacted fine level: the non-zero l0 words in (l1 word, bit) order and
    where each l1 word's run starts (Pyramid::l0c / l0c_base, vrt_types.h), 513 entries: the last is the count."""
    w = E.rebuild(mat, np.zeros(mat.shape + (3,), np.uint8))
    l0, l1, l2 = (np.ascontiguousarray(w[k], "<u8") for k in ("l0", "l1", "l2"))
    by_l1 = l0.reshape(8, 4, 8, 4, 8, 4).transpose(0, 2, 4, 1, 3, 5).reshape(512, 64)   # [l1 word (z, y, x)][bit z*16 + y*4 + x]
    full = by_l1 != 0
    base = np.concatenate([[0], np.cumsum(full.sum(axis=1))]).astype(np.uint32)
    l0c = np.ascontiguousarray(by_l1[full])
    for i in np.flatnonzero(l1)[:5]:                                                    # (the layout this builds is the documented one)
        bits = [b for b in range(64) if (int(l1[i]) >> b) & 1]
        assert full[i].sum() == len(bits) and all(full[i][b] for b in bits)
    return l0, l1, l2, np.concatenate([l0c, np.zeros(1, "<u8")]), base                  # (never empty: ctypes wants an address)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("name", GRIDS)
def test_packed_flat_descent_equals_branchy_descent(name):
    mat = GRIDS[name]()
    l0, l1, l2, l0c, base = levels(mat)
    first, loads = np.zeros(10, np.int32), C.c_longlong(0)
    bad = lib().cp_compare_descents(ptr(l0), ptr(l1), ptr(l2), ptr(l0c), ptr(base), ptr(first), C.byref(loads))
    x, y, z, start, *rest = (int(v) for v in first)
    assert bad == 0, (f"{name}: {bad} of {7 * G ** 3} queries differ, first at cell ({x}, {y}, {z}) from level {start}: "
                      f"packed flat (level, solid, nq) = {rest[:3]}, branchy = {rest[3:]}")
    assert (loads.value > 0) == bool((mat > 0).any())            # the fine words were asked for by their rank where there are any


@pytest.mark.parametrize("name", GRIDS)
def test_pack_equals_the_unpacked_expressions(name):
    l0, l1, l2, l0c, base = levels(GRIDS[name]())
    first = C.c_int(-1)
    bad = lib().cp_check_pack(ptr(l0), ptr(l1), ptr(l2), ptr(l0c), ptr(base), C.byref(first))
    assert bad == 0, f"{name}: {bad} of 512 l1 cells differ, first {first.value}"


def test_grids_are_what_they_claim():
    assert not GRIDS["empty"]().any() and GRIDS["full"]().all() and GRIDS["one_voxel"]().sum() == 1 and GRIDS["corners"]().sum() == 8
    for p in (0.001, 0.05, 0.5):
        assert abs(GRIDS[f"p{p}"]().mean() / p - 1) < 0.05
    base = levels(GRIDS["full"]())[4]
    assert base[512] == 32 ** 3 < 1 << 29                        # the largest fine base there is: below the packed level bits
    assert levels(GRIDS["p0.001"]())[4][512] > E.POOL_FINE_WORDS > levels(GRIDS["corners"]())[4][512]
