"""The arithmetic of vrt_update_voxels on the host: voxel_rt2_amd/csrc/vrt_edit.h compiled with g++ (tests/emul/edit_emul.cpp runs the
loops of the k_edit_* kernels) applies sequences of box edits to host copies of the materials, colours, packed texels and l0..l3; after
EVERY edit each array must equal, word for word, a numpy rebuild from scratch of the grid as it then stands (tests/edit.py).  Plus the
boundary: the entry point is exported and bound, and answers a NULL context without a GPU."""
import ctypes as C

import numpy as np
import pytest

import edit as E
import rays as R
from voxel_rt2_amd import _abi, _lib


def check(host, mat, rgb, label):
    assert host.mat.tobytes() == mat.tobytes() and host.rgb.tobytes() == rgb.tobytes(), f"{label}: stored voxels"
    want = E.rebuild(mat, rgb)
    for k in ("grid", "l0", "l1", "l2", "l3"):
        bad = np.flatnonzero(host.derived[k] != want[k])
        assert bad.size == 0, f"{label}: {bad.size} words of {k} differ, first at {bad[0]}: {host.derived[k][bad[0]]:#x} != {want[k][bad[0]]:#x}"


@pytest.mark.parametrize("name", E.SEQUENCES)
def test_named_sequences_equal_rebuild(name):
    base, edits = E.sequence(name)
    states = E.grids(name)
    host = E.HostGrid(*states[0])
    check(host, *states[0], f"{name}: base")
    for k, e in enumerate(edits):
        assert host.apply(*e) == 0
        check(host, *states[k + 1], f"{name}: edit {k}")


def test_sequences_are_what_they_claim():
    """The numpy side alone, so that no comparison passes on nothing."""
    bricks = lambda m: int((E.rebuild(m, np.zeros(m.shape + (3,), np.uint8))["l0"] != 0).sum())
    a, b, c = [m for m, _ in E.grids("lds_head")]
    assert bricks(a) < E.POOL_FINE_WORDS < bricks(b) and bricks(c) == bricks(a)
    a, b, c = [m for m, _ in E.grids("dense_flip")]
    assert 2 * bricks(a) < 32 ** 3 <= 2 * bricks(b) and bricks(c) == bricks(a)
    a, b, c = [m for m, _ in E.grids("last_voxel")]
    assert (a > 0).sum() == 1 and not (b > 0).any() and (c > 0).sum() == 1
    assert (R.grown_box(b)[0] > R.grown_box(b)[1]).all()                                     # the culling box of an empty grid: lo > hi
    for name in ("lone_voxel", "lone_voxel_256"):
        a, b = [m for m, _ in E.grids(name)]
        assert (b > 0).sum() == (a > 0).sum() + 1 and (R.grown_box(b)[1] > R.grown_box(a)[1]).any()   # the box grows
        wa, wb = (E.rebuild(m, np.zeros(m.shape + (3,), np.uint8)) for m in (a, b))
        first_new = np.flatnonzero(wb["l1"] != wa["l1"])
        assert first_new.size == 1 and first_new[0] < np.flatnonzero(wa["l1"])[0]           # a new l1 bit ahead of every other: l0c shifts
    (lo, hi) = E.UNALIGNED
    assert [E.touched(lo, hi, s) for s in (2, 4, 6)] == [2 * 17 * 2, 1 * 5 * 2, 1 * 2 * 2]
    states = E.grids("colour_material")
    assert all(np.array_equal(states[0][0] > 0, m > 0) for m, _ in states) and not np.array_equal(states[0][1], states[1][1])
    assert (E.grids("negative")[1][0] < 0).sum() > 100
    for name in ("corners", "corners_256", "corners_dense"):
        G = E.grids(name)[0][0].shape[0]
        (lo0, hi0, *_), (lo1, hi1, *_), (lo2, hi2, *_) = E.sequence(name)[1]
        assert lo0 == (0, 0, 0) and hi1 == (G, G, G) and (lo2, hi2) == ((0, 0, 0), (G, G, G))


def random_box(rng, G):
    """Mostly small boxes anywhere, aligned to nothing; some thin, some large, some touching the faces, one in sixteen empty."""
    kind = rng.integers(0, 16)
    size = rng.integers(1, [6, 6, 6, 6, 6, 6, 6, 6, 20, 20, 20, 20, 70, 70, G, G][kind] + 1, 3)
    if kind == 0:
        size[rng.integers(0, 3)] = 0
    if kind % 4 == 3:
        size[rng.integers(0, 3)] = 1
    lo = np.array([rng.integers(0, G - s + 1) for s in size])
    face = rng.random(3) < 0.15
    lo = np.where(face, np.where(rng.random(3) < 0.5, 0, G - size), lo)
    return tuple(int(v) for v in lo), tuple(int(v) for v in lo + size)


def random_edit(rng, G):
    lo, hi = random_box(rng, G)
    shape = tuple(h - l for l, h in zip(lo, hi))
    fill = rng.choice([0.0, 0.03, 0.5, 1.0])                       # clears, sparse, half, solid
    mat = np.where(rng.random(shape) < fill, rng.integers(1, 128, shape), rng.choice([0, 0, 0, -1, -128])).astype(np.int8)
    rgb = rng.integers(0, 256, shape + (3,)).astype(np.uint8)
    return lo, hi, mat, rgb


@pytest.mark.parametrize("G,base,n,seed", [(128, "sunlit", 200, 1), (128, "empty", 60, 2), (256, "s1_256", 24, 3)])
def test_random_boxes_equal_rebuild(G, base, n, seed):
    rng = np.random.default_rng([20250611, seed])
    mat, rgb = R.scene(base)[:2]
    host = E.HostGrid(mat, rgb)
    for k in range(n):
        e = random_edit(rng, G)
        assert host.apply(*e) == 0
        mat, rgb = E.apply_numpy(mat, rgb, e, copy=k == 0)
        check(host, mat, rgb, f"{base}: random edit {k}, box {e[0]}..{e[1]}")


def test_boxes_outside_the_grid_are_refused():
    host = E.HostGrid(*R.scene("empty")[:2])
    one = (np.zeros((1, 1, 1), np.int8), np.zeros((1, 1, 1, 3), np.uint8))
    for lo, hi in (((-1, 0, 0), (0, 1, 1)), ((0, 0, 128), (1, 1, 129)), ((5, 5, 5), (6, 4, 6)), ((0, 129, 0), (1, 130, 1))):
        assert host.apply(lo, hi, *one) == -1, (lo, hi)
    assert host.apply((128, 128, 128), (128, 128, 128), *one) == 0      # empty, at the far corner: fine


def test_update_voxels_is_exported_and_bound():
    """include/vrt_api.h declares it, the library exports it, _abi gives it its prototype, and a NULL context is VRT_E_INVALID."""
    assert "vrt_update_voxels" in _lib.exported_symbols()
    lib = _lib.load()
    fn = lib.vrt_update_voxels
    assert fn.restype is C.c_int and len(fn.argtypes) == 6
    lo, hi = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(1, 1, 1)
    mat, rgb = np.zeros((1, 1, 1), np.int8), np.zeros((1, 1, 1, 3), np.uint8)
    assert fn(None, lo, hi, mat.ctypes.data_as(C.c_void_p), rgb.ctypes.data_as(C.c_void_p), 0) == _abi.VRT_E_INVALID
    assert b"null" in lib.vrt_last_error()
