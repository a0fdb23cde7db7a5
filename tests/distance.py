"""Distance fields (vrt_distance_field): the named case families, two numpy brute forces that every result is compared with, and the
host build of voxel_rt2_amd/csrc/vrt_distance.h (tests/emul/distance_emul.cpp) behind ctypes.  Test infrastructure shared by
tests/test_distance_host.py (no GPU) and tests/test_gpu_distance.py.  Every comparison is byte for byte, over every cell of the box.

Expected values come from the brute forces alone.  Neither knows anything of a separable transform: include/vrt_api.h's definition
stated twice in numpy, each minimising the key (d2 << 24 | linear index of the target) -- the smallest distance, among equal distances
the smallest index --
  brute_targets   every cell of the box against every target of the grid: for sparse target sets;
  brute_offsets   every offset of squared length <= max_d2 against the whole box at once, the targets' indices shifted by it (cells
                  outside the grid hold no target): for dense grids and small max_d2.
reference() takes whichever is affordable; test_distance_host.py asserts once that they agree where both are.

A case is dict(grid, lo, hi, max_d2, to_empty); grid(name) is its materials."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import edit as E
import rays as R
from voxel_rt2_amd import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_SO = os.path.join(HERE, "emul", "_distance_emul.so")
_SRC = os.path.join(HERE, "emul", "distance_emul.cpp")
GCC = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unknown-pragmas"]
_lib = None
FAR, MAX_D2, TO_EMPTY = _abi.DIST_FAR, _abi.DIST_MAX_D2, _abi.DIST_TO_EMPTY
GUARD = 4096


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(ROOT, "voxel_rt2_amd", "csrc")
        deps = [_SRC, os.path.join(ROOT, "include", "vrt_api.h")] + [os.path.join(csrc, f) for f in ("vrt_distance.h", "vrt_edit.h", "vrt_trace.h", "vrt_types.h", "vrt_plan.h")]
        if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
            subprocess.run(GCC + ["-fPIC", "-shared", "-o", _SO, _SRC], check=True, capture_output=True)
        _lib = C.CDLL(_SO)
        _lib.distance_emul_plan.restype = C.c_longlong
        _lib.distance_emul_plan.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_uint, C.c_int]
        _lib.distance_emul_grown.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _lib.distance_emul_call.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint] + [C.c_void_p] * 3
    return _lib


build = lib
_p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- the host build ---------------------------------------------------------------------------------------------------------------
def emul_plan(G, lo, hi, max_d2, flags=0, nearest=True):
    return lib().distance_emul_plan(G, _p(np.array(lo, np.int32)), _p(np.array(hi, np.int32)), int(max_d2), flags, int(nearest))


def emul_grown(G, lo, hi, max_d2):
    out = np.zeros(6, np.int32)
    lib().distance_emul_grown(G, _p(np.array(lo, np.int32)), _p(np.array(hi, np.int32)), int(max_d2), _p(out))
    return out[:3].tolist(), out[3:].tolist()


def emul_call(mat, lo, hi, max_d2, to_empty=False, nearest=True, flags=None):
    """vrt_distance_field on host arrays: (return code, d2, nearest or None).  The scratch is plan_distance_layout's byte count followed
    by a guard that must come back untouched: the plan bounds what the passes write."""
    mat = np.ascontiguousarray(mat, np.int8)
    G = mat.shape[0]
    flags = (TO_EMPTY if to_empty else 0) if flags is None else flags
    shape = tuple(max(h - l, 0) for l, h in zip(lo, hi))
    d2 = np.full(shape, 0x5A5A5A5A, np.int32)
    near = np.full(shape, 0x5A5A5A5A, np.int32) if nearest else None
    need = max(int(emul_plan(G, lo, hi, max_d2, flags & TO_EMPTY, nearest)), 0)
    scratch = np.full(need + GUARD, 0xA5, np.uint8)
    rc = lib().distance_emul_call(G, _p(mat), _p(np.array(lo, np.int32)), _p(np.array(hi, np.int32)), int(max_d2), flags, _p(d2), _p(near), _p(scratch))
    assert (scratch[need:] == 0xA5).all(), "the passes wrote past plan_distance_layout's byte count"
    return rc, d2, near


# ---- the two references -------------------------------------------------------------------------------------------------------------
_BIG = np.int64(1) << 62


def _unkey(key, max_d2):
    d2 = key >> 24
    ok = d2 <= max_d2
    return np.where(ok, d2, FAR).astype(np.int32), np.where(ok, key & 0xFFFFFF, -1).astype(np.int32)


def brute_targets(mat, lo, hi, max_d2, to_empty=False, stride=1):
    """(d2, nearest): every cell of the box against every target of the grid.  stride > 1: of the cells lo, lo + stride, ... only (what
    box[::stride, ::stride, ::stride] holds)."""
    G = mat.shape[0]
    axes = [np.arange(l, h, stride, dtype=np.int64) for l, h in zip(lo, hi)]
    shape = tuple(len(a) for a in axes)
    t = np.argwhere((mat > 0) != bool(to_empty)).astype(np.int64)
    cells = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    key = np.full(len(cells), _BIG, np.int64)
    if len(t):
        idx = (t[:, 0] * G + t[:, 1]) * G + t[:, 2]
        step = max(1, (1 << 21) // len(t))
        for at in range(0, len(cells), step):
            c = cells[at:at + step]
            d = ((c[:, None, :] - t[None, :, :]) ** 2).sum(-1)
            key[at:at + step] = ((d << 24) | idx[None, :]).min(1)
    d2, near = _unkey(key, max_d2)
    return d2.reshape(shape), near.reshape(shape)


def offsets_within(max_d2):
    r = int(np.floor(np.sqrt(max_d2)))
    while (r + 1) ** 2 <= max_d2:
        r += 1
    o = np.stack(np.meshgrid(*[np.arange(-r, r + 1)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return o[(o ** 2).sum(1) <= max_d2], r


def brute_offsets(mat, lo, hi, max_d2, to_empty=False):
    """(d2, nearest): every offset with squared length <= max_d2 against the whole box at once."""
    G = mat.shape[0]
    shape = tuple(h - l for l, h in zip(lo, hi))
    offs, r = offsets_within(max_d2)
    gl, gh = [l - r for l in lo], [h + r for h in hi]     # the box grown by r: cells outside the grid hold no target
    cl, ch = [max(v, 0) for v in gl], [min(v, G) for v in gh]
    ax = [np.arange(a, b, dtype=np.int64) for a, b in zip(cl, ch)]
    idx = (ax[0][:, None, None] * G + ax[1][None, :, None]) * G + ax[2][None, None, :]
    held = np.full(tuple(b - a for a, b in zip(gl, gh)), _BIG, np.int64)     # the target's own index where a cell is a target
    inside = tuple(slice(a - g, b - g) for a, b, g in zip(cl, ch, gl))
    held[inside] = np.where((mat[cl[0]:ch[0], cl[1]:ch[1], cl[2]:ch[2]] > 0) != bool(to_empty), idx, _BIG)
    key = np.full(shape, _BIG, np.int64)
    for o in offs:
        sl = tuple(slice(r + int(d), r + int(d) + h - l) for l, h, d in zip(lo, hi, o))
        np.minimum(key, held[sl] + (np.int64(int((o ** 2).sum())) << 24), out=key)
    return _unkey(np.minimum(key, _BIG), max_d2)


def affordable(mat, lo, hi, max_d2, to_empty):
    """(brute_targets is, brute_offsets is)"""
    cells = int(np.prod([h - l for l, h in zip(lo, hi)]))
    targets = int(((mat > 0) != bool(to_empty)).sum())
    return cells * max(targets, 1) <= 3e8, cells * len(offsets_within(min(max_d2, 4000))[0]) <= 1e9 and max_d2 <= 4000


def reference(mat, lo, hi, max_d2, to_empty=False):
    by_targets, by_offsets = affordable(mat, lo, hi, max_d2, to_empty)
    assert by_targets or by_offsets, "neither brute force is affordable for this case: choose a smaller one"
    return (brute_targets if by_targets else brute_offsets)(mat, lo, hi, max_d2, to_empty)


# ---- grids and cases -------------------------------------------------------------------------------------------------------------------
C0 = (64, 64, 64)
TIE_K = 7
TWELVE = [(5, 0, 0), (0, 5, 0), (0, 0, 5), (3, 4, 0), (0, 3, 4), (4, 0, 3)]
LONE = (60, 61, 62)
S1_EDIT = E._pattern((60, 58, 66), (72, 70, 80), seed=9)


def _solids(G, cells):
    mat = np.zeros((G, G, G), np.int8)
    for c in cells:
        mat[tuple(c)] = 11
    return mat


@functools.lru_cache(maxsize=None)
def grid(name):
    """int8[G][G][G]: the materials of a named grid (colours: colours())"""
    if name in ("s1", "dense", "s1_256", "sponge256", "sunlit"):
        return R.scene(name)[0]
    if name in ("empty", "empty_256"):
        return _solids(256 if name.endswith("256") else 128, [])
    if name == "full":
        return np.full((128, 128, 128), 3, np.int8)
    if name in ("corners", "corners_256"):
        G = 256 if name.endswith("256") else 128
        return _solids(G, [(x, y, z) for x in (0, G - 1) for y in (0, G - 1) for z in (0, G - 1)] + [(G // 2,) * 3])
    if name in ("tie_x", "tie_y", "tie_z"):
        a = "xyz".index(name[-1])
        return _solids(128, [tuple(C0[k] + (s * TIE_K if k == a else 0) for k in range(3)) for s in (-1, 1)])
    if name == "twelve":
        return _solids(128, [tuple(C0[k] + s * o[k] for k in range(3)) for o in TWELVE for s in (-1, 1)])
    if name == "lone":
        mat = _solids(128, [LONE])
        mat[LONE[0] + 9, LONE[1], LONE[2]] = -7          # a negative material byte is not solid
        return mat
    if name == "s1_edit":
        return E.apply_numpy(*R.scene("s1")[:2], S1_EDIT)[0]
    raise KeyError(name)


def colours(name):
    if name in ("s1", "dense", "s1_256", "sponge256", "sunlit"):
        return R.scene(name)[1]
    if name == "s1_edit":
        return E.apply_numpy(*R.scene("s1")[:2], S1_EDIT)[1]
    m = grid(name)
    x, y, z = np.meshgrid(*[np.arange(m.shape[0])] * 3, indexing="ij")
    return np.where((m != 0)[..., None], np.stack([x * 2 + 1, y + 100, 255 - z], -1) % 256, 0).astype(np.uint8)


def params(name):
    return R.scene(name)[2] if name in ("s1", "dense", "s1_256", "sponge256", "sunlit") else R.scene("s1")[2] if name == "s1_edit" else R.FLOOR


def _case(grid, lo, hi, max_d2=MAX_D2, to_empty=False):
    return dict(grid=grid, lo=tuple(lo), hi=tuple(hi), max_d2=int(max_d2), to_empty=bool(to_empty))


def _around(c, r):
    return tuple(v - r for v in c), tuple(v + r + 1 for v in c)


CASES = {
    # nothing to find; everything a target
    "empty": _case("empty", (40, 50, 60), (70, 80, 90), max_d2=900),
    "full_to_empty": _case("full", (0, 0, 100), (30, 30, 128), max_d2=2000, to_empty=True),
    "full": _case("full", (90, 0, 0), (128, 30, 30), max_d2=50),
    "empty_to_empty": _case("empty", (0, 0, 0), (20, 20, 20), max_d2=50, to_empty=True),
    # a single solid in each grid corner and at the centre; the first unbounded, so that the grown box is the grid
    "corners_lo": _case("corners", (0, 0, 0), (30, 30, 30)),
    "corners_hi": _case("corners", (98, 98, 98), (128, 128, 128), max_d2=3 * 29 * 29),
    "corners_mid": _case("corners", (44, 50, 49), (84, 80, 79), max_d2=3 * 20 * 20),
    # two solids at -k and +k on one axis; twelve at d2 = 25 across the axes
    "tie_x": _case("tie_x", *_around(C0, 10), max_d2=400),
    "tie_y": _case("tie_y", *_around(C0, 10), max_d2=400),
    "tie_z": _case("tie_z", *_around(C0, 10), max_d2=400),
    "twelve": _case("twelve", *_around(C0, 10), max_d2=300),
    "twelve_25": _case("twelve", *_around(C0, 8), max_d2=25),
    "twelve_24": _case("twelve", *_around(C0, 8), max_d2=24),
    # max_d2: 0; exactly D of the box's cell (3, 4, 0) away from the lone solid, which is kept; D - 1, which is FAR
    "maxd2_0": _case("s1", (60, 60, 60), (90, 84, 90), max_d2=0),
    "maxd2_exact": _case("lone", (LONE[0] + 3, LONE[1] + 4, LONE[2]), (LONE[0] + 12, LONE[1] + 9, LONE[2] + 3), max_d2=25),
    "maxd2_minus": _case("lone", (LONE[0] + 3, LONE[1] + 4, LONE[2]), (LONE[0] + 12, LONE[1] + 9, LONE[2] + 3), max_d2=24),
    "s1_unbounded": _case("s1", (50, 60, 50), (74, 84, 74), max_d2=MAX_D2),
    # the only target outside the box: inside the grown box (R = 4 reaches it), and just outside it (R = 3 does not)
    "outside_in": _case("lone", (LONE[0] + 4, LONE[1] - 4, LONE[2] - 4), (LONE[0] + 10, LONE[1] + 4, LONE[2] + 4), max_d2=16),
    "outside_out": _case("lone", (LONE[0] + 4, LONE[1] - 4, LONE[2] - 4), (LONE[0] + 10, LONE[1] + 4, LONE[2] + 4), max_d2=15),
    # a box on each grid face: the grown box is cut on that side only
    "face_x0": _case("dense", (0, 50, 50), (6, 61, 63), max_d2=9),
    "face_x1": _case("dense", (122, 50, 50), (128, 61, 63), max_d2=9),
    "face_y0": _case("dense", (50, 0, 50), (61, 6, 63), max_d2=9),
    "face_y1": _case("dense", (50, 122, 50), (61, 128, 63), max_d2=9),
    "face_z0": _case("dense", (50, 50, 0), (61, 63, 6), max_d2=9, to_empty=True),
    "face_z1": _case("dense", (50, 50, 122), (61, 63, 128), max_d2=9, to_empty=True),
    # shapes: a cell (a line of length 1 in every pass with max_d2 = 0), lines along z and x, edges that are no multiple of any tile
    "cell": _case("s1", (70, 70, 70), (71, 71, 71), max_d2=100),
    "cell_d0": _case("s1", (64, 64, 64), (65, 65, 65), max_d2=0),
    "line_z": _case("s1", (80, 70, 0), (81, 71, 128), max_d2=100),
    "line_x": _case("s1", (0, 70, 80), (128, 71, 81), max_d2=100),
    "odd_box": _case("s1", (62, 40, 60), (67, 107, 93), max_d2=100),
    # half the cells solid
    "dense_9": _case("dense", (30, 40, 50), (70, 80, 90), max_d2=9),
    "dense_9_to_empty": _case("dense", (30, 40, 50), (70, 80, 90), max_d2=9, to_empty=True),
    # after an edit
    "s1_edit": _case("s1_edit", (56, 54, 62), (80, 78, 84), max_d2=64),
    # the other grid
    "corners_256": _case("corners_256", (226, 0, 226), (256, 30, 256), max_d2=3 * 29 * 29),
    "s1_256": _case("s1_256", (122, 121, 120), (138, 137, 136), max_d2=400),
    "sponge256_9": _case("sponge256", (0, 100, 216), (33, 140, 256), max_d2=9),
}
HOST_256 = ("corners_256",)
GPU_256 = ("corners_256", "s1_256", "sponge256_9")
NAMES_128 = tuple(n for n in CASES if n not in GPU_256)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(d2, nearest) of a case, from a brute force; computed once, shared, never written to"""
    c = CASES[name]
    d2, near = reference(grid(c["grid"]), c["lo"], c["hi"], c["max_d2"], c["to_empty"])
    d2.setflags(write=False)
    near.setflags(write=False)
    return d2, near


def check(got_d2, got_near, want, label):
    """byte for byte, every cell of the box"""
    d2, near = want
    assert got_d2.dtype == np.int32 and got_d2.shape == d2.shape, (label, got_d2.dtype, got_d2.shape, d2.shape)
    bad = np.argwhere(got_d2 != d2)
    assert len(bad) == 0, f"{label}: d2 differs in {len(bad)} of {d2.size} cells, first at box cell {bad[0].tolist()}: {got_d2[tuple(bad[0])]} != {d2[tuple(bad[0])]}"
    if got_near is not None:
        assert got_near.dtype == np.int32 and got_near.shape == near.shape, label
        bad = np.argwhere(got_near != near)
        assert len(bad) == 0, (f"{label}: nearest differs in {len(bad)} of {near.size} cells, first at box cell {bad[0].tolist()}: "
                               f"{got_near[tuple(bad[0])]} != {near[tuple(bad[0])]} (d2 {d2[tuple(bad[0])]})")
