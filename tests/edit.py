"""Voxel edits (vrt_update_voxels): the numpy rebuild from scratch that every edited state is compared with, the host build of
voxel_rt2_amd/csrc/vrt_edit.h (tests/emul/edit_emul.cpp) behind ctypes, and the named edit sequences.  Test infrastructure shared by
tests/test_voxel_edit_host.py (no GPU) and tests/test_gpu_voxel_edit.py.

An edit is (lo, hi, mat, rgb): the box [lo, hi) in array indices and its new content, int8[hx,hy,hz] and uint8[hx,hy,hz,3].
A sequence is (base scene, [edit, ...]); the grid after k edits is grids(base, edits)[k]."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import rays as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_SO = os.path.join(HERE, "emul", "_edit_emul.so")
_lib = None
POOL_FINE_WORDS = 1024   # VRT_POOL_FINE_WORDS (vrt_pool.h): the non-empty fine words the pooled kernel keeps in LDS


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(HERE, "emul", "edit_emul.cpp")
        csrc = os.path.join(ROOT, "voxel_rt2_amd", "csrc")
        deps = [src, os.path.join(HERE, "emul", "edit_emul.h"), os.path.join(ROOT, "include", "vrt_api.h")] + [os.path.join(csrc, f) for f in ("vrt_voxelize.h", "vrt_edit.h", "vrt_trace.h", "vrt_types.h")]
        if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unknown-pragmas",
                            "-o", _SO, src], check=True, capture_output=True)
        _lib = C.CDLL(_SO)
        _lib.edit_apply.argtypes = [C.c_int] + [C.c_void_p] * 11
        _lib.edit_touched.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    return _lib


# ---- the expectation: everything vrt_prepare derives from the voxels, from scratch, in numpy --------------------------------
def _brick_words(cells):
    """bool[X][Y][Z] -> u64[Z/4][Y/4][X/4]: bit z*16 + y*4 + x of word (bz, by, bx) = cell (4bx+x, 4by+y, 4bz+z)."""
    n = cells.shape[0] // 4
    bits = cells.reshape(n, 4, n, 4, n, 4).transpose(4, 2, 0, 5, 3, 1).reshape(n, n, n, 64)
    return np.ascontiguousarray(np.packbits(bits, axis=-1, bitorder="little")).view("<u8").reshape(n, n, n)


def rebuild(mat, rgb):
    """dict(grid, l0, l1, l2, l3): the packed texels in texel_index<G>'s order and the levels' words as flat arrays (k_pack_grid,
    k_build_l0, k_build_coarse).  l3 is one word; at 128 nothing reads it and it stays 0."""
    G = mat.shape[0]
    tex = (rgb[..., 0].astype(np.uint32) | rgb[..., 1].astype(np.uint32) << 8 | rgb[..., 2].astype(np.uint32) << 16 |
           np.maximum(mat, 0).astype(np.uint32) << 24)
    if G == 256:   # brick-tiled: the 64 texels of a 4x4x4 brick together, bricks in l0 word order
        tex = tex.reshape(64, 4, 64, 4, 64, 4).transpose(4, 2, 0, 5, 3, 1)
    out = dict(grid=np.ascontiguousarray(tex).reshape(-1))
    level = _brick_words(mat > 0)
    for name in ("l0", "l1", "l2"):
        out[name] = level.reshape(-1)
        level = _brick_words((level != 0).transpose(2, 1, 0)) if level.shape[0] >= 4 else None
    out["l3"] = level.reshape(-1) if G == 256 else np.zeros(1, "<u8")
    return out


class HostGrid:
    """Host copies of mat, rgb, the texels and l0..l3 that edit_emul.cpp edits in place."""

    def __init__(self, mat, rgb):
        self.mat, self.rgb = np.array(mat, np.int8), np.array(rgb, np.uint8)
        self.derived = {k: v.copy() for k, v in rebuild(self.mat, self.rgb).items()}

    def apply(self, lo, hi, bmat, brgb):
        bmat, brgb = np.ascontiguousarray(bmat, np.int8), np.ascontiguousarray(brgb, np.uint8)
        lo_, hi_ = np.array(lo, np.int32), np.array(hi, np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        d = self.derived
        return lib().edit_apply(self.mat.shape[0], p(lo_), p(hi_), p(bmat), p(brgb), p(self.mat), p(self.rgb), p(d["grid"]), p(d["l0"]), p(d["l1"]),
                                p(d["l2"]), p(d["l3"]))


def touched(lo, hi, shift):
    lo_, hi_ = np.array(lo, np.int32), np.array(hi, np.int32)
    return lib().edit_touched(lo_.ctypes.data_as(C.c_void_p), hi_.ctypes.data_as(C.c_void_p), shift)


def apply_numpy(mat, rgb, e, copy=True):
    lo, hi, bmat, brgb = e
    if copy:
        mat, rgb = mat.copy(), rgb.copy()
    mat[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = bmat
    rgb[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = brgb
    return mat, rgb


def grids(name):
    """[(mat, rgb)]: the base grid of sequence `name` and the grid after each of its edits."""
    base, edits = sequence(name)
    out = [R.scene(base)[:2]]
    for e in edits:
        out.append(apply_numpy(*out[-1], e))
    return out


# ---- the edit sequences -------------------------------------------------------------------------------------------------
def _fill(lo, hi, m, c):
    shape = tuple(h - l for l, h in zip(lo, hi))
    return tuple(lo), tuple(hi), np.full(shape, m, np.int8), np.broadcast_to(np.array(c, np.uint8), shape + (3,)).copy()


def _cut(mat, rgb, lo, hi):
    """the box's content in another grid: an edit that makes the box look like that grid"""
    s = tuple(slice(l, h) for l, h in zip(lo, hi))
    return tuple(lo), tuple(hi), mat[s].copy(), rgb[s].copy()


def _pattern(lo, hi, seed, m=11):
    """a box half filled, half cleared, voxel by voxel"""
    lo, hi, mat, rgb = _fill(lo, hi, 0, (0, 0, 0))
    rng = np.random.default_rng(seed)
    on = rng.random(mat.shape) < 0.5
    mat[on] = m
    rgb[on] = rng.integers(1, 256, (int(on.sum()), 3))
    return lo, hi, mat, rgb


def _one_per_brick(lo, hi, m=1, c=(200, 180, 90)):
    """one voxel in every 4x4x4 brick of a brick-aligned box"""
    lo, hi, mat, rgb = _fill(lo, hi, 0, (0, 0, 0))
    mat[1::4, 2::4, 3::4] = m
    rgb[1::4, 2::4, 3::4] = c
    return lo, hi, mat, rgb


SEQUENCES = ("lone_voxel", "last_voxel", "unaligned", "corners", "colour_material", "negative", "dense_flip", "lds_head",
             "lone_voxel_256", "unaligned_256", "corners_256", "corners_dense")
UNALIGNED = ((3, 5, 62), (6, 70, 67))   # crosses a brick boundary on x, 16- and 64-cell boundaries on y, a 64-cell boundary on z


@functools.lru_cache(maxsize=None)
def sequence(name):
    """(base scene of tests/rays.py, edits).  What each is the smallest case of: the docstring of tests/test_gpu_voxel_edit.py."""
    if name in ("lone_voxel", "lone_voxel_256"):      # empty space far from the scene, in an l1 cell before every occupied one
        G = 256 if name.endswith("256") else 128
        return ("s1_256" if G == 256 else "sunlit"), [_fill((5, G - 8, 9), (6, G - 7, 10), 11, (255, 64, 32))]
    if name == "last_voxel":                          # the grid becomes empty, then a voxel appears somewhere else
        return "one_voxel", [_fill((127, 64, 0), (128, 65, 1), 0, (0, 0, 0)), _fill((70, 66, 61), (71, 67, 62), 11, (32, 255, 64))]
    if name in ("unaligned", "unaligned_256"):        # filled, then half of it cleared again
        return ("s1_256" if name.endswith("256") else "sunlit"), [_fill(*UNALIGNED, 21, (90, 200, 250)), _pattern(*UNALIGNED, seed=3)]
    if name in ("corners", "corners_256", "corners_dense"):
        base = {"corners": "sunlit", "corners_256": "s1_256", "corners_dense": "dense"}[name]
        mat, rgb, _ = R.scene(base)
        G = mat.shape[0]
        other = (np.roll(mat, 8, axis=0), np.roll(rgb, 8, axis=0)) if G == 256 or base == "dense" else R.scene("s1")[:2]
        return base, [_pattern((0, 0, 0), (5, 6, 7), seed=4), _pattern((G - 7, G - 6, G - 5), (G, G, G), seed=5), _cut(*other, (0, 0, 0), (G, G, G))]
    if name == "colour_material":                     # colours only (the pyramid does not change), then material 2 -> 1 on solid voxels
        mat, rgb, _ = R.scene("sunlit")
        lo, hi = (30, 50, 40), (100, 70, 90)
        _, _, m, c = _cut(mat, rgb, lo, hi)
        c1 = np.where((m > 0)[..., None], 255 - c, c).astype(np.uint8)
        assert (m == 2).any()
        return "sunlit", [(lo, hi, m, c1), (lo, hi, np.where(m == 2, 1, m).astype(np.int8), c1)]
    if name == "negative":                            # coloured voxels with negative material bytes, on top of and beside a block
        lo, hi, m, c = _pattern((60, 56, 60), (70, 66, 70), seed=6, m=-5)
        m[::3] = -128
        return "sunlit", [(lo, hi, m, c)]
    if name == "dense_flip":                          # a voxel in 17 of every 32 bricks, under sunlit's emitting sun; then as before
        mat, rgb, _ = R.scene("sunlit")
        lo, hi = (0, 0, 0), (128, 128, 68)
        return "sunlit", [_one_per_brick(lo, hi), _cut(mat, rgb, lo, hi)]
    if name == "lds_head":                            # 1152 bricks of empty space above the scene get a voxel; then as before
        mat, rgb, _ = R.scene("sunlit")
        lo, hi = (40, 72, 40), (88, 120, 72)
        return "sunlit", [_one_per_brick(lo, hi, m=21), _cut(mat, rgb, lo, hi)]
    raise KeyError(name)
