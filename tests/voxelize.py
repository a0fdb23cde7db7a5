"""Triangles for vrt_voxelize_triangles: the named triangle families, the numpy brute force that every voxelised state is compared
with, an exact geometric predicate in Python fractions, and the host build of voxel_rt2_amd/csrc/vrt_voxelize.h
(tests/emul/voxelize_emul.cpp) behind ctypes.  Test infrastructure shared by tests/test_voxelize_host.py (no GPU) and
tests/test_gpu_voxelize.py.  Every comparison is bit for bit.

Expected grids come from brute() alone: include/vrt_api.h's specification stated once in numpy -- the snap in float32, then for every
triangle and EVERY cell of the clip box the thirteen-axis test in int64 on the projections of the triangle's three vertices and the
cube's eight corners (no set-up record, no per-axis constants, no hierarchy: nothing of vrt_voxelize.h's shape), highest index wins --
and tests/edit.py's rebuild() for what vrt_prepare derives.  The predicate itself is checked against geometry, not against a second
separating-axis test: exact_covers() clips the snapped triangle as a polygon against the cube's six half-spaces in fractions.

A case is (base scene of tests/rays.py, [call, ...]); a call is (triangles, lo, hi): an array of _abi.TRIANGLE and the clip box."""
import ctypes as C
import functools
import os
import subprocess
from fractions import Fraction

import numpy as np

import edit as E
import rays as R
from voxel_rt2_amd import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_SO = os.path.join(HERE, "emul", "_voxelize_emul.so")
_SRC = os.path.join(HERE, "emul", "voxelize_emul.cpp")
_lib = None
TRI, RESULT = _abi.TRIANGLE, _abi.VOXELIZE_RESULT
F = np.float32
GCC = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unknown-pragmas"]


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(ROOT, "voxel_rt2_amd", "csrc")
        deps = [_SRC, os.path.join(HERE, "emul", "edit_emul.h"), os.path.join(ROOT, "include", "vrt_api.h")] + [os.path.join(csrc, f) for f in ("vrt_voxelize.h", "vrt_edit.h", "vrt_trace.h", "vrt_types.h", "vrt_plan.h")]
        if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
            subprocess.run(GCC + ["-fPIC", "-shared", "-o", _SO, _SRC], check=True, capture_output=True)
        _lib = C.CDLL(_SO)
        _lib.vox_emul_call.argtypes = [C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int] + [C.c_void_p] * 8
        _lib.vox_emul_covers.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int]
        _lib.vox_emul_snap.argtypes = [C.c_float, C.c_int]
        _lib.vox_emul_valid.argtypes = [C.c_void_p]
        _lib.vox_emul_setup.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _lib.vox_emul_cells.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _lib.vox_emul_plan.restype = C.c_longlong
    return _lib


build = lib
_p = lambda a: a.ctypes.data_as(C.c_void_p)


# ---- the host build ---------------------------------------------------------------------------------------------------------------
def emul_call(grid, tris, lo, hi, chunk=1 << 20, grab=4, once=False):
    """vrt_voxelize_triangles on an edit.HostGrid, in place: (return code, result record).  once: the device path's shape -- batches of
    `chunk` triangles raise owners, one resolve over the whole array follows; otherwise the host path's, a resolve a chunk."""
    tris = np.ascontiguousarray(tris, TRI)
    lo_, hi_ = np.array(lo, np.int32), np.array(hi, np.int32)
    res = np.zeros(1, RESULT)
    d = grid.derived
    rc = lib().vox_emul_call(grid.mat.shape[0], len(tris), _p(tris), _p(lo_), _p(hi_), chunk, grab, int(once), _p(grid.mat), _p(grid.rgb), _p(d["grid"]), _p(d["l0"]),
                             _p(d["l1"]), _p(d["l2"]), _p(d["l3"]), _p(res))
    return rc, res[0]


def emul_covers(G, tri, cells, shift=0):
    cells = np.ascontiguousarray(cells, np.int32)
    out = np.zeros(len(cells), np.int8)
    lib().vox_emul_covers(G, _p(np.ascontiguousarray(tri, TRI).reshape(1)), len(cells), _p(cells), _p(out), shift)
    return out


def emul_setup(G, tri):
    out = np.zeros(85, np.int64)
    assert lib().vox_emul_setup(_p(np.ascontiguousarray(tri, TRI).reshape(1)), G, _p(out)) == 85
    return out


# ---- the specification in numpy ---------------------------------------------------------------------------------------------------
def snap(w, G):
    """int64 of the same shape: (int32)rintf(((w + 1.0f) * (float)(G / 2)) * 64.0f); np.rint rounds half to even"""
    with np.errstate(invalid="ignore", over="ignore"):
        u = (np.asarray(w, F) + F(1.0)) * F(G // 2)
        assert u.dtype == F
        return np.rint(u * F(64.0)).astype(np.int64)


def vertices(tris):
    return np.stack([tris["v0"], tris["v1"], tris["v2"]], axis=1)                                                # (n, 3, 3) float32


def valid(tris):
    v = vertices(tris).reshape(len(tris), 9)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(v).all(axis=1) & (np.abs(v) <= F(_abi.TRI_MAX_COORD)).all(axis=1)
    return ok & (tris["reserved0"] == 0) & (tris["reserved1"] == 0)


_CORNERS = np.array([(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.int64)


def axes13(v):
    """the thirteen axes of a snapped triangle v (3, 3) int64: the cube's normals, e0 x e1, the nine e_i x axis_a"""
    e = np.array([v[1] - v[0], v[2] - v[1], v[0] - v[2]])
    eye = np.eye(3, dtype=np.int64)
    return np.concatenate([eye, [np.cross(e[0], e[1])], [np.cross(e[i], eye[a]) for i in range(3) for a in range(3)]])


def covers(v, cells, edge=64):
    """bool[n]: the closed triangle v (snapped, int64) and the closed cubes [edge c, edge c + edge]^3 are not strictly apart on any of
    the thirteen axes.  Projections of the three vertices and the eight corners, all in int64 (< 2^56: include/vrt_api.h)."""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    hit = np.ones(len(cells), bool)
    for n in axes13(v):
        t = v @ n                                                                                              # (3,)
        q = (cells[:, None, :] + _CORNERS[None]) * edge @ n                                                    # (n, 8)
        hit &= ~((t.max() < q.min(axis=1)) | (t.min() > q.max(axis=1)))
    return hit


def box_cells(lo, hi):
    return np.stack(np.meshgrid(*[np.arange(l, h) for l, h in zip(lo, hi)], indexing="ij"), axis=-1).reshape(-1, 3)


def brute(mat, rgb, tris, lo, hi, cells=None):
    """(mat, rgb, result) after the call.  cells: the cells looked at (by default every cell of the box)."""
    mat, rgb = mat.copy(), rgb.copy()
    G = mat.shape[0]
    res = np.zeros(1, RESULT)[0]
    if len(tris) == 0 or any(h <= l for l, h in zip(lo, hi)):
        return mat, rgb, res
    cells = box_cells(lo, hi) if cells is None else cells
    owner = np.full(len(cells), -1, np.int64)
    ok = valid(tris)
    res["invalid"] = int((~ok).sum())
    s = snap(vertices(tris), G)
    for k in np.flatnonzero(ok):
        owner[covers(s[k], cells)] = k                                                                          # later triangles paint over
    w = owner >= 0
    if w.any():
        c, p = cells[w], tris["voxel"][owner[w]]
        mat[c[:, 0], c[:, 1], c[:, 2]] = (p >> 24).astype(np.uint8).view(np.int8)
        rgb[c[:, 0], c[:, 1], c[:, 2]] = np.stack([p & 0xFF, (p >> 8) & 0xFF, (p >> 16) & 0xFF], axis=1).astype(np.uint8)
        res["lo"], res["hi"], res["voxels"] = c.min(axis=0), c.max(axis=0) + 1, int(w.sum())
    return mat, rgb, res


# ---- geometry, exactly ------------------------------------------------------------------------------------------------------------
def exact_covers(v, cell, edge=64):
    """Do the convex hull of the snapped vertices v (3 integer triples) and the closed cube of `cell` share a point?  The hull as a
    closed vertex loop (a point is a loop of one, a segment a loop there and back), clipped against the six closed half-spaces one
    after the other (Sutherland-Hodgman) in exact rationals: something is left iff they do.  Coordinates are Python integers until
    an edge is cut and fractions from there (int and Fraction mix exactly), so the many cells a first plane rejects cost little."""
    poly = [tuple(int(x) for x in p) for p in v]
    for a in range(3):
        for sign, bound in ((1, edge * int(cell[a])), (-1, -edge * (int(cell[a]) + 1))):
            d = [sign * p[a] - bound for p in poly]                                                             # >= 0: inside
            out = []
            for i in range(len(poly)):
                p, q, dp, dq = poly[i], poly[(i + 1) % len(poly)], d[i], d[(i + 1) % len(poly)]
                if dp >= 0:
                    out.append(p)
                if (dp > 0 and dq < 0) or (dp < 0 and dq > 0):
                    t = Fraction(dp) / Fraction(dp - dq)
                    out.append(tuple(pa + t * (qa - pa) for pa, qa in zip(p, q)))
            poly = out
            if not poly:
                return False
    return True


# ---- triangles ---------------------------------------------------------------------------------------------------------------------
def payload(rgb, mat):
    return np.uint32(rgb[0] | rgb[1] << 8 | rgb[2] << 16 | (int(np.int8(mat).view(np.uint8)) << 24))


def world(G, vox):
    """voxel-unit coordinates (plane k at k) -> world float32; exact for the dyadic coordinates the families use"""
    return np.asarray(vox, np.float64).astype(F) * F(2.0 / G) - F(1.0)


def triangles(G, vox, payloads=None):
    """_abi.TRIANGLE records from (n, 3, 3) voxel-unit vertices; payload k by default a colour and material 11 that depend on k"""
    vox = np.asarray(vox, np.float64).reshape(-1, 3, 3)
    t = np.zeros(len(vox), TRI)
    w = world(G, vox)
    t["v0"], t["v1"], t["v2"] = w[:, 0], w[:, 1], w[:, 2]
    if payloads is None:
        payloads = [payload((40 + 37 * k % 200, 250 - 53 * k % 200, 30 + 91 * k % 220), 11) for k in range(len(vox))]
    t["voxel"] = payloads
    return t


def icosphere(centre, radius, subdivisions=0):
    """(vertices float64 (V, 3), faces int (F, 3)): an icosahedron, each triangle split in four `subdivisions` times"""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * radius + np.asarray(centre, np.float64), np.array(f, np.int64)


def cube12(lo_idx, hi_idx):
    """the twelve triangles (voxel units) of the closed box whose corners are the index box's -- what Renderer.box_of_voxels spans"""
    (x0, y0, z0), (x1, y1, z1) = lo_idx, hi_idx
    c = lambda i: ((x0, x1)[i & 1], (y0, y1)[(i >> 1) & 1], (z0, z1)[i >> 2])
    quads = [(0, 2, 6, 4), (1, 3, 7, 5), (0, 1, 5, 4), (2, 3, 7, 6), (0, 1, 3, 2), (4, 5, 7, 6)]
    return np.array([[c(q[0]), c(q[i]), c(q[i + 1])] for q in quads for i in (1, 2)], np.float64)


GENERIC = ("points", "segments", "in_plane", "sliver", "huge", "outside", "unaligned", "stack", "stack_reversed", "negative", "invalid", "cube12")
FIXED = {"carve_last": 128, "ico_sunlit": 128, "ico_dense": 128, "ico_s1_256": 256}
POINT_CELLS = (8, 4, 2, 1)


def cases():
    return [(n, G) for n in GENERIC for G in (128, 256)] + list(FIXED.items())


def origin(G):
    return G // 2 - 16


@functools.lru_cache(maxsize=None)
def case(name, G):
    """(base scene, [(tris, lo, hi), ...]).  Generic families live in the 32^3 box at the grid's centre, o = G / 2 - 16, coordinates below
    relative to o; each is the smallest case of something that can go wrong (tests/test_gpu_voxelize.py's docstring)."""
    base = "s1_256" if G == 256 else "sunlit"
    o = origin(G)
    lo, hi = (o, o, o), (o + 32, o + 32, o + 32)
    at = lambda pts: np.asarray(pts, np.float64) + o
    if name == "points":                              # on a grid vertex (8 cells), an edge (4), a face (2), inside a cell (1)
        pts = [(8, 8, 8), (12.5, 8, 20), (20.5, 12.5, 8), (24.5, 24.25, 3.75)]
        return base, [(triangles(G, at([[p, p, p] for p in pts])), lo, hi)]
    if name == "segments":                            # along a grid line; along a body diagonal (through grid vertices)
        return base, [(triangles(G, at([[(2, 4, 4), (12, 4, 4), (12, 4, 4)], [(3, 3, 3), (14, 14, 14), (8.5, 8.5, 8.5)]])), lo, hi)]
    if name == "in_plane":                            # lies in the grid plane z = o + 10: the cells on both sides
        return base, [(triangles(G, at([[(2, 3, 10), (28, 5, 10), (9, 27, 10)]])), lo, hi)]
    if name == "sliver":                              # one sixty-fourth thin, crossing bricks diagonally
        return base, [(triangles(G, at([[(1, 1, 1.5), (29, 30.25, 28.5), (29 + 1 / 64, 30.25, 28.5)]])), lo, hi)]
    if name == "huge":                                # larger than the grid, vertices at +-8 world units
        t = np.zeros(1, TRI)
        t["v0"], t["v1"], t["v2"], t["voxel"] = (-8, -8, -8), (8, 8, 8), (8, -8, 0.25), payload((10, 200, 90), 11)
        return base, [(t, lo, hi)]
    if name == "outside":                             # wholly outside the clip box; outside the grid; touching the box's plane x = o from outside
        far = np.array([[(-20, 2, 2), (-12, 9, 3), (-15, 4, 11)], [(-200, -300, 5), (-190, -300, 9), (-195, -310, 7)]], np.float64)
        touch = [[(-6, 4, 4), (0, 9.5, 6.5), (-5, 12, 13)], [(-3, 20, 20), (0, 20, 29), (0, 27, 22)]]            # a vertex, then an edge in the plane
        return base, [(triangles(G, at(np.concatenate([far, touch]))), lo, hi)]
    if name == "unaligned":                           # tests/edit.py's box: brick, 16-cell and 64-cell boundaries inside it
        (x0, y0, z0), (x1, y1, z1) = E.UNALIGNED
        vox = [[(x0 - 2, y0 - 3, z0 + 1), (x1 + 3, y1 + 2, z1 - 1.5), (x0 + 1, y1 + 4, z0 - 2)], [(x0 + 0.5, y0 + 30, z0 - 3), (x1 - 0.25, y0 + 34.5, z1 + 3), (x0 + 1.5, y0 + 50, z0 + 2.5)]]
        return base, [(triangles(G, vox), *E.UNALIGNED)]
    if name in ("stack", "stack_reversed"):           # identical triangles, different payloads: the highest index wins
        vox = at([[(3, 4, 5.5), (27, 6, 9.25), (11, 26, 20)]] * 5)
        pay = [payload((50 * k + 5, 255 - 40 * k, 17 * k), (11, 21, 2, 54, 1)[k]) for k in range(5)]
        return base, [(triangles(G, vox, pay if name == "stack" else pay[::-1]), lo, hi)]
    if name == "negative":                            # a negative material byte: stored as it is, texel alpha 0, not occupied
        return base, [(triangles(G, at([[(4, 20, 6), (25, 22.5, 8), (14, 26, 27)]]), [payload((9, 99, 199), -5)]), lo, hi)]
    if name == "invalid":                             # NaN, inf, 8 + 1 ulp between valid triangles
        t = triangles(G, at([[(2 + 3 * k, 3, 4), (4 + 3 * k, 25, 9), (3 + 3 * k, 12, 28)] for k in range(7)]))
        t["v0"][1, 2], t["v1"][3, 0], t["v2"][5, 1] = np.nan, np.inf, np.nextafter(F(8.0), F(9.0))
        t["v2"][6, 1] = F(-8.0)                                                                                 # on the bound: valid
        return base, [(t, lo, hi)]
    if name == "cube12":                              # a closed cube whose faces lie in grid planes
        return base, [(triangles(G, cube12((o + 6, o + 9, o + 5), (o + 19, o + 25, o + 22))), lo, hi)]
    if name == "carve_last":                          # the last voxel is carved away (the grid becomes empty), then one appears elsewhere
        carve = triangles(128, [[(127.5, 64.5, 0.5)] * 3], [payload((0, 0, 0), 0)])
        add = triangles(128, [[(70.5, 66.25, 61.5)] * 3], [payload((32, 255, 64), 11)])
        return "one_voxel", [(carve, (120, 60, 0), (128, 68, 4)), (add, (64, 64, 56), (80, 72, 64))]
    if name.startswith("ico_"):                       # a 20-triangle icosphere in a 32^3 box on three scenes
        base = name[4:]
        G = R.scene(base)[0].shape[0]
        o = origin(G)
        v, f = icosphere((o + 16.3, o + 15.6, o + 16.9), 13.7)
        return base, [(triangles(G, v[f]), (o, o, o), (o + 32, o + 32, o + 32))]
    raise KeyError(name)


@functools.lru_cache(maxsize=8)
def states(name, G):
    """[(mat, rgb, result)]: the base grid (result None) and the brute force's grid and result after each call"""
    base, calls = case(name, G)
    out = [R.scene(base)[:2] + (None,)]
    for tris, lo, hi in calls:
        out.append(brute(out[-1][0], out[-1][1], tris, lo, hi))
    return out


def same_result(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("lo", "hi", "voxels", "invalid"))
