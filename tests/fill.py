"""Meshes for vrt_fill_triangles: the named mesh families, the numpy brute force that every filled state is compared with, the exact
geometric predicate in Python fractions, and the host build of voxel_rt2_amd/csrc/vrt_fill.h (tests/emul/fill_emul.cpp) behind ctypes.
Test infrastructure shared by tests/test_fill_host.py (no GPU) and tests/test_gpu_fill.py.  Every comparison is bit for bit.

Expected grids come from brute() alone: include/vrt_api.h's INSIDE stated once in numpy -- tests/voxelize.py's snap in float32, then for
every valid triangle and every cell of the clip box the cascade in int64 straight from the header's text (the three edge functions with
their tie signs, the plane function with its own; no set-up record, no first cell, no toggle bitmap, no prefix: nothing of vrt_fill.h's
shape), the parity over the triangles -- and tests/edit.py's rebuild() for what vrt_prepare derives.  The cascade itself is checked
against geometry, not against a second cascade: exact_crossing() evaluates plain strict tests in fractions at q + (eps, eps^2, eps^3).

A case is (base scene of tests/rays.py, [call, ...]); a call is (triangles, lo, hi, voxel)."""
import ctypes as C
import functools
import os
import subprocess
from fractions import Fraction

import numpy as np

import rays as R
import voxelize as V
from voxel_rt2_amd import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_SO = os.path.join(HERE, "emul", "_fill_emul.so")
_SRC = os.path.join(HERE, "emul", "fill_emul.cpp")
_lib = None
TRI, RESULT = _abi.TRIANGLE, _abi.VOXELIZE_RESULT
SETUP_WORDS = 36


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(ROOT, "voxel_rt2_amd", "csrc")
        deps = [_SRC, os.path.join(HERE, "emul", "edit_emul.h"), os.path.join(ROOT, "include", "vrt_api.h")] + [os.path.join(csrc, f) for f in ("vrt_fill.h", "vrt_voxelize.h", "vrt_edit.h", "vrt_trace.h", "vrt_types.h", "vrt_plan.h")]
        if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
            subprocess.run(V.GCC + ["-fPIC", "-shared", "-o", _SO, _SRC], check=True, capture_output=True)
        _lib = C.CDLL(_SO)
        _lib.fill_emul_call.argtypes = [C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_longlong, C.c_int] + [C.c_void_p] * 8
        _lib.fill_emul_columns.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.fill_emul_setup.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _lib.fill_emul_cells.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.fill_emul_prefix.argtypes = [C.c_longlong, C.c_void_p]
        _lib.fill_emul_plan.restype = C.c_longlong
    return _lib


build = lib
_p = lambda a: a.ctypes.data_as(C.c_void_p)


# ---- the host build ---------------------------------------------------------------------------------------------------------------
def emul_call(grid, tris, lo, hi, voxel, chunk=1 << 20, grab=8):
    """vrt_fill_triangles on an edit.HostGrid, in place: (return code, result record); batches of `chunk` triangles toggle, one resolve"""
    tris = np.ascontiguousarray(tris, TRI)
    lo_, hi_ = np.array(lo, np.int32), np.array(hi, np.int32)
    res = np.zeros(1, RESULT)
    d = grid.derived
    rc = lib().fill_emul_call(grid.mat.shape[0], len(tris), _p(tris), _p(lo_), _p(hi_), int(voxel), chunk, grab, _p(grid.mat), _p(grid.rgb), _p(d["grid"]), _p(d["l0"]),
                              _p(d["l1"]), _p(d["l2"]), _p(d["l3"]), _p(res))
    return rc, res[0]


def emul_columns(G, tri, cols):
    """(in int8[n], first int64[n]) of fill_column_in / fill_first_cell for columns (n, 2)"""
    cols = np.ascontiguousarray(cols, np.int32)
    inn, first = np.zeros(len(cols), np.int8), np.zeros(len(cols), np.int64)
    lib().fill_emul_columns(G, _p(np.ascontiguousarray(tri, TRI).reshape(1)), len(cols), _p(cols), _p(inn), _p(first))
    return inn, first


def emul_setup(G, tri):
    out = np.zeros(SETUP_WORDS, np.int64)
    assert lib().fill_emul_setup(_p(np.ascontiguousarray(tri, TRI).reshape(1)), G, _p(out)) == SETUP_WORDS
    return out


def emul_cells(G, tri, lo, hi):
    out = np.zeros(9, np.int32)
    lib().fill_emul_cells(_p(np.ascontiguousarray(tri, TRI).reshape(1)), G, _p(np.array(lo, np.int32)), _p(np.array(hi, np.int32)), _p(out))
    return out


# ---- the specification in numpy ---------------------------------------------------------------------------------------------------
def _first_sign(*xs):
    """the sign of the first non-zero of the arguments (arrays broadcast against scalars)"""
    out = np.zeros(np.broadcast(*xs).shape, np.int64)
    for x in xs[::-1]:
        out = np.where(np.asarray(x) != 0, np.sign(x), out)
    return out


def crosses_below(v, lo, hi):
    """bool[hx, hy, hz]: does the snapped triangle v (3, 3) int64 cross below each cell of the box -- the header's cascade, in int64"""
    shape = tuple(h - l for l, h in zip(lo, hi))
    n = np.cross(v[1] - v[0], v[2] - v[1])
    sg = int(np.sign(n[2]))
    if sg == 0:
        return np.zeros(shape, bool)
    qx, qy, qz = (64 * np.arange(l, h, dtype=np.int64) + 32 for l, h in zip(lo, hi))
    qx, qy = qx[:, None], qy[None, :]
    inn = np.ones(shape[:2], bool)
    for p, r in ((v[0], v[1]), (v[1], v[2]), (v[2], v[0])):
        d = r - p
        inn &= sg * _first_sign(d[0] * (qy - p[1]) - d[1] * (qx - p[0]), -d[1], d[0]) > 0
    out = np.zeros(shape, bool)
    ix, iy = np.nonzero(inn)                                                                                    # (F where the column is not in decides nothing)
    f = (n[0] * (qx[ix, 0] - v[0][0]) + n[1] * (qy[0, iy] - v[0][1]))[:, None] + n[2] * (qz - v[0][2])[None, :]
    out[ix, iy] = sg * _first_sign(f, n[0], n[1], n[2]) > 0
    return out


def inside(tris, G, lo, hi):
    """bool[hx, hy, hz]: the parity over the valid triangles"""
    par = np.zeros(tuple(h - l for l, h in zip(lo, hi)), bool)
    s = V.snap(V.vertices(tris), G)
    for k in np.flatnonzero(V.valid(tris)):
        par ^= crosses_below(s[k], lo, hi)
    return par


def brute(mat, rgb, tris, lo, hi, voxel):
    """(mat, rgb, result) after the call"""
    mat, rgb = mat.copy(), rgb.copy()
    res = np.zeros(1, RESULT)[0]
    if len(tris) == 0 or any(h <= l for l, h in zip(lo, hi)):
        return mat, rgb, res
    res["invalid"] = int((~V.valid(tris)).sum())
    w = inside(tris, mat.shape[0], lo, hi)
    if w.any():
        voxel = int(voxel)
        c = np.argwhere(w) + np.array(lo)
        mat[c[:, 0], c[:, 1], c[:, 2]] = np.uint8(voxel >> 24).view(np.int8)
        rgb[c[:, 0], c[:, 1], c[:, 2]] = (voxel & 0xFF, (voxel >> 8) & 0xFF, (voxel >> 16) & 0xFF)
        res["lo"], res["hi"], res["voxels"] = c.min(axis=0), c.max(axis=0) + 1, int(w.sum())
    return mat, rgb, res


# ---- geometry, exactly ------------------------------------------------------------------------------------------------------------
EPS = Fraction(1, 2 ** 80)
# Why 2^-80 is small enough to stand for the infinitesimal.  Every perturbed quantity is an integer plus a polynomial in eps whose
# coefficients are integers below 2^38 (edge components < 2^18, normal components < 2^37): E + (-d_y) eps + d_x eps^2 and
# F + n_x eps + n_y eps^2 + n_z eps^3.  A non-zero integer term is >= 1 in magnitude, and everything after it is below
# 3 * 2^38 * 2^-80 < 1: it keeps its sign.  If the terms up to eps^(k-1) vanish, the eps^k term is >= eps^k in magnitude and all later
# ones together are below 2 * 2^38 * eps^(k+1) = 2^-41 eps^k: again the first non-zero term decides, which is the header's cascade.


def exact_crossing(v, cx, cy):
    """For the snapped triangle v (3 integer triples) and column (cx, cy): None if the vertical line through the perturbed centre
    misses the triangle, else the height (a fraction) at which it meets the triangle's plane.  Plain strict tests: the point is strictly
    on the inner side of the three projected edges.  Cell cz of the column is crossed below iff that height < 64 cz + 32 + eps^3."""
    v = [[int(x) for x in p] for p in v]
    px, py = 64 * cx + 32 + EPS, 64 * cy + 32 + EPS ** 2
    area = (v[1][0] - v[0][0]) * (v[2][1] - v[0][1]) - (v[1][1] - v[0][1]) * (v[2][0] - v[0][0])
    if area == 0:
        return None
    for i in range(3):
        p, r = v[i], v[(i + 1) % 3]
        side = (r[0] - p[0]) * (py - p[1]) - (r[1] - p[1]) * (px - p[0])
        if side * area <= 0:
            return None
    # barycentric interpolation of z: no normal, no plane function
    w1 = ((px - v[0][0]) * (v[2][1] - v[0][1]) - (py - v[0][1]) * (v[2][0] - v[0][0])) / area
    w2 = ((v[1][0] - v[0][0]) * (py - v[0][1]) - (v[1][1] - v[0][1]) * (px - v[0][0])) / area
    return v[0][2] + w1 * (v[1][2] - v[0][2]) + w2 * (v[2][2] - v[0][2])


def exact_first_cell(height):
    """the smallest cz with height < 64 cz + 32 + eps^3"""
    cz = (height - 32) // 64                                                                                    # floor, exact
    while not height < 64 * cz + 32 + EPS ** 3:
        cz += 1
    while height < 64 * (cz - 1) + 32 + EPS ** 3:
        cz -= 1
    return int(cz)


def convex_sides(s, cells):
    """For a CONVEX closed mesh (snapped triangles s (n, 3, 3) int64): (strictly inside, strictly outside) bool per cell, centres
    against every face plane in integers; the reference side is that of an integer point near the vertices' mean."""
    ref = np.round(s.reshape(-1, 3).mean(axis=0)).astype(np.int64)
    q = 64 * np.asarray(cells, np.int64) + 32
    n = np.cross(s[:, 1] - s[:, 0], s[:, 2] - s[:, 1])                                                          # (n, 3)
    keep = (n != 0).any(axis=1)
    n, v0 = n[keep], s[keep, 0]
    side_ref = np.sign(((ref[None] - v0) * n).sum(axis=1))
    assert (side_ref != 0).all()
    side = np.sign(q @ n.T - (v0 * n).sum(axis=1)[None])                                                        # (cells, faces), int64: below 2^56
    return (side == side_ref[None]).all(axis=1), (side == -side_ref[None]).any(axis=1)


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
PAY = int(V.payload((90, 160, 230), 11))
TET = [(0, 1, 2), (0, 3, 1), (1, 3, 2), (2, 3, 0)]


def mesh(G, vox, faces=None):
    """_abi.TRIANGLE records from voxel-unit vertices; their own `voxel` words hold a payload the call must ignore"""
    vox = np.asarray(vox, np.float64)
    return V.triangles(G, vox if faces is None else vox.reshape(-1, 3)[np.asarray(faces)], payloads=np.uint32(0x7F0B0C0D))


def torus(centre, major, minor, nu=16, nv=8):
    u, v = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    ring = major + minor * np.cos(v)
    pts = np.stack([ring * np.cos(u), ring * np.sin(u), minor * np.sin(v)], axis=-1).reshape(-1, 3) + np.asarray(centre, np.float64)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    return pts, np.array([t for i in range(nu) for j in range(nv) for t in ((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))])


def fan(apex, base_z, ring):
    """a pyramid: a fan of triangles from the apex down to a ring, closed below by a fan around the ring's centre"""
    ax, ay, az = apex
    ring = [(x, y, base_z) for x, y in ring]
    tris = []
    for k in range(len(ring)):
        a, b = ring[k], ring[(k + 1) % len(ring)]
        tris += [[apex, a, b], [(ax, ay, base_z), b, a]]
    return np.array(tris, np.float64)


CONVEX = ("cube_planes", "cube_centres", "tetra_centres", "fan_apex", "icosphere")
SAME_AS_ICOSPHERE = ("reversed", "mixed", "halves")
NOTHING = ("duplicated", "flat", "below", "above")
GENERIC = CONVEX + ("torus", "nested", "overlap") + SAME_AS_ICOSPHERE + NOTHING + ("hemisphere", "invalid", "slivers", "poke", "carve", "negative")


def cases():
    return [(n, G) for n in GENERIC for G in (128, 256)]


def origin(G):
    return G // 2 - 16


def default_box(G):
    """36 x 34 x 47 voxels around the meshes: two toggle words a column, neither end on a word or brick boundary; the meshes span
    z' = 12 .. 36 of it, across the word boundary, so the carry is exercised"""
    o = origin(G)
    return (o - 2, o - 1, o - 7), (o + 34, o + 33, o + 40)


@functools.lru_cache(maxsize=None)
def case(name, G):
    """(base scene, [(tris, lo, hi, voxel), ...]).  The meshes live in the 32^3 cells at the grid's centre, o = G / 2 - 16, coordinates
    below relative to o; each is the smallest case of something that can go wrong (tests/test_gpu_fill.py's docstring)."""
    base = "s1_256" if G == 256 else "sunlit"
    o = origin(G)
    lo, hi = default_box(G)
    at = lambda pts: np.asarray(pts, np.float64) + o
    ico = lambda c=(16.3, 15.6, 16.9), r=11.7, sub=1: V.icosphere(tuple(x + o for x in c), r, sub)
    one = lambda tris, pay=PAY: (base, [(tris, lo, hi, pay)])
    if name == "cube_planes":                         # faces in grid planes: no centre lies on anything
        return one(mesh(G, V.cube12((o + 6, o + 9, o + 5), (o + 19, o + 25, o + 22))))
    if name == "cube_centres":                        # faces through cell centres: depth ties on two faces, edge ties on the four side faces' diagonals and borders, vertex ties at the corners
        return one(mesh(G, at(V.cube12((6.5, 9.5, 5.5), (19.5, 25.5, 22.5)))))
    if name == "tetra_centres":                       # every vertex on a cell centre
        return one(mesh(G, at([(4.5, 4.5, 6.5), (26.5, 6.5, 9.5), (10.5, 27.5, 12.5), (14.5, 12.5, 28.5)]), TET))
    if name == "fan_apex":                            # six triangles meet in an apex exactly over a column's centre: one of them owns it
        ring = [(26.5, 16.5), (21.5, 25.5), (11.5, 25.5), (6.5, 16.5), (11.5, 7.5), (21.5, 7.5)]
        return one(mesh(G, at(fan((16.5, 16.5, 27.5), 6.5, ring))))
    if name == "icosphere":
        v, f = ico()
        return one(mesh(G, v, f))
    if name == "torus":                               # a hole: columns through it enter and leave twice
        v, f = torus((o + 16.2, o + 15.7, o + 16.4), 9.3, 3.9)
        return one(mesh(G, v, f))
    if name == "nested":                              # a sphere inside a sphere: a hollow ball
        (v0, f0), (v1, f1) = ico(), ico(r=6.3, sub=0)
        return one(np.concatenate([mesh(G, v0, f0), mesh(G, v1, f1)]))
    if name == "overlap":                             # two closed meshes that overlap: XOR
        (v0, f0), (v1, f1) = ico((12.2, 14.1, 15.3), 8.8), ico((20.4, 18.2, 17.6), 8.6)
        return one(np.concatenate([mesh(G, v0, f0), mesh(G, v1, f1)]))
    if name in ("reversed", "mixed"):                 # orientation must not matter
        v, f = ico()
        f = f.copy()
        sel = slice(None) if name == "reversed" else slice(0, None, 3)
        f[sel] = f[sel][:, ::-1]
        return one(mesh(G, v, f))
    if name == "halves":                              # the box filled in two calls, split along z off any word boundary: the lower call's triangles lie below the upper box
        v, f = ico()
        t = mesh(G, v, f)
        return base, [(t, lo, hi[:2] + (o + 15,), PAY), (t, lo[:2] + (o + 15,), hi, PAY)]
    if name == "duplicated":                          # every triangle twice: cancels
        v, f = ico()
        t = mesh(G, v, f)
        return one(np.concatenate([t, t]))
    if name == "flat":                                # a closed mesh of no volume: a tilted quad and its back side
        a, b, c, d = (4.5, 5.5, 8.5), (27.5, 6.5, 12.5), (28.5, 26.5, 20.5), (5.5, 25.5, 16.5)
        return one(mesh(G, at([[a, b, c], [a, c, d], [c, b, a], [d, c, a]])))
    if name in ("below", "above"):                    # a closed cube under / over a flat box: every column crossed twice, or never
        z = (2, 8) if name == "below" else (22, 30)
        t = mesh(G, V.cube12((o + 6, o + 9, o + z[0]), (o + 19, o + 25, o + z[1])))
        return base, [(t, (o, o, o + 10), (o + 32, o + 32, o + 20), PAY)]
    if name == "hemisphere":                          # open: defined, everything above the cap inside the box
        v, f = ico()
        return one(mesh(G, v, f[v[f].mean(axis=1)[:, 2] > o + 16.9]))
    if name == "invalid":                             # one triangle of a closed mesh is invalid: skipped, counted, the rest is an open mesh
        v, f = ico()
        t = mesh(G, v, f)
        t["v1"][37, 1] = np.nan
        return one(t)
    if name == "slivers":                             # a tetrahedron 1/64 thick, and sub-voxel ones around and beside a cell centre
        thin = at([(1, 1, 1.5), (29, 30.25, 28.5), (29 + 1 / 64, 30.25, 28.5), (29, 30.25 + 1 / 64, 28.5 + 1 / 64)])
        around = at(np.array([(10.5, 10.5, 10.5)]) + np.array([(-6, -5, -7), (9, -4, -6), (-3, 10, -5), (1, 2, 12)]) / 64)
        beside = at(np.array([(20.25, 7.25, 9.75)]) + np.array([(-6, -5, -7), (9, -4, -6), (-3, 10, -5), (1, 2, 12)]) / 64)
        return one(np.concatenate([mesh(G, p, TET) for p in (thin, around, beside)]))
    if name == "poke":                                # the mesh pokes through all six sides of a small box whose corners are outside it
        v, f = ico(r=13.7)
        return base, [(mesh(G, v, f), (o + 7, o + 8, o + 9), (o + 25, o + 24, o + 25), PAY)]
    if name == "carve":                               # a solid block, then a sphere carved out of it with mat = 0
        v, f = ico((14.2, 17.1, 15.8), 8.4)
        block = mesh(G, V.cube12((o + 3, o + 4, o + 5), (o + 29, o + 28, o + 27)))
        return base, [(block, lo, hi, int(V.payload((200, 90, 40), 21))), (mesh(G, v, f), lo, hi, int(V.payload((1, 2, 3), 0)))]
    if name == "negative":                            # a negative material byte: stored as it is, texel alpha 0, not occupied
        return one(mesh(G, at([(4.5, 4.5, 6.5), (26.5, 6.5, 9.5), (10.5, 27.5, 12.5), (14.5, 12.5, 28.5)]), TET), int(V.payload((9, 99, 199), -5)))
    raise KeyError(name)


@functools.lru_cache(maxsize=8)
def states(name, G):
    """[(mat, rgb, result)]: the base grid (result None) and the brute force's grid and result after each call"""
    base, calls = case(name, G)
    out = [R.scene(base)[:2] + (None,)]
    for tris, lo, hi, voxel in calls:
        out.append(brute(out[-1][0], out[-1][1], tris, lo, hi, voxel))
    return out


same_result = V.same_result
