"""Boxes for vrt_sweep_boxes: scenes (tests/cast.py's), box families from fixed seeds, the expected records and the host build of
voxel_rt2_amd/csrc/vrt_sweep.h (tests/emul/sweep_emul.cpp).  Test infrastructure shared by tests/test_sweep_boxes_host.py (no GPU) and
tests/test_gpu_sweep_boxes.py.  Records are compared bit for bit (mismatches()).

Expected values come from brute() alone: include/vrt_api.h's specification stated once in numpy float32, independently of vrt_sweep.h.
For each box it evaluates the per-cell test on EVERY solid voxel of the grid -- the solids are unpacked from the finest pyramid level as
tests/edit.py's rebuild builds it, not taken from a candidate region -- and takes the minimum under the total order (start overlap, t's
bits, linear index; the floor first).  numpy's float32 +, -, *, / are the correctly rounded binary32 operations and nothing is contracted.
Where the specification says dm_max / dm_min, np.maximum / np.minimum serve: no operand is ever a NaN (move_a != 0 where a quotient is
formed, and its numerator is finite), and the two can differ only in the sign of a zero, which none of `<`, `>=`, `==` and `+ 0.0f` sees."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import cast as K
import edit as E
import rays as R
from voxel_rt2_amd import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_SO = os.path.join(HERE, "emul", "_sweep_emul.so")
_lib = None
BOX, HIT = _abi.BOX_SWEEP, _abi.SWEEP_HIT
INF = np.float32(np.inf)
F = np.float32

SCENES = ("sunlit", "s1", "one_voxel", "dense", "s1_256", "empty", "tie")
CENSUS = ("sunlit", "s1", "dense", "s1_256")
FAMILIES = ("random", "resting", "dyadic", "overlap", "zeros", "thin", "extreme", "outside", "far", "span", "tmax", "invalid")
MAX_COORD = 64.0


def scene(name):
    return K.scene(name)


def per_family(name):
    """boxes a family: the brute force visits every solid per box, so few where there are more than a million of them"""
    return 32 if int((scene(name)[0] > 0).sum()) > 1000000 else 360


def cases():
    return [(s, f) for s in SCENES for f in FAMILIES]


# ---- the specification in numpy ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def derived(name):
    mat, rgb, _ = scene(name)
    return E.rebuild(mat, rgb)


def solids_of(l0, G):
    """int[n, 3]: the cells whose bit is set in the finest level (words (bz * n + by) * n + bx, bit z * 16 + y * 4 + x), in the order
    of their linear index (x * G + y) * G + z"""
    n = G // 4
    bits = np.unpackbits(np.ascontiguousarray(l0).view(np.uint8), bitorder="little").reshape(n, n, n, 4, 4, 4)   # bz by bx z y x
    cells = bits.transpose(2, 5, 1, 4, 0, 3).reshape(G, G, G)                                                   # [x][y][z]
    return np.argwhere(cells != 0)


@functools.lru_cache(maxsize=None)
def solids(name):
    G = scene(name)[0].shape[0]
    s = solids_of(derived(name)["l0"], G)
    assert len(s) == int((scene(name)[0] > 0).sum())
    return s


def planes(G):
    p = np.arange(G + 1, dtype=F) * F(2.0 / G) - F(1.0)
    assert (p.astype(np.float64) == np.arange(G + 1) * (2.0 / G) - 1.0).all()                                   # exact in binary32
    return p


def valid(b):
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(b["lo"]).all(axis=1) & np.isfinite(b["hi"]).all(axis=1) & np.isfinite(b["move"]).all(axis=1)
        ok &= (b["lo"] <= b["hi"]).all(axis=1) & (np.abs(b["lo"]) <= MAX_COORD).all(axis=1) & (np.abs(b["hi"]) <= MAX_COORD).all(axis=1)
        ok &= (b["t_max"] > 0) & (b["reserved"] == 0)
    return ok


def miss_record(n):
    want = np.zeros(n, HIT)
    want["t"], want["cell"] = INF, -1
    return want


def _cell_terms(box, p, S):
    """enter[n], exit[n], never[n], e[3][n] of the per-cell test of one box on the cells S"""
    n = len(S)
    e, x = [], []
    never = np.zeros(n, bool)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore", under="ignore"):
        for a in range(3):
            lo, hi, m = F(box["lo"][a]), F(box["hi"][a]), F(box["move"][a])
            plo, phi = p[:-1], p[1:]                                                                            # per cell index on this axis
            if m > 0:
                ea, xa = (plo - hi) / m, (phi - lo) / m
            elif m < 0:
                ea, xa = (phi - lo) / m, (plo - hi) / m
            else:
                ea, xa = np.full(len(plo), -INF, F), np.full(len(plo), INF, F)
                never |= ~((lo < phi) & (hi > plo))[S[:, a]]
            assert ea.dtype == F and xa.dtype == F
            e.append(ea[S[:, a]])
            x.append(xa[S[:, a]])
        enter = np.maximum(np.maximum(e[0], e[1]), e[2])
        exit_ = np.minimum(np.minimum(x[0], x[1]), x[2])
    return enter, exit_, never, e


def brute(name, boxes, S=None, floor_height=None):
    """(want records, info) for the boxes on scene `name` (or on the solids S with the given floor).  info, one entry a box, for the
    census and the region check: index_tie, axis_tie, floor_tie (bools), acc_lo / acc_hi (the bounds of every accepted cell, lo > hi
    where none was)."""
    mat, _, params = scene(name)
    G = mat.shape[0]
    S = solids(name) if S is None else S
    fh = F(params["floor_height"] if floor_height is None else floor_height)
    p = planes(G)
    lin = (S[:, 0].astype(np.int64) * G + S[:, 1]) * G + S[:, 2]
    n = len(boxes)
    want = miss_record(n)
    info = dict(index_tie=np.zeros(n, bool), axis_tie=np.zeros(n, bool), floor_tie=np.zeros(n, bool),
                acc_lo=np.full((n, 3), 1 << 20, np.int64), acc_hi=np.full((n, 3), -1, np.int64))
    ok = valid(boxes)
    for k in np.flatnonzero(ok):
        b = boxes[k]
        t_max = F(b["t_max"])
        enter, exit_, never, e = _cell_terms(b, p, S)
        with np.errstate(invalid="ignore"):
            met = (enter < exit_) & (exit_ > 0) & ~never
            start = met & (enter < 0)
            t = (enter + F(0.0)).astype(F)
            contact = met & (enter >= 0) & (t < t_max)
        acc = start | contact
        if acc.any():
            info["acc_lo"][k], info["acc_hi"][k] = S[acc].min(axis=0), S[acc].max(axis=0)
        # the floor
        floor_start, t_f = False, None
        if not (int(b["flags"]) & _abi.SWEEP_NO_FLOOR):
            if F(b["lo"][1]) < fh:
                floor_start = True
            elif F(b["move"][1]) < 0:
                with np.errstate(over="ignore", under="ignore"):
                    tf = F(F(fh - F(b["lo"][1])) / F(b["move"][1])) + F(0.0)
                if tf < t_max:
                    t_f = F(tf)
        if floor_start:
            want[k]["t"], want[k]["kind"] = 0.0, _abi.SWEEP_START
        elif start.any():
            c = S[np.flatnonzero(start)[np.argmin(lin[start])]]
            want[k]["t"], want[k]["kind"], want[k]["cell"] = 0.0, _abi.SWEEP_START, c
        else:
            tv = t[contact].min() if contact.any() else None
            if t_f is not None and (tv is None or t_f <= tv):                                                   # the floor is tested first
                want[k]["t"], want[k]["kind"] = t_f, _abi.SWEEP_FLOOR
                want[k]["normal"] = (0.0, 1.0, 0.0)
                info["floor_tie"][k] = tv is not None and tv == t_f
            elif tv is not None:
                at = contact & (t == tv)                                                                        # (t >= +0: equal values are equal bits)
                i = np.flatnonzero(at)[np.argmin(lin[at])]
                axes = [a for a in range(3) if e[a][i] == enter[i]]
                normal = np.zeros(3, F)
                normal[axes[0]] = -1.0 if b["move"][axes[0]] > 0 else 1.0
                want[k]["t"], want[k]["kind"], want[k]["cell"], want[k]["normal"] = tv, _abi.SWEEP_VOXEL, S[i], normal
                info["index_tie"][k], info["axis_tie"][k] = at.sum() > 1, len(axes) > 1
    return want, info


# ---- the box families (world units) ----------------------------------------------------------------------------------------------
def _boxes(lo, hi, move, t_max=1.0):
    b = np.zeros(len(lo), BOX)
    with np.errstate(over="ignore", invalid="ignore"):
        b["lo"], b["hi"], b["move"], b["t_max"] = lo, hi, move, t_max
    return b


def _cells(S, G, rng, n):
    """n cells to aim at: solid ones, or any where the grid has none"""
    return S[rng.integers(0, len(S), n)].astype(np.float64) if len(S) else rng.integers(0, G, (n, 3)).astype(np.float64)


def _beside(S, G, rng, n):
    """n x/z positions (voxel units) clear of every solid's column, where there is room: beside the solids' bounds, else outside the grid"""
    lo, hi = (S.min(axis=0), S.max(axis=0) + 1) if len(S) else (np.array([G // 2] * 3), np.array([G // 2] * 3))
    out = rng.uniform(0, G, (n, 3))
    side = rng.random(n) < 0.5
    a = np.where(rng.random(n) < 0.5, 0, 2)
    off = rng.uniform(14.0, 30.0, n)
    out[np.arange(n), a] = np.where(side, lo[a] - off, hi[a] + off)
    return out


def _t_max(rng, n):
    return np.select([np.arange(n) % 3 == 0, np.arange(n) % 3 == 1], [np.full(n, 1.0), np.full(n, np.inf)], rng.uniform(0.05, 2.0, n))


def random_boxes(rng, G, S, fh, n):
    """0.5 to 12 voxels an edge.  Centres: near a solid, anywhere around the grid, beside the solids and above the floor.  Moves: anywhere,
    towards a solid, down."""
    dx = 2.0 / G
    size = rng.uniform(0.5, 12.0, (n, 3))
    k = np.arange(n) % 5
    t_max = _t_max(rng, n)
    floor_y = (fh + 1.0) / dx
    centre = rng.uniform(-0.2 * G, 1.2 * G, (n, 3))
    lift = (np.arange(n) % 8 != 0) & (centre[:, 1] - size[:, 1] / 2 < floor_y)                                   # most of them start above the floor
    centre[lift, 1] = floor_y + size[lift, 1] / 2 + rng.uniform(0.0, 40.0, int(lift.sum()))
    near = _cells(S, G, rng, n) + rng.normal(0.0, 9.0, (n, 3))
    centre[k == 1] = near[k == 1]
    centre[k == 2] = near[k == 2] + np.array([0.0, 14.0, 0.0])
    height = rng.uniform(2.0, 40.0, n)
    beside = _beside(S, G, rng, n)
    beside[:, 1] = floor_y + size[:, 1] / 2 + height
    centre[k >= 3] = beside[k >= 3]
    move = rng.standard_normal((n, 3)) * rng.uniform(0.0, 40.0, (n, 1))
    aim = _cells(S, G, rng, n) + 0.5 - centre
    move[k == 1] = (aim * rng.uniform(0.3, 1.5, (n, 1)))[k == 1]
    move[k == 2] = (np.array([0.0, -1.0, 0.0]) * rng.uniform(4.0, 60.0, (n, 1)) + rng.normal(0.0, 1.0, (n, 3)))[k == 2]
    reach = (height + rng.uniform(1.0, 30.0, n)) / np.where(np.isfinite(t_max), t_max, 1.0)                     # far enough to land within t_max
    move[k >= 3] = (np.array([0.0, -1.0, 0.0]) * reach[:, None] + rng.normal(0.0, 0.5, (n, 3)))[k >= 3]
    lo, hi = (centre - size / 2) * dx - 1.0, (centre + size / 2) * dx - 1.0
    return _boxes(lo, hi, move * dx, t_max)


def resting_boxes(rng, G, S, fh, n):
    """A face of the box exactly in a face plane of a solid voxel (lo or hi equal to a p(k)) or in the floor plane, the box over the
    voxel's face on the other axes; moving into the face, away from it and along it."""
    dx = 2.0 / G
    p = planes(G).astype(np.float64)
    cells = _cells(S, G, rng, n).astype(np.int64)
    size = rng.uniform(0.5, 3.0, (n, 3))
    a = rng.integers(0, 3, n)
    a[::3] = 1
    above = rng.random(n) < 0.5
    above[::3] = True
    rows = np.arange(n)
    if len(S):                                                                                                  # cells whose neighbour on that side is empty
        occ = np.zeros((G + 2,) * 3, bool)
        occ[S[:, 0] + 1, S[:, 1] + 1, S[:, 2] + 1] = True
        for axis in range(3):
            for up in (False, True):
                step = np.eye(3, dtype=np.int64)[axis] * (1 if up else -1)
                free = S[~occ[tuple((S + 1 + step).T)]]
                pick = (a == axis) & (above == up)
                if len(free):
                    cells[pick] = free[rng.integers(0, len(free), int(pick.sum()))]
    centre = cells + rng.uniform(0.0, 1.0, (n, 3))
    lo, hi = (centre - size / 2) * dx - 1.0, (centre + size / 2) * dx - 1.0
    w = size[rows, a] * dx
    lo[rows, a] = np.where(above, p[cells[rows, a] + 1], p[cells[rows, a]] - w)
    hi[rows, a] = np.where(above, p[cells[rows, a] + 1] + w, p[cells[rows, a]])
    how = (np.arange(n) // 3) % 3                                                                               # into, away, along
    move = rng.normal(0.0, 2.0, (n, 3)) * dx
    into = np.where(above, -1.0, 1.0) * rng.uniform(0.5, 6.0, n) * dx
    move[rows, a] = np.select([how == 0, how == 1], [into, -into], np.where(rng.random(n) < 0.5, 0.0, -0.0))
    fl = np.arange(n) % 5 >= 3                                                                                  # on the floor plane
    beside = _beside(S, G, rng, n) * dx - 1.0
    lo[fl] = beside[fl] - size[fl] * dx / 2
    hi[fl] = beside[fl] + size[fl] * dx / 2
    lo[fl, 1] = F(fh)
    hi[fl, 1] = F(fh) + size[fl, 1] * dx
    move[fl, 1] = np.select([how[fl] == 0, how[fl] == 1], [-np.abs(into[fl]), np.abs(into[fl])], 0.0)
    return _boxes(lo, hi, move, np.where(np.arange(n) % 2 == 0, 1.0, np.inf))


def dyadic_boxes(rng, G, S, fh, n):
    """Faces on grid planes, moves whole or half cells a unit of t: contacts with several cells at bit-equal t (a box wider than a cell
    onto a flat surface: index ties) and onto an edge or a corner (a diagonal move from a diagonal offset: axis ties)."""
    dx = 2.0 / G
    cells = _cells(S, G, rng, n).astype(np.int64)
    size = rng.integers(1, 6, (n, 3))
    k = np.arange(n) % 3
    lo = np.empty((n, 3), np.int64)
    move = np.zeros((n, 3))
    step = rng.choice((0.5, 1.0, 2.0, 4.0), n)
    # k == 0: straight down (or along another axis) onto the cell from d cells away, the box overhanging it on the other axes
    # k == 1, 2: from a diagonal offset of d cells on two or three axes, moving back along the diagonal at equal speed
    d = rng.integers(0, 9, n)
    sign = rng.choice((-1, 1), (n, 3))
    axes = np.zeros((n, 3), bool)
    axes[np.arange(n), rng.integers(0, 3, n)] = True
    axes[k == 0, 1] = (rng.random(int((k == 0).sum())) < 0.6) | axes[k == 0, 1]
    axes[k == 0] &= np.cumsum(axes[k == 0], axis=1) == 1                                                         # exactly one axis
    two = rng.integers(0, 3, n)
    axes[k == 1] = np.arange(3)[None, :] != two[k == 1, None]
    axes[k == 2] = True
    for a in range(3):
        off = np.where(sign[:, a] > 0, cells[:, a] + 1 + d, cells[:, a] - d - size[:, a])                       # the box's lo when it is d cells off on this axis
        over = cells[:, a] - rng.integers(0, size[:, a])                                                         # ... when it overlaps the cell's slab
        lo[:, a] = np.where(axes[:, a], off, over)
        move[:, a] = np.where(axes[:, a], -sign[:, a] * step, 0.0)
    free = ~axes & (rng.random((n, 3)) < 0.25) & (k[:, None] == 0)
    move = np.where(free, rng.choice((-1.0, 1.0, 0.5), (n, 3)), move)                                           # sliding while it falls
    hi = lo + size
    return _boxes(lo * dx - 1.0, hi * dx - 1.0, move * dx, np.where(np.arange(n) % 4 == 0, np.inf, 16.0))


def tie_boxes(rng, n):
    """The tie scene only: over the voxels that hang under the floor plane with their top faces in it (x 96..115, z 40..79), falling
    straight down or askew by dyadic moves: the floor's t and the voxels' are bit-equal, and the floor is tested first."""
    dx = 1.0 / 64
    size = rng.integers(1, 5, (n, 3))
    lo = np.stack([rng.integers(94, 114, n), 48 + rng.integers(0, 20, n), rng.integers(38, 78, n)], axis=1)
    move = np.stack([rng.choice((0.0, 0.0, 0.5, -1.0), n), -rng.choice((0.5, 1.0, 2.0, 3.0), n), rng.choice((0.0, -0.0, 1.0), n)], axis=1)
    return _boxes(lo * dx - 1.0, (lo + size) * dx - 1.0, move * dx, np.inf)


def overlap_boxes(rng, G, S, fh, n):
    """Boxes that start inside solids, under the floor plane, or both; and next to them boxes that only touch."""
    dx = 2.0 / G
    cells = _cells(S, G, rng, n)
    size = rng.uniform(0.2, 6.0, (n, 3))
    centre = cells + rng.uniform(0.0, 1.0, (n, 3))
    k = np.arange(n) % 4
    beside = _beside(S, G, rng, n)
    centre[k == 1] = beside[k == 1]
    lo, hi = (centre - size / 2) * dx - 1.0, (centre + size / 2) * dx - 1.0
    under = (k == 1) | (k == 2)
    drop = rng.uniform(0.01, 3.0, n) * dx
    shift = np.where(under, np.minimum(F(fh) - drop - lo[:, 1], 0.0), 0.0)                                      # lo_y below the plane
    shift = np.where(k == 2, F(fh) - drop - lo[:, 1], shift)                                                    # ... taking a box in a solid along: both
    lo[:, 1] += shift
    hi[:, 1] += shift
    touch = k == 3                                                                                              # only touching the cell, from above
    lo[touch, 1] = (np.floor(cells[touch, 1]) + 1) * dx - 1.0
    hi[touch, 1] = lo[touch, 1] + size[touch, 1] * dx
    move = rng.normal(0.0, 3.0, (n, 3)) * dx
    move[::5] = 0.0
    return _boxes(lo, hi, move, _t_max(rng, n))


def zero_component_boxes(rng, G, S, fh, n):
    """`random` with one or two move components +0 or -0."""
    b = random_boxes(rng, G, S, fh, n)
    zeros = np.zeros((n, 3), bool)
    zeros[np.arange(n), rng.integers(0, 3, n)] = True
    second = rng.random(n) < 0.5
    zeros[np.arange(n)[second], rng.integers(0, 3, n)[second]] = True
    zeros[zeros.all(axis=1), 1] = False
    b["move"] = np.where(zeros, np.where(rng.random((n, 3)) < 0.5, 0.0, -0.0), b["move"])
    return b


def thin_boxes(rng, G, S, fh, n):
    """Sheets, segments and points: lo == hi on one, two or three axes; some of them on grid planes."""
    b = random_boxes(rng, G, S, fh, n)
    flat = np.zeros((n, 3), bool)
    for j in range(n):
        flat[j, rng.permutation(3)[:1 + j % 3]] = True
    mid = ((b["lo"].astype(np.float64) + b["hi"]) / 2)
    snap = rng.random((n, 3)) < 0.3
    mid = np.where(snap, np.round((mid + 1.0) * (G / 2.0)) * (2.0 / G) - 1.0, mid).astype(F)
    b["lo"] = np.where(flat, mid, b["lo"])
    b["hi"] = np.where(flat, mid, b["hi"])
    return b


def extreme_boxes(rng, G, S, fh, n):
    """Subnormal and 1e30 move components with t_max = inf (and a few finite ones)."""
    b = random_boxes(rng, G, S, fh, n)
    mag = rng.choice((1e-40, 1e-45, 3e-39, 1e30, 3e38, 1e20), (n, 3))
    which = rng.random((n, 3)) < 0.6
    which[np.arange(n), rng.integers(0, 3, n)] = True
    with np.errstate(over="ignore"):
        b["move"] = np.where(which, np.sign(b["move"]) * mag, b["move"]).astype(F)
    b["t_max"] = np.where(np.arange(n) % 5 == 0, rng.choice((1e-30, 1.0, 1e30), n), np.inf)
    return b


def outside_boxes(rng, G, S, fh, n):
    """Partly or wholly outside the grid: straddling a face of it, beyond it and moving in, past, away."""
    dx = 2.0 / G
    size = rng.uniform(0.5, 12.0, (n, 3))
    centre = rng.uniform(0.0, G, (n, 3))
    a = rng.integers(0, 3, n)
    side = rng.choice((-1.0, 1.0), n)
    dist = np.where(np.arange(n) % 3 == 0, rng.uniform(-4.0, 4.0, n), rng.uniform(4.0, 200.0, n))               # straddling / beyond
    rows = np.arange(n)
    centre[rows, a] = np.where(side > 0, G + dist, -dist)
    target = _cells(S, G, rng, n) + 0.5
    move = (target - centre) * rng.uniform(0.5, 2.0, (n, 1))
    k = np.arange(n) % 5                                                                                        # 0, 1: in, towards a solid
    move[k == 2] = rng.normal(0.0, 20.0, (n, 3))[k == 2]
    move[k == 3] = (np.array([0.0, -1.0, 0.0]) * rng.uniform(10.0, 300.0, (n, 1)))[k == 3]
    centre[k == 3, 1] = np.maximum(centre[k == 3, 1], (fh + 1.0) / dx + 8.0)
    move[k == 4] *= -1.0
    lo, hi = (centre - size / 2) * dx - 1.0, (centre + size / 2) * dx - 1.0
    return _boxes(lo, hi, move * dx, _t_max(rng, n))


def far_boxes(rng, G, S, fh, n):
    """A coordinate exactly at +-64: boxes that start there and come in, and boxes that reach from there into the grid."""
    dx = 2.0 / G
    b = random_boxes(rng, G, S, fh, n)
    lo, hi, move = b["lo"].astype(np.float64), b["hi"].astype(np.float64), b["move"].astype(np.float64)
    a = rng.integers(0, 3, n)
    rows = np.arange(n)
    k = np.arange(n) % 4
    w = hi[rows, a] - lo[rows, a]
    target = _cells(S, G, rng, n)[rows, a] * dx - 1.0
    lo[rows, a] = np.select([k == 0, k == 1, k == 2], [64.0 - w, -64.0, lo[rows, a]], -64.0)
    hi[rows, a] = np.select([k == 0, k == 1, k == 2], [64.0, -64.0 + w, 64.0], hi[rows, a])
    move[rows, a] = np.select([k == 0, k == 1], [(target - 64.0) * rng.uniform(0.5, 1.5, n), (target + 64.0) * rng.uniform(0.5, 1.5, n)], move[rows, a])
    return _boxes(lo, hi, move, b["t_max"])


def span_boxes(rng, G, S, fh, n):
    """One box spanning the whole grid (the first), then boxes of a quarter of the grid and more an edge, resting and moving."""
    size = np.where(np.arange(n)[:, None] % 3 == 0, rng.uniform(0.5, 2.2, (n, 3)), rng.uniform(0.25, 0.6, (n, 3)))
    centre = rng.uniform(-0.9, 0.9, (n, 3))
    lo, hi = centre - size / 2, centre + size / 2
    lo[0], hi[0] = -1.0, 1.0
    lo[1::2, 1] = (S[:, 1].max() + 1 if len(S) else G // 2) * (2.0 / G) - 1.0 + rng.uniform(0.0, 0.2, len(lo[1::2]))   # above every solid
    hi[1::2, 1] = lo[1::2, 1] + size[1::2, 1]
    move = rng.normal(0.0, 0.3, (n, 3))
    move[0] = 0.0
    move[1::2] = np.array([0.0, -1.0, 0.0]) * rng.uniform(0.1, 2.0, (len(move[1::2]), 1))
    return _boxes(lo, hi, move, np.where(np.arange(n) % 2 == 0, 1.0, np.inf))


def invalid_boxes(rng, G, S, fh, n):
    """The invalid classes -- a non-finite field, lo > hi, a coordinate beyond +-64, t_max NaN, 0 or negative, a non-zero `reserved` --
    and between them valid neighbours: t_max = inf, lo == hi, a coordinate at exactly +-64, a tiny t_max, a huge move."""
    b = random_boxes(rng, G, S, fh, n).copy()
    bad = np.array([np.inf, -np.inf, np.nan], F)
    for j in range(n):
        c, a = j % 12, int(rng.integers(0, 3))
        if c == 0:
            b[("lo", "hi", "move")[int(rng.integers(0, 3))]][j, a] = bad[rng.integers(0, 3)]
        elif c == 1:
            b["lo"][j, a], b["hi"][j, a] = b["hi"][j, a] + F(1e-3), b["lo"][j, a]
        elif c == 2:
            if rng.random() < 0.5:
                b["hi"][j, a] = np.nextafter(F(64.0), INF)
            else:
                b["lo"][j, a] = np.nextafter(F(-64.0), -INF)
        elif c == 3:
            b["t_max"][j] = (np.nan, 0.0, -0.0, -1.0, -np.inf)[rng.integers(0, 5)]
        elif c == 4:
            b["reserved"][j] = (1, 0x80000000, 7)[rng.integers(0, 3)]
        elif c == 5:
            b["t_max"][j] = np.inf
        elif c == 6:
            b["hi"][j, a] = b["lo"][j, a]
        elif c == 7:
            if rng.random() < 0.5:
                b["hi"][j, a] = 64.0
            else:
                b["lo"][j, a] = -64.0
        elif c == 8:
            b["t_max"][j] = (1e-40, 1e-6)[rng.integers(0, 2)]
        elif c == 9:
            b["move"][j, a] = (1e30, -1e30, 1e-40)[rng.integers(0, 3)]
        elif c == 10:
            b["flags"][j] = 0xFFFFFFFE | (j & 1)                                                                # unknown flag bits are ignored
    return b


_MAKERS = dict(random=random_boxes, resting=resting_boxes, dyadic=dyadic_boxes, overlap=overlap_boxes, zeros=zero_component_boxes,
               thin=thin_boxes, extreme=extreme_boxes, outside=outside_boxes, far=far_boxes, span=span_boxes, invalid=invalid_boxes)


@functools.lru_cache(maxsize=None)
def family(name, fam):
    """(boxes, expected records, info) of one family on one scene: generated once, from a seed of its own, and left alone.  Every other
    box of a family carries VRT_SWEEP_NO_FLOOR."""
    mat, _, params = scene(name)
    G, fh = mat.shape[0], params["floor_height"]
    S = solids(name)
    n = per_family(name)
    rng = np.random.default_rng([20251019, SCENES.index(name), FAMILIES.index(fam)])
    if fam == "tmax":     # the boxes of `random`, `resting` and `dyadic` that meet something later than at once: t_max just below, at, just above t, and far off
        src = [family(name, f) for f in ("random", "resting", "dyadic", "zeros")]
        boxes, want = np.concatenate([s[0] for s in src]), np.concatenate([s[1] for s in src])
        pick = np.flatnonzero(np.isfinite(want["t"]) & (want["t"] > 0))
        pick = pick[np.linspace(0, len(pick) - 1, min(n, len(pick))).astype(int)] if len(pick) else pick
        boxes, t = boxes[pick].copy(), want["t"][pick]
        choice = np.arange(len(boxes)) % 4
        boxes["t_max"] = np.select([choice == 0, choice == 1, choice == 2], [np.nextafter(t, F(0)), t, np.nextafter(t, INF)], F(2.0) * t)
    else:
        boxes = _MAKERS[fam](rng, G, S, fh, n)
        if name == "tie" and fam == "dyadic":
            boxes = np.concatenate([boxes, tie_boxes(rng, 240)])
        if fam != "invalid":
            boxes["flags"] = np.arange(len(boxes)) % 2
            if name == "tie" and fam == "dyadic":
                boxes["flags"][-240:] = (np.arange(240) % 4 == 3)
        else:
            boxes["flags"] |= (np.arange(len(boxes)) % 2).astype(np.uint32)
    want, info = brute(name, boxes)
    assert len(boxes) <= 4000 and (len(S) <= 1000000 or len(boxes) <= 200)
    for a in (boxes, want) + tuple(info.values()):
        a.setflags(write=False)
    return boxes, want, info


def census(names=CENSUS):
    """Over every family of the named scenes: valid boxes and, of their expected records, the kinds, the six contact normals, the ties
    and the contacts at exactly t = 0."""
    out = dict(valid=0, miss=0, floor=0, voxel=0, start=0, index_ties=0, axis_ties=0, floor_ties=0, at_zero=0, normals=[0] * 6)
    for name in names:
        for fam in FAMILIES:
            boxes, want, info = family(name, fam)
            ok = valid(boxes)
            out["valid"] += int(ok.sum())
            for k, key in ((_abi.SWEEP_MISS, "miss"), (_abi.SWEEP_FLOOR, "floor"), (_abi.SWEEP_VOXEL, "voxel"), (_abi.SWEEP_START, "start")):
                out[key] += int((ok & (want["kind"] == k)).sum())
            out["index_ties"] += int(info["index_tie"].sum())
            out["axis_ties"] += int(info["axis_tie"].sum())
            out["floor_ties"] += int(info["floor_tie"].sum())
            contact = (want["kind"] == _abi.SWEEP_FLOOR) | (want["kind"] == _abi.SWEEP_VOXEL)
            out["at_zero"] += int((contact & (want["t"] == 0)).sum())
            for a in range(3):
                for s, sign in enumerate((-1.0, 1.0)):
                    out["normals"][2 * a + s] += int(((want["kind"] == _abi.SWEEP_VOXEL) & (want["normal"][:, a] == sign)).sum())
    return out


def check_census(report=print):
    """The brute force's answers alone: no comparison passes on misses, on one kind of record, on one face or without ties."""
    for name in CENSUS:
        c = census((name,))
        report(f"sweep census {name:8s} {c}")
        for key in ("miss", "floor", "voxel", "start"):
            assert 10 * c[key] >= c["valid"], (name, key, c)
    c = census(CENSUS)
    report(f"sweep census all      {c}")
    assert min(c["normals"]) >= 100, c
    assert c["index_ties"] >= 50 and c["axis_ties"] >= 50 and c["at_zero"] >= 100, c
    t = census(("tie",))
    report(f"sweep census tie      {t}")
    assert t["floor_ties"] >= 50, t
    assert scene("tie")[2]["floor_height"] == 48 * (1 / 64) - 1
    for name in SCENES:
        boxes = family(name, "invalid")[0]
        bad = int((~valid(boxes)).sum())
        assert len(boxes) // 4 <= bad <= len(boxes) - len(boxes) // 4, (name, bad)


# ---- comparison ----------------------------------------------------------------------------------------------------------------
def mismatches(got, want):
    """Indices of the records that differ in any field, floats by their bits."""
    bad = ~R.same_f32(got["t"], want["t"]) | (got["kind"] != want["kind"]) | (got["cell"] != want["cell"]).any(axis=1)
    bad |= ~R.same_f32(got["normal"], want["normal"]).all(axis=1)
    return np.flatnonzero(bad)


def check(got, boxes, want, label):
    bad = mismatches(got, want)
    assert bad.size == 0, f"{label}: {bad.size} of {len(boxes)} records differ: " + "; ".join(f"box {k} {boxes[k]} got={got[k]} want={want[k]}" for k in bad[:3])


# ---- the host build ------------------------------------------------------------------------------------------------------------
class SweepScene(C.Structure):
    _fields_ = [("grid_res", C.c_int32), ("pad", C.c_int32), ("floor_height", C.c_float), ("pad2", C.c_float), ("cull", C.c_float * 8),
                ("l0", C.c_void_p), ("l1", C.c_void_p)]


GXX = ["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unknown-pragmas"]


def sources():
    csrc = os.path.join(ROOT, "voxel_rt2_amd", "csrc")
    src = os.path.join(HERE, "emul", "sweep_emul.cpp")
    return src, [src, os.path.join(ROOT, "include", "vrt_api.h"), os.path.join(ROOT, "include", "vrt_detmath.h")] + \
        [os.path.join(csrc, f) for f in ("vrt_sweep.h", "vrt_plan.h", "vrt_trace.h", "vrt_types.h")]


def lib():
    global _lib
    if _lib is None:
        src, deps = sources()
        if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
            subprocess.run(GXX + ["-shared", "-o", _SO, src], check=True, capture_output=True)
        _lib = C.CDLL(_SO)
        _lib.sweep_emul_boxes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]
        _lib.sweep_emul_regions.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
        _lib.sweep_emul_valid.argtypes = [C.c_void_p]
        _lib.sweep_emul_chunk.restype = C.c_longlong
        _lib.sweep_emul_blocks.argtypes = [C.c_longlong, C.c_int, C.c_int]
        _lib.sweep_emul_sizes.argtypes = [C.c_int]
    return _lib


class HostScene:
    """The scene as k_sweep_boxes reads it, built in numpy (tests/edit.py: rebuild; tests/rays.py: grown_box), for sweep_emul_boxes."""

    def __init__(self, name, open_box=False):
        mat, rgb, params = scene(name)
        self.keep = derived(name)
        s = self.s = SweepScene()
        s.grid_res, s.floor_height = mat.shape[0], params["floor_height"]
        lo, hi, _ = R.grown_box(mat)
        s.cull[:] = [-1e30] * 3 + [1e30] * 3 + [0.0, 0.0] if open_box else list(lo) + list(hi) + [1.0, 0.0]
        s.l0, s.l1 = self.keep["l0"].ctypes.data, self.keep["l1"].ctypes.data

    def sweep(self, boxes, lanes=64, prune=True):
        out = np.zeros(len(boxes), HIT)
        boxes = np.ascontiguousarray(boxes)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib().sweep_emul_boxes(C.byref(self.s), int(lanes), int(prune), len(boxes), p(boxes), p(out)) == 0
        return out

    def regions(self, boxes):
        out = np.zeros((len(boxes), 7), np.int32)
        boxes = np.ascontiguousarray(boxes)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib().sweep_emul_regions(C.byref(self.s), len(boxes), p(boxes), p(out)) == 0
        return out
