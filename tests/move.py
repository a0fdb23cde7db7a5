"""Moving voxels (vrt_move_voxels): the named cases, two brute forces that every result is compared with, and the host build of
voxel_rt2_amd/csrc/vrt_move.h (tests/emul/move_emul.cpp) behind ctypes.  Test infrastructure shared by tests/test_move_host.py (no GPU)
and tests/test_gpu_move_voxels.py.  Every comparison is byte for byte, over every voxel of the grid, plus the result record.

Expected values come from the brute forces alone.  Neither knows anything of snapshot words, z steps, tiles or the order of the passes:
include/vrt_api.h's rules stated twice --
  brute      every cell of the grid at once in numpy int64: the map, the piece cells, who receives, who is vacated, who is occupied, the
             final grid and the record;
  brute_py   the same rules cell by cell in Python's unbounded ints (small boxes: the cases at the coefficient bounds).
tests/test_move_host.py asserts once that they agree.

A case is dict(grid, src, dst, m, t, flags, select, value); grid(name) is (mat, rgb).  Maps are written as the FORWARD map a reader thinks
in -- p' = R (p - pivot) + pivot + shift -- and inverted here: exactly, in integers, for the signed permutation matrices (inverse_exact),
in float64 like the facade for the others (inverse_rounded)."""
import ctypes as C
import functools
import itertools
import os
import subprocess

import numpy as np

import distance as D
import label as L
from voxel_rt2_amd import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_SO = os.path.join(HERE, "emul", "_move_emul.so")
_SRC = os.path.join(HERE, "emul", "move_emul.cpp")
GCC = D.GCC
_lib = None
GUARD = 4096
ERASE, KEEP, DRY, IF_FREE = _abi.MOVE_ERASE_SOURCE, _abi.MOVE_KEEP_SOLID, _abi.MOVE_DRY_RUN, _abi.MOVE_IF_FREE
ONE = 1 << 16


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(ROOT, "voxel_rt2_amd", "csrc")
        deps = [_SRC, os.path.join(ROOT, "include", "vrt_api.h")] + [os.path.join(csrc, f) for f in ("vrt_move.h", "vrt_edit.h", "vrt_trace.h", "vrt_types.h")]
        if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
            subprocess.run(GCC + ["-fPIC", "-shared", "-o", _SO, _SRC], check=True, capture_output=True)
        _lib = C.CDLL(_SO)
        _lib.move_emul_plan.restype = C.c_longlong
        _lib.move_emul_plan.argtypes = [C.c_longlong, C.c_longlong, C.c_int]
        _lib.move_emul_tile.argtypes = [C.c_void_p]
        _lib.move_emul_map.argtypes = [C.c_void_p] * 5
        _lib.move_emul_line.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p]
        _lib.move_emul_call.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 2
    return _lib


build = lib
_p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


def record_of(case, flags=None):
    """the vrt_voxel_move record of a case"""
    rec = np.zeros(1, _abi.VOXEL_MOVE)
    rec[0]["src_lo"], rec[0]["src_hi"], rec[0]["dst_lo"], rec[0]["dst_hi"] = case["src"][0], case["src"][1], case["dst"][0], case["dst"][1]
    rec[0]["m"], rec[0]["t"] = case["m"], case["t"]
    rec[0]["select_value"], rec[0]["flags"] = case["value"], case["flags"] if flags is None else flags
    return rec


def result_dict(res):
    return dict(lo=tuple(int(v) for v in res[0]["lo"]), hi=tuple(int(v) for v in res[0]["hi"]), written=int(res[0]["written"]), blocked=int(res[0]["blocked"]),
                erased=int(res[0]["erased"]))


# ---- the host build ---------------------------------------------------------------------------------------------------------------
def emul_call(mat, rgb, case, select=None, staged=False, want_result=True, record=None):
    """vrt_move_voxels on copies of host arrays: (return code, mat, rgb, result dict or None).  The scratch is move_layout's byte count
    followed by a guard that must come back untouched: the plan bounds what the passes write."""
    mat, rgb = np.array(mat, np.int8, order="C"), np.array(rgb, np.uint8, order="C")
    rec = record_of(case) if record is None else record
    n_src = int(np.prod([max(h - l, 0) for l, h in zip(rec[0]["src_lo"], rec[0]["src_hi"])]))
    n_dst = int(np.prod([max(h - l, 0) for l, h in zip(rec[0]["dst_lo"], rec[0]["dst_hi"])]))
    need = int(lib().move_emul_plan(n_src, n_dst, int(select is not None and staged)))
    scratch = np.full(need + GUARD, 0xA5, np.uint8)
    res = np.full(1, -7, _abi.MOVE_RESULT) if want_result else None
    sel = None if select is None else np.ascontiguousarray(select, np.int32)
    rc = lib().move_emul_call(mat.shape[0], _p(mat), _p(rgb), _p(rec), _p(sel), int(staged), _p(res), _p(scratch))
    assert (scratch[need:] == 0xA5).all(), "the passes wrote past move_layout's byte count"
    return rc, mat, rgb, (result_dict(res) if res is not None and rc == 0 else None)


def emul_map(m, t, d):
    S, s = np.zeros(3, np.int64), np.zeros(3, np.int64)
    lib().move_emul_map(_p(np.array(m, np.int32)), _p(np.array(t, np.int64)), _p(np.array(d, np.int32)), _p(S), _p(s))
    return [int(v) for v in S], [int(v) for v in s]


def emul_line(m, t, d, n):
    S = np.zeros((n, 3), np.int64)
    lib().move_emul_line(_p(np.array(m, np.int32)), _p(np.array(t, np.int64)), _p(np.array(d, np.int32)), n, _p(S))
    return S


# ---- the two references -------------------------------------------------------------------------------------------------------------
def brute(mat, rgb, case, select=None, flags=None):
    """(mat, rgb, record) after the call: include/vrt_api.h's rules over every cell of the grid"""
    G = mat.shape[0]
    (slo, shi), (dlo, dhi) = case["src"], case["dst"]
    m, t = [int(v) for v in case["m"]], [int(v) for v in case["t"]]
    flags = case["flags"] if flags is None else flags
    ax = np.arange(G, dtype=np.int64)
    c = [(2 * ax + 1).reshape([-1 if k == a else 1 for k in range(3)]) for a in range(3)]
    cell = [ax.reshape([-1 if k == a else 1 for k in range(3)]) for a in range(3)]
    in_dst = np.ones((G, G, G), bool)
    for a in range(3):
        in_dst &= (cell[a] >= dlo[a]) & (cell[a] < dhi[a])
    piece = np.zeros((G, G, G), bool)                                                        # PIECE CELLS: selected, in the source box, material > 0
    sl = tuple(slice(l, h) for l, h in zip(slo, shi))
    piece[sl] = (mat[sl] > 0) & (True if select is None else np.asarray(select).reshape(piece[sl].shape) == case["value"])
    s, ok = [], in_dst.copy()
    for a in range(3):
        S = m[3 * a] * c[0] + m[3 * a + 1] * c[1] + m[3 * a + 2] * c[2] + t[a]                 # THE MAP, int64
        sa = S >> 17
        ok &= (sa >= slo[a]) & (sa < shi[a])
        s.append(np.clip(sa, 0, G - 1))
    receives = ok & piece[s[0], s[1], s[2]]
    vacated = piece if flags & ERASE else np.zeros_like(piece)
    occupied = (mat > 0) & ~vacated
    blocked = int((receives & occupied).sum())
    takes = receives & ~occupied if flags & KEEP else receives
    record = dict(lo=(0, 0, 0), hi=(0, 0, 0), written=0, blocked=blocked, erased=0)
    if flags & IF_FREE and blocked:
        return mat.copy(), rgb.copy(), record
    at = np.argwhere(takes)
    record["written"], record["erased"] = len(at), int(vacated.sum())
    if len(at):
        record["lo"], record["hi"] = tuple(int(v) for v in at.min(0)), tuple(int(v) + 1 for v in at.max(0))
    if flags & DRY:
        return mat.copy(), rgb.copy(), record
    out_m = np.where(takes, mat[s[0], s[1], s[2]], np.where(vacated, 0, mat)).astype(np.int8)
    out_c = np.where(takes[..., None], rgb[s[0], s[1], s[2]], np.where(vacated[..., None], 0, rgb)).astype(np.uint8)
    return out_m, out_c, record


def brute_py(mat, rgb, case, select=None, flags=None):
    """the same rules, cell by cell in Python ints; only the cells of the two boxes can change"""
    (slo, shi), (dlo, dhi) = case["src"], case["dst"]
    m, t = [int(v) for v in case["m"]], [int(v) for v in case["t"]]
    flags = case["flags"] if flags is None else flags
    in_src = lambda p: all(slo[a] <= p[a] < shi[a] for a in range(3))

    def is_piece(p):
        if not in_src(p) or int(mat[p]) <= 0:
            return False
        return select is None or int(np.asarray(select)[tuple(p[a] - slo[a] for a in range(3))]) == case["value"]
    vac = lambda p: bool(flags & ERASE) and is_piece(p)
    todo, blocked, erased = {}, 0, 0
    for p in itertools.product(*[range(l, h) for l, h in zip(slo, shi)]):
        if vac(p):
            erased += 1
            todo[p] = None
    writes = []
    for d in itertools.product(*[range(l, h) for l, h in zip(dlo, dhi)]):
        s = tuple((sum(m[3 * a + b] * (2 * d[b] + 1) for b in range(3)) + t[a]) >> 17 for a in range(3))
        if not is_piece(s):
            continue
        occupied = int(mat[d]) > 0 and not vac(d)
        blocked += occupied
        if not (flags & KEEP and occupied):
            writes.append(d)
            todo[d] = s
    record = dict(lo=(0, 0, 0), hi=(0, 0, 0), written=0, blocked=blocked, erased=0)
    out_m, out_c = mat.copy(), rgb.copy()
    if flags & IF_FREE and blocked:
        return out_m, out_c, record
    record["written"], record["erased"] = len(writes), erased
    if writes:
        record["lo"], record["hi"] = tuple(min(w[a] for w in writes) for a in range(3)), tuple(max(w[a] for w in writes) + 1 for a in range(3))
    if not flags & DRY:
        for p, s in todo.items():
            out_m[p], out_c[p] = (0, 0) if s is None else (mat[s], rgb[s])
    return out_m, out_c, record


# ---- maps -----------------------------------------------------------------------------------------------------------------------------
def rotations24():
    """the 24 signed permutation matrices of determinant +1, as integer arrays"""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            R = np.zeros((3, 3), np.int64)
            for i in range(3):
                R[i, perm[i]] = signs[i]
            if round(np.linalg.det(R)) == 1:
                out.append(R)
    assert len(out) == 24
    return out


def inverse_exact(R, pivot2=(0, 0, 0), shift=(0, 0, 0)):
    """(m, t) for p' = R (p - pivot) + pivot + shift with R a signed permutation matrix, pivot2 = 2 * pivot and shift in whole numbers: all
    integer arithmetic (the inverse is the transpose)."""
    inv = np.asarray(R, np.int64).T
    p2, s = np.asarray(pivot2, np.int64), np.asarray(shift, np.int64)
    return (inv * ONE).reshape(-1).tolist(), ((p2 - inv @ (p2 + 2 * s)) * ONE).tolist()


def inverse_rounded(R, pivot=(0, 0, 0), shift=(0, 0, 0)):
    inv = np.linalg.inv(np.asarray(R, np.float64))
    pivot, shift = np.asarray(pivot, np.float64), np.asarray(shift, np.float64)
    return np.rint(inv * 65536.0).astype(np.int64).reshape(-1).tolist(), np.rint((pivot - inv @ (pivot + shift)) * 131072.0).astype(np.int64).tolist()


def rot(axis, degrees):
    a, (c, s) = "xyz".index(axis), (np.cos(np.radians(degrees)), np.sin(np.radians(degrees)))
    R = np.eye(3)
    i, j = (a + 1) % 3, (a + 2) % 3
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def image_box(G, src, R, pivot, shift):
    """the bounds of the source box's eight mapped corners, grown by one cell and clipped to the grid"""
    corners = np.array([[src[(k >> a) & 1][a] for a in range(3)] for k in range(8)], np.float64)
    image = (corners - np.asarray(pivot, np.float64)) @ np.asarray(R, np.float64).T + np.asarray(pivot, np.float64) + np.asarray(shift, np.float64)
    lo = np.clip(np.floor(image.min(0)).astype(int) - 1, 0, G)
    hi = np.clip(np.ceil(image.max(0)).astype(int) + 1, 0, G)
    return tuple(int(v) for v in lo), tuple(int(v) for v in np.maximum(lo, hi))


# ---- the grids ------------------------------------------------------------------------------------------------------------------------
SRC = ((61, 13, 2), (68, 19, 7))                  # crosses brick, 16-cell and 64-cell boundaries
FACES = {"x0": ((0, 40, 41), (4, 45, 47)), "x1": ((123, 40, 41), (128, 46, 46)), "y0": ((30, 0, 70), (36, 3, 75)), "y1": ((30, 124, 70), (35, 128, 76)),
         "z0": ((90, 30, 0), (95, 36, 4)), "z1": ((90, 30, 125), (96, 35, 128))}
FREE = ((96, 64, 0), (128, 128, 64))              # no voxel at all: placements that nothing blocks
WHOLE = lambda G: ((0, 0, 0), (G, G, G))


def _fill(mat, rgb, rng, lo, hi, solid, negative):
    shape = tuple(h - l for l, h in zip(lo, hi))
    u = rng.random(shape)
    m = np.where(u < solid, rng.integers(1, 101, shape), np.where(u < solid + negative, rng.integers(-3, 0, shape), 0)).astype(np.int8)
    sl = tuple(slice(l, h) for l, h in zip(lo, hi))
    mat[sl] = m
    rgb[sl] = np.where((m != 0)[..., None], rng.integers(1, 256, shape + (3,)), 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def grid(name):
    """(mat int8[G][G][G], rgb uint8[G][G][G][3]) of a named grid, read-only"""
    if name == "clutter":                          # sparse clutter with negative bytes everywhere but FREE; dense around SRC and in the face boxes
        G, rng = 128, np.random.default_rng(20261021)
        mat, rgb = np.zeros((G, G, G), np.int8), np.zeros((G, G, G, 3), np.uint8)
        _fill(mat, rgb, rng, *WHOLE(G), 0.08, 0.04)
        _fill(mat, rgb, rng, (56, 8, 0), (74, 24, 12), 0.6, 0.15)
        for lo, hi in FACES.values():
            _fill(mat, rgb, rng, lo, hi, 0.6, 0.15)
        sl = tuple(slice(l, h) for l, h in zip(*FREE))
        mat[sl], rgb[sl] = 0, 0
    elif name == "block":                          # one block of solid voxels in empty space, none of them on the faces of its region
        G, rng = 128, np.random.default_rng(5)
        mat, rgb = np.zeros((G, G, G), np.int8), np.zeros((G, G, G, 3), np.uint8)
        _fill(mat, rgb, rng, (60, 12, 4), (68, 20, 12), 1.0, 0.0)
    elif name == "sponge256":
        mat, rgb = D.grid("sponge256"), D.colours("sponge256")
    else:
        raise KeyError(name)
    mat, rgb = np.ascontiguousarray(mat), np.ascontiguousarray(rgb)
    mat.setflags(write=False)
    rgb.setflags(write=False)
    return mat, rgb


def params(name):
    return D.params("sponge256") if name == "sponge256" else D.params("empty")


# ---- the selections -------------------------------------------------------------------------------------------------------------------
def selection(kind, gridname, src):
    """(select or None, value) over the source box"""
    shape = tuple(h - l for l, h in zip(*src))
    if kind is None:
        return None, 0
    if kind == "checker":
        x, y, z = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
        return ((x + y + z) % 2).astype(np.int32), 1
    labels = L.brute_flood(grid(gridname)[0], src[0], src[1], 6, False)
    if kind == "root":                             # the labels of the box, the largest component's root
        roots, sizes = np.unique(labels[labels >= 0], return_counts=True)
        return labels, int(roots[np.argmax(sizes)])
    if kind == "nobody":
        return labels, -5
    raise KeyError(kind)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _case(grid, src, dst, m, t, flags=ERASE, select=None):
    return dict(grid=grid, src=(tuple(src[0]), tuple(src[1])), dst=(tuple(dst[0]), tuple(dst[1])), m=[int(v) for v in m], t=[int(v) for v in t], flags=int(flags),
                select=select, value=None)


def _forward(grid, src, R, pivot, shift, flags=ERASE, select=None, dst=None, exact=False):
    G = 256 if grid == "sponge256" else 128
    m, t = inverse_exact(R, [int(round(2 * v)) for v in pivot], shift) if exact else inverse_rounded(R, pivot, shift)
    return _case(grid, src, image_box(G, src, R, pivot, shift) if dst is None else dst, m, t, flags, select)


CENTRE = (64.5, 16.0, 4.5)                        # of SRC
I3 = np.eye(3, dtype=np.int64)
CASES = {}
CASES["identity_tight"] = _forward("clutter", SRC, I3, (0, 0, 0), (0, 0, 0), dst=SRC, exact=True)
CASES["identity_whole"] = _forward("clutter", SRC, I3, (0, 0, 0), (0, 0, 0), dst=WHOLE(128), exact=True, flags=0)
for _n, _s in (("overlap", (1, 0, 0)), ("near", (0, -3, 2)), ("far", (20, 30, 40)), ("free", (40, 60, 10)), ("cut", (-62, 0, 0)), ("off", (-80, 0, 0))):
    CASES[f"shift_{_n}"] = _forward("clutter", SRC, I3, (0, 0, 0), _s, exact=True)
CASES["shift_whole"] = _forward("clutter", SRC, I3, (0, 0, 0), (-3, 5, 1), dst=WHOLE(128), exact=True)
for _k, _R in enumerate(rotations24()):
    CASES[f"rot{_k:02d}_int"] = _forward("clutter", SRC, _R, (64, 16, 4), (0, 0, 0), exact=True)
    CASES[f"rot{_k:02d}_half"] = _forward("clutter", SRC, _R, (64.5, 15.5, 4.5), (30, 70, 20), exact=True)
ROTATION_NAMES = tuple(n for n in CASES if n.startswith("rot"))
CASES["mirror"] = _forward("clutter", SRC, np.diag([-1, 1, 1]), (64.5, 0, 0), (0, 0, 9), exact=True)
for _a in "xyz":
    CASES[f"turn30_{_a}"] = _forward("clutter", SRC, rot(_a, 30.0), CENTRE, (35, 60, 30))
CASES["shear"] = _case("clutter", SRC, ((50, 5, 0), (80, 30, 14)), [ONE, 20000, 0, 0, ONE, -30000, 1234, 0, ONE], [-3 << 17, 5 << 16, 12345])
CASES["scale_2"] = _forward("clutter", SRC, np.diag([2.0, 2.0, 2.0]), CENTRE, (36, 70, 20))
CASES["scale_half"] = _forward("clutter", SRC, np.diag([0.5, 0.5, 0.5]), CENTRE, (0, 0, 0))
CASES["zero_hit"] = _case("clutter", SRC, ((100, 70, 10), (104, 73, 15)), [0] * 9, [(2 * 63 + 1) << 16, (2 * 15 + 1) << 16, (2 * 4 + 1) << 16])
CASES["zero_miss"] = _case("clutter", SRC, ((100, 70, 10), (104, 73, 15)), [0] * 9, [5 << 17, 5 << 17, 5 << 17])
_B, _T = _abi.MOVE_M_MAX, _abi.MOVE_T_MAX
CASES["bound_m_hit"] = _case("clutter", SRC, WHOLE(128), [_B, 0, 0, 0, -_B, 0, 0, 0, _B], [(61 - 16 * 3 - 8) << 17, (16 * 4 + 8 + 15) << 17, (4 - 8) << 17])
for _k, (_sm, _st) in enumerate(itertools.product((1, -1), repeat=2)):
    CASES[f"bound_all_{_k}"] = _case("clutter", SRC, ((0, 0, 0), (128, 6, 128)), [_sm * _B] * 9, [_st * _T] * 3)
CASES["bound_mixed"] = _case("clutter", SRC, ((120, 120, 120), (128, 128, 128)), [_B, -_B, _B, -_B, _B, -_B, _B, _B, -_B], [_T, -_T, 62 << 17])
BOUND_NAMES = tuple(n for n in CASES if n.startswith("bound") or n.startswith("zero"))
_Rz = rotations24()[10]
CASES["dst_cut_at_face"] = _forward("clutter", SRC, _Rz, (64.5, 15.5, 4.5), (0, 0, -3), exact=True)
CASES["dst_missing"] = _forward("clutter", SRC, _Rz, (64.5, 15.5, 4.5), (30, 70, 20), dst=((2, 2, 2), (9, 9, 9)), exact=True)
CASES["dst_empty"] = _forward("clutter", SRC, _Rz, (64.5, 15.5, 4.5), (30, 70, 20), dst=((70, 70, 70), (70, 75, 75)), exact=True)
CASES["src_empty"] = _case("clutter", ((61, 13, 2), (61, 19, 7)), SRC, (I3 * ONE).reshape(-1), [0, 0, 0])
for _f, _box in FACES.items():
    _a = "xyz".index(_f[0])
    CASES[f"face_{_f}"] = _forward("clutter", _box, rotations24()[5 + _a], [(_box[0][k] + _box[1][k]) // 2 for k in range(3)], [2 if k != _a else 0 for k in range(3)], exact=True)
for _sel in ("root", "nobody", "checker"):
    CASES[f"select_{_sel}_shift"] = _forward("clutter", SRC, I3, (0, 0, 0), (2, 1, 1), select=_sel, exact=True)
    CASES[f"select_{_sel}_turn"] = _forward("clutter", SRC, rot("y", 30.0), CENTRE, (35, 60, 30), select=_sel)
for _fl in range(16):
    CASES[f"flags{_fl:02d}_blocked"] = _forward("clutter", SRC, _Rz, (64.5, 15.5, 4.5), (3, 1, 1), flags=_fl, select="checker", exact=True)
    CASES[f"flags{_fl:02d}_free"] = _forward("clutter", SRC, _Rz, (64.5, 15.5, 4.5), (40, 60, 10), flags=_fl, exact=True)
FLAG_NAMES = tuple(n for n in CASES if n.startswith("flags"))
CASES["whole_onto_itself"] = _forward("clutter", WHOLE(128), rotations24()[7], (64, 64, 64), (0, 0, 0), dst=WHOLE(128), exact=True)
CASE_256 = "sponge256_turn"
CASES[CASE_256] = _forward("sponge256", ((130, 100, 61), (187, 150, 192)), rot("z", 30.0), (158.5, 125.0, 126.5), (20, 40, -10), flags=ERASE | KEEP)
NAMES_128 = tuple(n for n in CASES if n != CASE_256)
# what a device test compares a whole context on (frames, rays): one of each kind
DEEP = ("shift_overlap", "rot10_int", "turn30_y", "select_root_turn", "flags03_blocked", "face_z1")


@functools.lru_cache(maxsize=None)
def select_of(name):
    c = CASES[name]
    sel, value = selection(c["select"], c["grid"], c["src"])
    if sel is not None:
        sel.setflags(write=False)
    return sel, value


def case(name):
    c = dict(CASES[name])
    c["value"] = select_of(name)[1]
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    """(mat, rgb, record) of a case, from the numpy brute force; computed once, shared, never written to"""
    mat, rgb, rec = brute(*grid(CASES[name]["grid"]), case(name), select_of(name)[0])
    mat.setflags(write=False)
    rgb.setflags(write=False)
    return mat, rgb, rec


def check(got_mat, got_rgb, got_record, want, label):
    """byte for byte, every voxel of the grid; then the record"""
    mat, rgb, record = want
    if got_mat.tobytes() != mat.tobytes():
        bad = np.argwhere(got_mat != mat)
        raise AssertionError(f"{label}: materials differ in {len(bad)} cells, first at {bad[0].tolist()}: {got_mat[tuple(bad[0])]} != {mat[tuple(bad[0])]}")
    if got_rgb.tobytes() != rgb.tobytes():
        bad = np.argwhere((got_rgb != rgb).any(-1))
        raise AssertionError(f"{label}: colours differ in {len(bad)} cells, first at {bad[0].tolist()}")
    if got_record is not None:
        assert got_record == record, (label, got_record, record)
