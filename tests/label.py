"""Connected components (vrt_label_components): the named case families, two brute forces that every result is compared with, and the
host build of voxel_rt2_amd/csrc/vrt_label.h (tests/emul/label_emul.cpp) behind ctypes.  Test infrastructure shared by
tests/test_label_host.py (no GPU) and tests/test_gpu_label.py.  Every comparison is byte for byte, over every cell of the box, plus
the result record.

Expected values come from the brute forces alone.  Neither knows anything of union-find, tiles or forward neighbours: include/vrt_api.h's
definition stated twice --
  brute_propagate   every member seeded with its own grid index; the minimum over the whole neighbourhood, masked to members, again
                    and again until nothing changes (numpy; asserts that it converged within MAX_ROUNDS rounds, so a wrong grid cannot
                    make a test crawl);
  brute_flood       members visited in ascending index order, a flood with an explicit queue from each one still unlabelled, whose
                    index is the component's label (plain Python: small boxes, and the long chains that propagation is slow on).
reference() takes whichever is affordable; test_label_host.py asserts once that they agree where both are.

A case is dict(grid, lo, hi, conn, empty); grid(name) is its materials.  The families sit side by side in one 128^3 grid ("families"),
each in a box of its own at an unaligned offset, once with the family's cells solid and once with them empty in a solid block."""
import collections
import ctypes as C
import functools
import itertools
import os
import subprocess

import numpy as np

import distance as D
from voxel_rt2_amd import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_SO = os.path.join(HERE, "emul", "_label_emul.so")
_SRC = os.path.join(HERE, "emul", "label_emul.cpp")
GCC = D.GCC
_lib = None
GUARD = 4096
MAX_ROUNDS = 1024
POISON = 0x5A5A5A5A
CONN_FLAG = {6: 0, 18: _abi.LABEL_CONN_18, 26: _abi.LABEL_CONN_26}


def flags_of(conn, empty):
    return CONN_FLAG[conn] | (_abi.LABEL_EMPTY if empty else 0)


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(ROOT, "voxel_rt2_amd", "csrc")
        deps = [_SRC, os.path.join(ROOT, "include", "vrt_api.h")] + [os.path.join(csrc, f) for f in ("vrt_label.h", "vrt_edit.h", "vrt_trace.h", "vrt_types.h", "vrt_plan.h")]
        if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
            subprocess.run(GCC + ["-fPIC", "-shared", "-o", _SO, _SRC], check=True, capture_output=True)
        _lib = C.CDLL(_SO)
        _lib.label_emul_plan.restype = C.c_longlong
        _lib.label_emul_plan.argtypes = [C.c_longlong, C.c_int]
        _lib.label_emul_tile.argtypes = [C.c_void_p]
        _lib.label_emul_forward.argtypes = [C.c_uint, C.c_void_p]
        _lib.label_emul_call.argtypes = [C.c_int] + [C.c_void_p] * 3 + [C.c_uint] + [C.c_void_p] * 3 + [C.c_int, C.c_uint, C.c_int, C.c_void_p]
    return _lib


build = lib
_p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- the host build ---------------------------------------------------------------------------------------------------------------
def emul_plan(nv, staged=False):
    return int(lib().label_emul_plan(int(nv), int(staged)))


@functools.lru_cache(maxsize=None)
def tile():
    out = np.zeros(3, np.int32)
    lib().label_emul_tile(_p(out))
    return tuple(int(v) for v in out)


def emul_forward(conn):
    out = np.zeros(39, np.int32)
    n = lib().label_emul_forward(CONN_FLAG[conn], _p(out))
    return [tuple(int(v) for v in out[3 * k:3 * k + 3]) for k in range(n)]


def emul_call(mat, lo, hi, conn=6, empty=False, flags=None, staged=False, seed=0, stale=False, want_result=True, after_tiles=False):
    """vrt_label_components on host arrays: (return code, labels, result dict or None[, the words after the tile phase]).  The scratch
    is plan_label_layout's byte count followed by a guard that must come back untouched: the plan bounds what the phases write."""
    mat = np.ascontiguousarray(mat, np.int8)
    G = mat.shape[0]
    flags = flags_of(conn, empty) if flags is None else flags
    shape = tuple(max(h - l, 0) for l, h in zip(lo, hi))
    labels = np.full(shape, POISON, np.int32)
    res = np.full(1, -7, _abi.LABEL_RESULT) if want_result else None
    mid = np.full(shape, POISON, np.int32) if after_tiles else None
    need = emul_plan(int(np.prod(shape)), staged)
    scratch = np.full(need + GUARD, 0xA5, np.uint8)
    rc = lib().label_emul_call(G, _p(mat), _p(np.array(lo, np.int32)), _p(np.array(hi, np.int32)), flags, _p(labels), _p(res), _p(scratch), int(staged), int(seed),
                               int(stale), _p(mid))
    assert (scratch[need:] == 0xA5).all(), "the phases wrote past plan_label_layout's byte count"
    r = None if res is None else {k: int(res[0][k]) for k in ("cells", "components", "reserved")}
    return (rc, labels, r, mid) if after_tiles else (rc, labels, r)


# ---- the two references -------------------------------------------------------------------------------------------------------------
def neighbourhood(conn):
    """every offset of the neighbourhood (both halves): |d| <= 1 per axis, 1 <= |d|_1 <= 1, 2 or 3"""
    most = {6: 1, 18: 2, 26: 3}[conn]
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if 1 <= sum(abs(v) for v in o) <= most]


def members_of(mat, lo, hi, empty):
    sl = tuple(slice(l, h) for l, h in zip(lo, hi))
    return (mat[sl] > 0) != bool(empty)


def grid_indices(G, lo, hi):
    ax = [np.arange(l, h, dtype=np.int32) for l, h in zip(lo, hi)]
    return (ax[0][:, None, None] * G + ax[1][None, :, None]) * G + ax[2][None, None, :]


def brute_propagate(mat, lo, hi, conn=6, empty=False, max_rounds=MAX_ROUNDS):
    """(labels, rounds)"""
    big = np.int32(0x7FFFFFFF)
    member = members_of(mat, lo, hi, empty)
    shape = member.shape
    lab = np.where(member, grid_indices(mat.shape[0], lo, hi), big).astype(np.int32)
    if lab.size == 0:
        return np.full(shape, -1, np.int32), 0
    pad = np.full(tuple(s + 2 for s in shape), big, np.int32)
    offs = neighbourhood(conn)
    for rounds in range(1, max_rounds + 1):
        pad[1:-1, 1:-1, 1:-1] = lab
        new = lab.copy()
        for o in offs:
            np.minimum(new, pad[tuple(slice(1 + d, 1 + d + s) for d, s in zip(o, shape))], out=new)
        new[~member] = big
        if np.array_equal(new, lab):
            return np.where(member, lab, -1).astype(np.int32), rounds
        lab = new
    raise AssertionError(f"brute_propagate did not converge within {max_rounds} rounds: the wrong grid?")


def brute_flood(mat, lo, hi, conn=6, empty=False):
    member = members_of(mat, lo, hi, empty)
    shape = member.shape
    G = mat.shape[0]
    out = np.full(shape, -1, np.int32)
    todo = member.copy()
    offs = neighbourhood(conn)
    for flat in np.flatnonzero(member):                                                       # ascending: box order is grid order
        c = np.unravel_index(flat, shape)
        if not todo[c]:
            continue
        seed = ((lo[0] + int(c[0])) * G + lo[1] + int(c[1])) * G + lo[2] + int(c[2])
        todo[c] = False
        queue = collections.deque([tuple(int(v) for v in c)])
        while queue:
            x, y, z = queue.popleft()
            out[x, y, z] = seed
            for dx, dy, dz in offs:
                u = (x + dx, y + dy, z + dz)
                if 0 <= u[0] < shape[0] and 0 <= u[1] < shape[1] and 0 <= u[2] < shape[2] and todo[u]:
                    todo[u] = False
                    queue.append(u)
    return out


def affordable(mat, lo, hi, conn, empty, deep=False):
    """(brute_propagate is, brute_flood is)"""
    n = int(members_of(mat, lo, hi, empty).sum())
    return not deep, n * len(neighbourhood(conn)) <= 1_500_000


def reference(mat, lo, hi, conn=6, empty=False, deep=False):
    by_propagate, by_flood = affordable(mat, lo, hi, conn, empty, deep)
    assert by_propagate or by_flood, "neither brute force is affordable for this case: choose a smaller one"
    return brute_propagate(mat, lo, hi, conn, empty)[0] if by_propagate else brute_flood(mat, lo, hi, conn, empty)


def record_of(labels, G, lo):
    """the result record the labels imply: members, and cells that carry their own index"""
    own = grid_indices(G, lo, tuple(l + s for l, s in zip(lo, labels.shape)))
    return dict(cells=int((labels >= 0).sum()), components=int((labels == own).sum()), reserved=0)


def table_of(labels, G, lo):
    """the table of components the labels imply, sorted by root: (root, size, lo[3], hi[3]) -- hi exclusive, grid coordinates"""
    rows = []
    for root in np.unique(labels[labels >= 0]):
        at = np.argwhere(labels == root)
        rows.append((int(root), len(at), tuple(int(v) + l for v, l in zip(at.min(0), lo)), tuple(int(v) + l + 1 for v, l in zip(at.max(0), lo))))
    return rows


# ---- the families: member masks of a box ---------------------------------------------------------------------------------------------
SHAPE = (17, 18, 70)            # 3 x 3 x 2 tiles of 8 x 8 x 64, none of the high ones whole


def serpentine(shape):
    """One 6-connected chain through the box, built by walking it: z lines at even (x, y) visited boustrophedon in y within a layer and
    in x across layers, each hop to the next line going through the one odd cell between them at the z end the walk has reached."""
    m = np.zeros(shape, bool)
    xs, ys = list(range(0, shape[0], 2)), list(range(0, shape[1], 2))
    z_end = 0
    for i, x in enumerate(xs):
        row = ys if i % 2 == 0 else ys[::-1]
        for j, y in enumerate(row):
            m[x, y, :] = True
            z_end = shape[2] - 1 - z_end                                                      # the walk runs the line to its other end
            if j + 1 < len(row):
                m[x, (y + row[j + 1]) // 2, z_end] = True
            elif i + 1 < len(xs):
                m[x + 1, y, z_end] = True
    return m


def combs(shape):
    """two interleaved combs: teeth along y at x = 0, 4, 8.. from a spine at y = 0, and at x = 2, 6, .. from a spine at y = ny - 1"""
    m = np.zeros(shape, bool)
    ny = shape[1]
    m[0::4, 0:ny - 2, :] = True
    m[:, 0, :] = True
    m[2::4, 2:ny, :] = True
    m[:, ny - 1, :] = True
    return m


def _cells(shape, cells):
    m = np.zeros(shape, bool)
    for c in cells:
        m[tuple(c)] = True
    return m


def family(name, shape=SHAPE, seed=1):
    """bool[shape]: the members"""
    tx, ty, tz = tile()
    x, y, z = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    if name == "none":
        return np.zeros(shape, bool)
    if name == "full":
        return np.ones(shape, bool)
    if name == "corners":
        return _cells(shape, itertools.product(*[(0, s - 1) for s in shape]))
    if name == "checker":
        return (x + y + z) % 2 == 0
    if name == "tile_edge":                                                                  # pairs that meet across an edge of a tile only
        return _cells(shape, [(tx - 1, ty - 1, 5), (tx, ty, 5), (3, ty - 1, tz - 1), (3, ty, tz), (tx - 1, 12, tz), (tx, 12, tz - 1),
                              (2 * tx, 2, 9), (2 * tx - 1, 1, 9)])
    if name == "tile_corner":                                                                # pairs that meet across a corner of a tile only
        return _cells(shape, [(tx - 1, ty - 1, tz - 1), (tx, ty, tz), (2 * tx - 1, ty, tz - 1), (2 * tx, ty - 1, tz), (tx, 2 * ty - 1, tz), (tx - 1, 2 * ty, tz - 1)])
    if name == "serpentine":
        return serpentine(shape)
    if name == "serpentine_mirror":
        return np.ascontiguousarray(serpentine(shape)[::-1, ::-1, ::-1])
    if name == "combs":
        return combs(shape)
    if name == "reenter":                                                                    # two slabs that a shell outside the box joins
        return (x % 6 < 2) & (y > 1) & (z > 2)
    if name.startswith("random"):
        return np.random.default_rng(seed).random(shape) < float(name[6:]) / 10.0
    raise KeyError(name)


FAMILIES = ("none", "full", "corners", "checker", "tile_edge", "tile_corner", "serpentine", "serpentine_mirror", "combs", "reenter", "random1", "random3", "random6")
DEEP = ("serpentine", "serpentine_mirror")            # chains that propagation needs thousands of rounds for: brute_flood
SLOT_Z = 51


def slot(family_name, empty):
    """(lo, hi) of the box a family sits in, in the "families" grid"""
    i = FAMILIES.index(family_name) * 2 + int(bool(empty))
    lo = (1 + 18 * (i % 7), 2 + 19 * (i // 7), SLOT_Z)
    return lo, tuple(l + s for l, s in zip(lo, SHAPE))


def embed(mat, mask, lo, empty, shell=False):
    """the members of `mask` written into mat at lo: solid where a member (non-solid with `empty`), and the other way round elsewhere in
    the box; non-solid bytes are 0 or negative.  shell: the layer of cells around the box made members too."""
    hi = tuple(l + s for l, s in zip(lo, mask.shape))
    G = mat.shape[0]
    if shell:
        out = tuple(slice(max(l - 1, 0), min(h + 1, G)) for l, h in zip(lo, hi))
        mat[out] = 0 if empty else 9
    solid = mask != bool(empty)
    x, y, z = np.meshgrid(*[np.arange(s) for s in mask.shape], indexing="ij")
    mat[tuple(slice(l, h) for l, h in zip(lo, hi))] = np.where(solid, 1 + (x + 2 * y + 3 * z) % 100, np.where((x + y + z) % 3 == 0, -5, 0)).astype(np.int8)


def noise(G, seed):
    """half the cells solid, the others 0 or negative"""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((G, G, G)) < 0.5, rng.integers(1, 120, (G, G, G)), rng.integers(-3, 1, (G, G, G))).astype(np.int8)


EDIT_BOX = ((40, 60, 50), (80, 100, 90))


@functools.lru_cache(maxsize=None)
def grid(name):
    """int8[G][G][G]: the materials of a named grid"""
    if name == "families":
        mat = noise(128, 77)
        for f in FAMILIES:
            for empty in (False, True):
                embed(mat, family(f), slot(f, empty)[0], empty, shell=f == "reenter")
        mat.setflags(write=False)
        return mat
    if name == "small":                                                                      # an edge that is no power of two
        mat = noise(40, 5)
        mat.setflags(write=False)
        return mat
    if name == "long":                                                                       # room for 2 T + 1 cells along z
        mat = noise(136, 6)
        mat.setflags(write=False)
        return mat
    if name == "cube32":
        mat = noise(32, 8)
        mat.setflags(write=False)
        return mat
    if name == "s1_edit":
        return D.grid("s1_edit")
    return D.grid(name)


def colours(name):
    if name in ("families", "small", "long", "cube32"):
        m = grid(name)
        x, y, z = np.meshgrid(*[np.arange(m.shape[0])] * 3, indexing="ij")
        return np.where((m != 0)[..., None], np.stack([x * 2 + 1, y + 100, 255 - z], -1) % 256, 0).astype(np.uint8)
    return D.colours(name)


def params(name):
    return D.params(name if name not in ("families", "small", "long", "cube32") else "empty")


def _case(grid, lo, hi, conn=6, empty=False, deep=False):
    return dict(grid=grid, lo=tuple(int(v) for v in lo), hi=tuple(int(v) for v in hi), conn=conn, empty=bool(empty), deep=deep)


CASES = {}
for _f in FAMILIES:
    for _e in (False, True):
        for _c in (6, 18, 26):
            CASES[f"{_f}_{'empty' if _e else 'solid'}_{_c}"] = _case("families", *slot(_f, _e), conn=_c, empty=_e, deep=_f in DEEP)
FAMILY_NAMES = tuple(CASES)
# three at 256^3, in the half of the grid whose indices exceed 2^23
CASES_256 = {
    "sponge256_solid_6": _case("sponge256", (130, 100, 61), (187, 150, 192)),
    "sponge256_empty_26": _case("sponge256", (199, 3, 120), (256, 40, 256), conn=26, empty=True),
    "sponge256_solid_18": _case("sponge256", (128, 200, 0), (160, 256, 70), conn=18),
}
CASES.update(CASES_256)
# half the cells solid: 64^3 boxes at two offsets
DENSE_BOXES = (((0, 0, 0), (64, 64, 64)), ((37, 61, 59), (101, 125, 123)))
for _i, (_lo, _hi) in enumerate(DENSE_BOXES):
    for _e in (False, True):
        for _c in (6, 18, 26):
            CASES[f"dense{_i}_{'empty' if _e else 'solid'}_{_c}"] = _case("dense", _lo, _hi, conn=_c, empty=_e)
DENSE_NAMES = tuple(n for n in CASES if n.startswith("dense"))
WHOLE = {
    "dense_whole_solid_6": _case("dense", (0, 0, 0), (128, 128, 128)),
    "s1_whole_empty_6": _case("s1", (0, 0, 0), (128, 128, 128), empty=True),
}
CASES.update(WHOLE)
CASES["s1_edit"] = _case("s1_edit", *EDIT_BOX, conn=26)
CASES["s1_before_edit"] = _case("s1", *EDIT_BOX, conn=26)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(labels, record) of a case, from a brute force; computed once, shared, never written to"""
    c = CASES[name]
    m = grid(c["grid"])
    labels = reference(m, c["lo"], c["hi"], c["conn"], c["empty"], c["deep"])
    labels.setflags(write=False)
    return labels, record_of(labels, m.shape[0], c["lo"])


def check(got, got_record, want, label):
    """byte for byte, every cell of the box; then the record"""
    labels, record = want
    assert got.dtype == np.int32 and got.shape == labels.shape, (label, got.dtype, got.shape, labels.shape)
    if got.tobytes() != labels.tobytes():
        bad = np.argwhere(got != labels)
        raise AssertionError(f"{label}: labels differ in {len(bad)} of {labels.size} cells, first at box cell {bad[0].tolist()}: {got[tuple(bad[0])]} != {labels[tuple(bad[0])]}")
    if got_record is not None:
        assert {k: int(got_record[k]) for k in ("cells", "components", "reserved")} == record, (label, got_record, record)
