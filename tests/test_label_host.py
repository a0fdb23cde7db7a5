"""vrt_label_components WITHOUT a GPU: the host build of voxel_rt2_amd/csrc/vrt_label.h (tests/emul/label_emul.cpp: the kernels' loops phase
by phase, the entry point's checks, plan_label_layout's scratch) against two brute forces that know nothing of union-find
(tests/label.py).  Byte for byte over every cell of every box, plus the result record:
  - every case family of tests/label.py at 6-, 18- and 26-connectivity, for solid and for empty members: nothing, everything, single cells
    in the corners, a 3-D checkerboard, cells that meet only across an edge or only across a corner of a tile, a serpentine chain and its
    mirror image, two interleaved combs, slabs joined only outside the box, random fills at 0.1, 0.3 and 0.6;
  - the cases are what they claim; the two brute forces agree where both are affordable;
  - boxes of extent 1, T - 1, T, T + 1 and 2 T + 1 on each axis with the tile's edge T there, a corner that is no multiple of the
    tile, boxes on every grid face, a grid whose edge is no power of two, the whole of a 32^3 grid;
  - the host path's staging gives the same bytes; the plan's byte count bounds what is touched (a guard behind it comes back untouched on
    every call);
  - ORDER: several shuffles of the order in which tiles, slots and forward neighbours are visited change no byte; nor does a seam phase
    whose loads return a randomly chosen earlier value of the word;
  - what the tile phase leaves: every member names a member of its own tile and component, no larger than itself;
  - the forward neighbours are the later half of each neighbourhood; export, ctypes binding, constants, the error codes and empty cases."""
import ctypes as C
import re

import numpy as np
import pytest

import label as L
from voxel_rt2_amd import _abi, _lib


@pytest.mark.parametrize("name", L.FAMILY_NAMES)
def test_emulation_equals_brute_force(name):
    c = L.CASES[name]
    rc, labels, record = L.emul_call(L.grid(c["grid"]), c["lo"], c["hi"], c["conn"], c["empty"])
    assert rc == _abi.VRT_OK
    L.check(labels, record, L.expected(name), name)


def test_the_cases_are_what_they_claim():
    comps = lambda n: L.expected(n)[1]["components"]
    cells = lambda n: L.expected(n)[1]["cells"]
    nv = int(np.prod(L.SHAPE))
    for kind in ("solid", "empty"):
        assert cells(f"none_{kind}_6") == 0 and (L.expected(f"none_{kind}_26")[0] == -1).all()
        assert cells(f"full_{kind}_6") == nv and comps(f"full_{kind}_6") == comps(f"full_{kind}_26") == 1
        lo = L.CASES[f"full_{kind}_6"]["lo"]
        assert (L.expected(f"full_{kind}_6")[0] == (lo[0] * 128 + lo[1]) * 128 + lo[2]).all()   # the box's first cell
        assert [comps(f"corners_{kind}_{c}") for c in (6, 18, 26)] == [8, 8, 8]
        assert comps(f"checker_{kind}_6") == cells(f"checker_{kind}_6") == (nv + 1) // 2 and comps(f"checker_{kind}_18") == comps(f"checker_{kind}_26") == 1
        assert [comps(f"tile_edge_{kind}_{c}") for c in (6, 18, 26)] == [8, 4, 4]
        assert [comps(f"tile_corner_{kind}_{c}") for c in (6, 18, 26)] == [6, 6, 3]
        assert [comps(f"serpentine_{kind}_{c}") for c in (6, 18, 26)] == [1, 1, 1]
        assert [comps(f"combs_{kind}_{c}") for c in (6, 18, 26)] == [2, 2, 2]
        assert [comps(f"reenter_{kind}_{c}") for c in (6, 18, 26)] == [3, 3, 3]                # joined outside the box only
        assert comps(f"random3_{kind}_6") > comps(f"random3_{kind}_18") > comps(f"random3_{kind}_26") > 1
    # the serpentine is a chain: every cell but the two ends has exactly two 6-neighbours
    m = np.pad(L.family("serpentine"), 1)
    deg = sum(np.roll(m, s, a) for a in range(3) for s in (-1, 1))[m]
    assert sorted(np.unique(deg, return_counts=True)[1].tolist()) == [2, m.sum() - 2] and set(np.unique(deg).tolist()) == {1, 2}
    # its mirror image's smallest cell is the chain's far end: in the mirror the label is not the first cell the walk laid down
    first = np.argwhere(L.family("serpentine"))[0].tolist()
    assert first == [0, 0, 0] and not L.family("serpentine_mirror")[0, 0, 0]
    # the slabs of `reenter` ARE one piece in the grid: a box one cell larger says so
    c = L.CASES["reenter_solid_6"]
    grown = L.reference(L.grid("families"), [v - 1 for v in c["lo"]], [v + 1 for v in c["hi"]], 6, False)
    inner = grown[1:-1, 1:-1, 1:-1]
    assert len(np.unique(inner[L.expected("reenter_solid_6")[0] >= 0])) == 1


def test_the_two_brute_forces_agree():
    for name in ("tile_edge_solid_18", "tile_corner_empty_26", "combs_solid_6", "reenter_empty_18", "random1_solid_26", "random3_solid_6", "random3_empty_18", "random6_solid_6", "checker_solid_6"):
        c = L.CASES[name]
        m = L.grid(c["grid"])
        assert all(L.affordable(m, c["lo"], c["hi"], c["conn"], c["empty"])), name
        a, rounds = L.brute_propagate(m, c["lo"], c["hi"], c["conn"], c["empty"])
        b = L.brute_flood(m, c["lo"], c["hi"], c["conn"], c["empty"])
        assert a.tobytes() == b.tobytes() and rounds >= 1, name
    lo, hi = (3, 5, 2), (12, 17, 40)                                                           # a short serpentine: both can walk it
    m = np.zeros((40, 40, 40), np.int8)
    L.embed(m, L.serpentine((9, 12, 38)), lo, False)
    a, rounds = L.brute_propagate(m, lo, hi, 6, False, max_rounds=4096)
    assert a.tobytes() == L.brute_flood(m, lo, hi, 6, False).tobytes() and rounds > L.MAX_ROUNDS > 0
    with pytest.raises(AssertionError):
        L.brute_propagate(m, lo, hi, 6, False)                                                 # the bound on the rounds bites


def _axis_boxes():
    t = (8, 8, 64)                                                                             # asserted against the build below
    out = []
    for a in range(3):
        for e in (1, t[a] - 1, t[a], t[a] + 1, 2 * t[a] + 1):
            ext = [9, 10, 11]
            ext[a] = e
            out.append((a, e, tuple(ext)))
    return out


@pytest.mark.parametrize("axis,extent,shape", _axis_boxes())
def test_extents_around_the_tile_edge(axis, extent, shape):
    assert L.tile() == (8, 8, 64)
    m = L.grid("long")
    lo = (3, 5, 6)                                                                             # no multiple of the tile
    hi = tuple(l + s for l, s in zip(lo, shape))
    for conn, empty in ((6, False), (26, False), (18, True)):
        rc, labels, record = L.emul_call(m, lo, hi, conn, empty)
        want = L.reference(m, lo, hi, conn, empty)
        L.check(labels, record, (want, L.record_of(want, m.shape[0], lo)), f"axis {axis} extent {extent} conn {conn} empty {empty}")


def _face_boxes(G):
    out = {"whole": ((0, 0, 0), (G, G, G))}
    for a in range(3):
        for side in (0, 1):
            lo, hi = [7, 9, 5], [7 + 13, 9 + 11, 5 + 17]
            lo[a], hi[a] = (0, 6) if side == 0 else (G - 6, G)
            out[f"{'xyz'[a]}{side}"] = (tuple(lo), tuple(hi))
    return out


@pytest.mark.parametrize("grid,box", [("cube32", b) for b in _face_boxes(32)] + [("small", b) for b in _face_boxes(40)])
def test_grid_faces_and_whole_grids(grid, box):
    """boxes pressed against every face of the grid, and the whole grid: 32^3, and 40^3 whose edge is no power of two"""
    m = L.grid(grid)
    lo, hi = _face_boxes(m.shape[0])[box]
    for conn, empty in ((6, False), (18, False), (26, True)):
        rc, labels, record = L.emul_call(m, lo, hi, conn, empty)
        want = L.reference(m, lo, hi, conn, empty)
        L.check(labels, record, (want, L.record_of(want, m.shape[0], lo)), f"{grid} {box} conn {conn} empty {empty}")


ORDER_CASES = ("full_solid_6", "full_empty_26", "checker_solid_18", "tile_edge_solid_18", "tile_corner_solid_26", "serpentine_solid_6", "serpentine_mirror_empty_6",
               "combs_solid_26", "reenter_solid_6", "random3_solid_6", "random3_empty_18", "random6_solid_26")


@pytest.mark.parametrize("name", ORDER_CASES)
def test_no_order_changes_a_byte(name):
    """the order in which tiles, slots and forward neighbours are visited, shuffled three ways in every phase"""
    c = L.CASES[name]
    for seed in (1, 2, 12345):
        rc, labels, record = L.emul_call(L.grid(c["grid"]), c["lo"], c["hi"], c["conn"], c["empty"], seed=seed)
        L.check(labels, record, L.expected(name), f"{name} seed {seed}")


@pytest.mark.parametrize("name", ORDER_CASES)
def test_stale_loads_change_no_byte(name):
    """the seam phase on a memory whose loads return a randomly chosen EARLIER value of the word (the atomic min sees the truth):
    vrt_label.h's stale-tolerance argument"""
    c = L.CASES[name]
    for seed in (0, 3, 99):
        rc, labels, record = L.emul_call(L.grid(c["grid"]), c["lo"], c["hi"], c["conn"], c["empty"], seed=seed, stale=True)
        L.check(labels, record, L.expected(name), f"{name} stale, seed {seed}")


@pytest.mark.parametrize("name", ["random3_solid_6", "serpentine_solid_6", "full_empty_26", "combs_solid_18"])
def test_the_tile_phase_leaves_tile_roots(name):
    c = L.CASES[name]
    m = L.grid(c["grid"])
    rc, labels, record, mid = L.emul_call(m, c["lo"], c["hi"], c["conn"], c["empty"], after_tiles=True)
    own = L.grid_indices(128, c["lo"], c["hi"])
    member = labels >= 0
    assert ((mid >= 0) == member).all() and (mid[~member] == -1).all()
    assert (mid[member] <= own[member]).all() and (mid[member] >= labels[member]).all()        # L[x] <= x, and never below the component's smallest cell
    at = np.stack(np.unravel_index(mid[member], (128, 128, 128)), -1) - np.array(c["lo"])       # the named cell, box-local
    mine = np.argwhere(member)
    assert (at // np.array(L.tile()) == mine // np.array(L.tile())).all()                      # in the cell's own tile
    assert (labels[tuple(at.T)] == labels[member]).all()                                       # and of its own component
    assert (mid[tuple(at.T)] == mid[member]).all()                                             # and a root there: the tile is flat


def test_host_path_staging_and_the_plan():
    c = L.CASES["random3_solid_18"]
    m = L.grid(c["grid"])
    rc, labels, record = L.emul_call(m, c["lo"], c["hi"], c["conn"], c["empty"], staged=True)
    L.check(labels, record, L.expected("random3_solid_18"), "staged")
    rc, labels, record = L.emul_call(m, c["lo"], c["hi"], c["conn"], c["empty"], want_result=False)
    assert rc == _abi.VRT_OK and record is None and labels.tobytes() == L.expected("random3_solid_18")[0].tobytes()
    nv = labels.size
    assert 16 <= L.emul_plan(nv) <= 256                                                        # "a few counter words"
    assert 4 * nv + 16 <= L.emul_plan(nv, staged=True) <= 4 * nv + 16 + 512                    # "4 bytes per box cell plus 16"
    assert L.emul_plan(256 ** 3, staged=True) >= 4 * 256 ** 3 + 16


def test_forward_neighbours_are_the_later_half():
    for conn, n in ((6, 3), (18, 9), (26, 13)):
        f = L.emul_forward(conn)
        assert len(f) == len(set(f)) == n and all(o > (0, 0, 0) for o in f)                     # lexicographically later
        assert sorted(f + [tuple(-v for v in o) for o in f]) == sorted(L.neighbourhood(conn))   # with their mirror images: the neighbourhood
    assert L.emul_forward(26)[:9] == L.emul_forward(18) and L.emul_forward(18)[:3] == L.emul_forward(6)


def test_export_binding_constants_and_error_codes():
    assert "vrt_label_components" in _lib.exported_symbols()
    hdr = open(L.ROOT + "/include/vrt_api.h").read()
    e = re.search(r"VRT_LABEL_EMPTY = (\d+), VRT_LABEL_CONN_18 = (\d+), VRT_LABEL_CONN_26 = (\d+)", hdr)
    assert tuple(int(v) for v in e.groups()) == (_abi.LABEL_EMPTY, _abi.LABEL_CONN_18, _abi.LABEL_CONN_26) == (1, 2, 4)
    assert _abi.LABEL_RESULT.itemsize == 16 and _abi.LABEL_RESULT.fields["components"][1] == 8
    assert "No counterpart in the reference. */\nenum { VRT_LABEL_EMPTY" in hdr
    hip = _lib.load()
    _abi.declare(hip, "vrt_")
    fn = hip.vrt_label_components
    assert fn.restype is C.c_int and len(fn.argtypes) == 7 and fn.argtypes[3] is C.c_uint32
    out = np.zeros(1, np.int32)
    assert fn(None, (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(1, 1, 1), 0, out.ctypes.data_as(C.c_void_p), None, 0) == _abi.VRT_E_INVALID
    # the entry point's checks, as the emulation repeats them
    m = L.grid("small")
    call = lambda lo=(1, 1, 1), hi=(2, 2, 2), flags=0: L.emul_call(m, lo, hi, flags=flags)[0]
    assert call() == _abi.VRT_OK
    for flags in (1, 2, 3, 4, 5):
        assert call(flags=flags) == _abi.VRT_OK, flags
    for flags in (6, 7, 8, 0x80000000, 0x10):
        assert call(flags=flags) == _abi.VRT_E_INVALID, flags
    for lo, hi in (((2, 1, 1), (1, 2, 2)), ((-1, 0, 0), (0, 1, 1)), ((39, 39, 39), (40, 40, 41))):
        assert call(lo, hi) == _abi.VRT_E_INVALID, (lo, hi)
    for lo, hi in (((5, 5, 5), (5, 9, 9)), ((40, 40, 40), (40, 40, 40))):                      # empty boxes: OK, no label, the record zeroed
        rc, labels, record = L.emul_call(m, lo, hi)
        assert rc == _abi.VRT_OK and labels.size == 0 and record == dict(cells=0, components=0, reserved=0)
    rc, labels, record = L.emul_call(m, (7, 7, 7), (8, 8, 8), empty=not bool(m[7, 7, 7] > 0))   # one cell, a member: its own root
    assert rc == _abi.VRT_OK and labels[0, 0, 0] == (7 * 40 + 7) * 40 + 7 and record == dict(cells=1, components=1, reserved=0)
    rc, labels, record = L.emul_call(m, (7, 7, 7), (8, 8, 8), empty=bool(m[7, 7, 7] > 0))
    assert labels[0, 0, 0] == -1 and record == dict(cells=0, components=0, reserved=0)
