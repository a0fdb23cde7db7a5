"""vrt_voxelize_triangles on the host: the functions of voxel_rt2_amd/csrc/vrt_voxelize.h compiled with g++
(tests/emul/voxelize_emul.cpp runs the loops of the k_vox_* kernels, the lanes of a wave one after the other).
  the predicate against geometry   covers(triangle, cell) == an exact polygon clip in fractions (tests/voxelize.py, exact_covers),
                                   over every cell of the triangle's bounds grown by one, for every family; and the numpy brute force's
                                   own thirteen-axis test against the same clip, so that the expectation is anchored too
  whole calls                      the emulated call on tests/edit.py's HostGrid == the brute force + a rebuild from scratch, word for
                                   word on mat, rgb, texels and l0..l3, and the result record; chunks of 3 triangles and grabs of one
                                   item, so that overlapping pairs straddle chunks; every family at 128 and 256; and the device path's
                                   shape above one batch, batches of 3 resolved once with base 0
  the hierarchy                    a 16^3 cell or a brick that the cube test rejects holds no covered voxel
  the snap                         ties go to even, grid planes land on 64 k, the bound and the non-finite gate
  int64 headroom                   the set-up of the triangle with vertices at the +-8 extremes against Python's unbounded integers
  the boundary                     export, binding, record sizes, and a stand-alone program built with -fsanitize=address,undefined (no
                                   sanitizer runs on code loaded into Python)"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import edit as E
import rays as R
import voxelize as V
from voxel_rt2_amd import _abi, _lib

F = np.float32


def snapped(tris, G):
    return V.snap(V.vertices(tris), G)


def bounds_cells(s, lo, hi, grow=1):
    """every cell of the snapped triangle's bounds grown by `grow`, inside the clip box grown by `grow`"""
    c0 = np.maximum(((s.min(axis=0) - 1) >> 6) - grow, np.array(lo) - grow)
    c1 = np.minimum((s.max(axis=0) >> 6) + grow + 1, np.array(hi) + grow)
    if (c1 <= c0).any():
        return np.zeros((0, 3), np.int64)
    return V.box_cells(c0, c1)


@pytest.mark.parametrize("name,G", V.cases())
def test_predicate_equals_the_exact_clip(name, G):
    covered = 0
    for tris, lo, hi in V.case(name, G)[1]:
        ok = V.valid(tris)
        s = snapped(tris, G)
        seen = set()
        for k in range(len(tris)):
            if not ok[k]:
                assert (V.emul_covers(G, tris[k], np.zeros((2, 3), np.int32)) == -1).all()
                continue
            if s[k].tobytes() in seen:                # (a stack of identical triangles: once)
                continue
            seen.add(s[k].tobytes())
            cells = bounds_cells(s[k], lo, hi)
            got, mine = V.emul_covers(G, tris[k], cells), V.covers(s[k], cells)
            want = np.array([V.exact_covers(s[k], c) for c in cells], bool)
            assert np.array_equal(got == 1, want), f"{name}/{G} triangle {k}: {(got != want).sum()} of {len(cells)} cells differ from the exact clip"
            assert np.array_equal(mine, want), f"{name}/{G} triangle {k}: the brute force's own test differs from the exact clip"
            covered += int(want.sum())
    assert covered > 0


def test_points_cover_eight_four_two_one_cells():
    for G in (128, 256):
        tris, lo, hi = V.case("points", G)[1][0]
        for k, n in enumerate(V.POINT_CELLS):
            assert int(V.emul_covers(G, tris[k], V.box_cells(lo, hi)).sum()) == n


def check_whole(name, G, chunk, grab, once=False):
    base, calls = V.case(name, G)
    grid = E.HostGrid(*R.scene(base)[:2])
    for (tris, lo, hi), (mat, rgb, res) in zip(calls, V.states(name, G)[1:]):
        rc, got = V.emul_call(grid, tris, lo, hi, chunk, grab, once)
        assert rc == 0
        assert V.same_result(got, res), f"{name}/{G}: result {got} != {res}"
        assert grid.mat.tobytes() == mat.tobytes() and grid.rgb.tobytes() == rgb.tobytes(), f"{name}/{G}: {(grid.mat != mat).sum()} materials differ"
        want = E.rebuild(mat, rgb)
        for k in ("grid", "l0", "l1", "l2", "l3"):
            assert grid.derived[k].tobytes() == want[k].tobytes(), f"{name}/{G}: {k} differs from the rebuild"
    return V.states(name, G)[-1][2]


@pytest.mark.parametrize("name,G", [c for c in V.cases() if c[1] == 128])
def test_emulated_call_equals_brute_force_128(name, G):
    res = check_whole(name, G, 3, 1)
    if name not in ("carve_last",):
        assert res["voxels"] > 0, "the comparison would pass trivially"


@pytest.mark.parametrize("name,G", [c for c in V.cases() if c[1] == 256])
def test_emulated_call_equals_brute_force_256(name, G):
    assert check_whole(name, G, 3, 1)["voxels"] > 0


@pytest.mark.parametrize("name,G", [("stack", 128), ("stack_reversed", 128), ("invalid", 128), ("cube12", 128), ("carve_last", 128), ("ico_dense", 128), ("ico_s1_256", 256)])
def test_batches_resolved_once_equal_brute_force(name, G):
    """The device path with n above a batch: batches (here of 3 triangles) only raise owners, numbered base + index + 1, and ONE resolve with
    base 0 reads the payloads from the whole array -- an owner of the first batch and one of the last are resolved by the same pass."""
    check_whole(name, G, 3, 1, once=True)
    check_whole(name, G, 2, 64, once=True)


@pytest.mark.parametrize("name", ["stack", "stack_reversed", "invalid", "ico_sunlit", "cube12"])
def test_chunk_and_grab_sizes_change_no_byte(name):
    tris, lo, hi = V.case(name, 128)[1][0]
    ref = E.HostGrid(*R.scene(V.case(name, 128)[0])[:2])
    r0 = V.emul_call(ref, tris, lo, hi)[1]
    for chunk, grab in ((1, 1), (2, 64), (3, 8), (19, 5)):
        for once in (False, True):
            g = E.HostGrid(*R.scene(V.case(name, 128)[0])[:2])
            r = V.emul_call(g, tris, lo, hi, chunk, grab, once)[1]
            assert V.same_result(r, r0) and g.mat.tobytes() == ref.mat.tobytes() and g.rgb.tobytes() == ref.rgb.tobytes(), (chunk, grab, once)


def test_stack_highest_index_wins_and_carve_empties_the_grid():
    for name, top in (("stack", 4), ("stack_reversed", 4)):
        tris = V.case(name, 128)[1][0][0]
        mat, rgb, res = V.states(name, 128)[1]
        p = int(tris["voxel"][top])
        w = mat != R.scene("sunlit")[0]
        assert w.any() and set(np.unique(mat[w]).tolist()) == {np.int8(p >> 24)}
    mats = [s[0] for s in V.states("carve_last", 128)]
    assert (mats[0] > 0).sum() == 1 and (mats[1] > 0).sum() == 0 and (mats[2] > 0).sum() == 1 and mats[2][70, 66, 61] == 11


@pytest.mark.parametrize("name,G", [("huge", 128), ("sliver", 128), ("ico_sunlit", 128), ("in_plane", 256), ("segments", 256)])
def test_rejected_cubes_hold_no_covered_voxel(name, G):
    """vox_cube at edge 16 and 4 against edge 1: every covered voxel lies in a brick and a 16^3 cell that are met."""
    tris, lo, hi = V.case(name, G)[1][0]
    cells = V.box_cells(lo, hi)
    for k in np.flatnonzero(V.valid(tris)):
        hit = cells[V.emul_covers(G, tris[k], cells) == 1]
        for shift in (2, 4):
            parents = np.unique(hit >> shift, axis=0)
            assert (V.emul_covers(G, tris[k], parents, shift) == 1).all()
            # and the cube test at that edge is the same predicate on a larger cube
            some = np.unique(cells >> shift, axis=0)
            s = snapped(tris, G)[k]
            assert np.array_equal(V.emul_covers(G, tris[k], some, shift) == 1, V.covers(s, some, 64 << shift))


def test_snap_ties_planes_and_the_gate():
    lib = V.lib()
    for G in (128, 256):
        p = np.arange(G + 1, dtype=F) * F(2.0 / G) - F(1.0)
        assert [lib.vox_emul_snap(float(x), G) for x in p] == [64 * k for k in range(G + 1)]
        assert np.array_equal(V.snap(p, G), 64 * np.arange(G + 1))
        # ties: w with (w + 1) * (G / 2) * 64 = k + 0.5 exactly, k small enough for binary32 to hold the half
        for k in (-3, -2, -1, 0, 1, 2, 3, 4, 101, 102, 8190, 8191):
            w = F((k + 0.5) / (32.0 * G) - 1.0)
            assert (float(w) + 1.0) * 32.0 * G == k + 0.5                                     # exact in binary32
            want = k if k % 2 == 0 else k + 1
            assert lib.vox_emul_snap(float(w), G) == want == int(V.snap(w, G)), (G, k)
        assert lib.vox_emul_snap(8.0, G) == 9 * (G // 2) * 64 and lib.vox_emul_snap(-8.0, G) == -7 * (G // 2) * 64
    assert 9 * 128 * 64 == 73728 < 2 ** 17
    t = V.triangles(128, [[(1, 2, 3), (4, 5, 6), (7, 8, 10)]])
    assert lib.vox_emul_valid(t.ctypes.data_as(C.c_void_p)) == 1
    for field in ("v0", "v1", "v2"):
        for a in range(3):
            for bad in (np.nan, np.inf, -np.inf, np.nextafter(F(8.0), F(9.0)), np.nextafter(F(-8.0), F(-9.0)), F(1e30)):
                u = t.copy()
                u[field][0, a] = bad
                assert lib.vox_emul_valid(u.ctypes.data_as(C.c_void_p)) == 0 and not V.valid(u)[0]
            for good in (8.0, -8.0, -0.0, 1e-40):
                u = t.copy()
                u[field][0, a] = good
                assert lib.vox_emul_valid(u.ctypes.data_as(C.c_void_p)) == 1 and V.valid(u)[0]
    for field in ("reserved0", "reserved1"):
        u = t.copy()
        u[field] = 1
        assert lib.vox_emul_valid(u.ctypes.data_as(C.c_void_p)) == 0 and not V.valid(u)[0]
        assert V.emul_call(E.HostGrid(*R.scene("one_voxel")[:2]), u, (0, 0, 0), (4, 4, 4))[0] == -1


def test_int64_headroom_at_the_extremes():
    """Every intermediate of the set-up, for triangles with all vertices at (+-8, +-8, +-8), against Python's unbounded integers."""
    corners = [(x, y, z) for x in (-8.0, 8.0) for y in (-8.0, 8.0) for z in (-8.0, 8.0)]
    worst = 0
    for G in (128, 256):
        for i, j, k in ((0, 7, 5), (0, 3, 5), (1, 6, 4), (7, 0, 2), (2, 5, 7), (6, 1, 3), (0, 7, 7)):
            t = np.zeros(1, V.TRI)
            t["v0"], t["v1"], t["v2"] = corners[i], corners[j], corners[k]
            got = [int(x) for x in V.emul_setup(G, t)]
            v = [[int(x) for x in row] for row in V.snap(V.vertices(t), G)[0]]
            e = [[v[(i + 1) % 3][a] - v[i][a] for a in range(3)] for i in range(3)]
            cross = lambda p, q: [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]
            dot = lambda p, q: sum(x * y for x, y in zip(p, q))
            want = [x for row in v for x in row] + [min(r[a] for r in v) for a in range(3)] + [max(r[a] for r in v) for a in range(3)]
            n = cross(e[0], e[1])
            pr = [dot(n, r) for r in v]
            want += n + [min(pr), max(pr), sum(x for x in n if x < 0), sum(x for x in n if x > 0)]
            for i_ in range(3):
                for a in range(3):
                    ax = cross(e[i_], [int(a == b) for b in range(3)])
                    pr = [dot(ax, r) for r in v]
                    want += ax + [min(pr), max(pr), sum(x for x in ax if x < 0), sum(x for x in ax if x > 0)]
            assert got == want, (G, i, j, k)
            assert max(abs(x) for x in want) < 2 ** 56
            # the projections of the grid's far corner cell, the largest the cube test forms
            far = (n[0] * G + n[1] * G + n[2] * G + sum(x for x in n if x > 0)) * 64
            assert abs(far) < 2 ** 56
            worst = max(worst, max(abs(x) for x in want))
    assert worst > 2 ** 49                            # (the case is an extreme one: int32 or a double's 53 bits would not do for long)


def test_boundary_export_binding_and_sizes():
    lib = V.lib()
    assert (lib.vox_emul_sizes(0), lib.vox_emul_sizes(1), lib.vox_emul_sizes(2)) == (V.TRI.itemsize, V.RESULT.itemsize, 16) == (48, 40, 16)
    assert lib.vox_emul_plan(0) == 1 << 18 and lib.vox_emul_plan(1) == 1 << 20 and lib.vox_emul_plan(2) == 4
    assert "vrt_voxelize_triangles" in _lib.exported_symbols()
    hip = _lib.load()
    _abi.declare(hip, "vrt_")
    assert hip.vrt_voxelize_triangles.argtypes is not None and len(hip.vrt_voxelize_triangles.argtypes) == 7
    t = np.zeros(1, V.TRI)
    assert hip.vrt_voxelize_triangles(None, 1, t.ctypes.data_as(C.c_void_p), (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(1, 1, 1), None, 0) == _abi.VRT_E_INVALID


def test_standalone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "voxelize_emul_asan")
    build = subprocess.run(V.GCC[:1] + ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DVOX_EMUL_MAIN", "-Wno-unknown-pragmas",
                                        "-o", exe, V._SRC], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-3000:]
    assert run.stdout.startswith("ok:")
