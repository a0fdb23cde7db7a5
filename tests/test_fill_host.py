"""vrt_fill_triangles on the host: the functions of voxel_rt2_amd/csrc/vrt_fill.h compiled with g++ (tests/emul/fill_emul.cpp runs
the loops of the k_fill_* kernels, the lanes of a wave one after the other).
  the predicate against geometry   fill_column_in / fill_first_cell == plain strict tests in fractions at q + (eps, eps^2, eps^3),
                                   eps = 2^-80 (tests/fill.py says why that is small enough), for every triangle of every family
                                   and every cell of its bounds grown by one; the numpy brute force's own cascade against the same
                                   tests, so that the expectation is anchored too
  whole calls                      the emulated call on tests/edit.py's HostGrid == the brute force + a rebuild from scratch, word for
                                   word on mat, rgb, texels and l0..l3, and the result record; batches of 3 triangles and grabs of one
                                   item; every family at 128 and 256; chunk and grab sizes change no byte
  what the families promise        reversed / mixed orientation and two half boxes == the icosphere's grid; duplicated, flat, below
                                   and above write nothing; nested spheres are hollow; carving empties
  geometric sanity                 for the convex closed meshes a cell whose centre is strictly inside is filled, strictly outside not
  int64 headroom                   set-up, edge functions and first cells of triangles with vertices at the +-8 extremes against
                                   Python's unbounded integers
  the boundary                     export, binding, plan constants, and a stand-alone program built with -fsanitize=address,undefined
                                   (no sanitizer runs on code loaded into Python)"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import edit as E
import fill as FL
import rays as R
import voxelize as V
from voxel_rt2_amd import _abi, _lib


def columns_grown(s, grow=1):
    """every column of the snapped triangle's xy bounds grown by `grow`"""
    c0 = ((s[:, :2].min(axis=0) - 1) >> 6) - grow
    c1 = (s[:, :2].max(axis=0) >> 6) + grow + 1
    return np.stack(np.meshgrid(np.arange(c0[0], c1[0]), np.arange(c0[1], c1[1]), indexing="ij"), axis=-1).reshape(-1, 2), (c0, c1)


@pytest.mark.parametrize("name", FL.GENERIC)
def test_predicate_equals_strict_tests_at_the_perturbed_point(name):
    """Per column the exact crossing height (or a miss), and from it the exact first cell; then EVERY cell of the bounds grown by one:
    crossed below iff the column is in and cz >= the first cell -- for the header's functions and for the brute force's cascade."""
    G = 128
    owned, seen = 0, set()
    for tris, lo, hi, _ in FL.case(name, G)[1]:
        ok = V.valid(tris)
        snapped = V.snap(V.vertices(tris), G)
        for k in range(len(tris)):
            s = snapped[k]
            if not ok[k]:
                assert (FL.emul_columns(G, tris[k], np.zeros((2, 2), np.int32))[0] == -1).all()
                continue
            if s.tobytes() in seen:
                continue
            seen.add(s.tobytes())
            cols, (c0, c1) = columns_grown(s)
            z0, z1 = int((s[:, 2].min() - 1) >> 6) - 1, int(s[:, 2].max() >> 6) + 2
            inn, first = FL.emul_columns(G, tris[k], cols)
            mine = FL.crosses_below(s, (int(c0[0]), int(c0[1]), z0), (int(c1[0]), int(c1[1]), z1)).reshape(len(cols), z1 - z0)
            cz = np.arange(z0, z1)
            for i, (cx, cy) in enumerate(cols):
                h = FL.exact_crossing(s, int(cx), int(cy))
                assert (h is not None) == bool(inn[i]), f"{name} triangle {k} column {(cx, cy)}: in = {inn[i]}, exactly {h}"
                want = np.zeros(len(cz), bool) if h is None else cz >= FL.exact_first_cell(h)
                if h is not None:
                    assert int(first[i]) == FL.exact_first_cell(h), f"{name} triangle {k} column {(cx, cy)}: first cell {first[i]}, exactly {FL.exact_first_cell(h)}"
                    owned += 1
                assert np.array_equal(mine[i], want), f"{name} triangle {k} column {(cx, cy)}: the brute force's cascade differs from the strict tests"
    assert owned > 0


def test_ties_occur_in_the_families_that_promise_them():
    """cube_centres, tetra_centres and fan_apex are there for E == 0 and F == 0: count them."""
    G = 128
    for name, want_e, want_f in (("cube_centres", True, True), ("tetra_centres", True, False), ("fan_apex", True, True)):
        tris, lo, hi, _ = FL.case(name, G)[1][0]
        e_ties = f_ties = 0
        for s in V.snap(V.vertices(tris), G):
            n = np.cross(s[1] - s[0], s[2] - s[1])
            cols, _ = columns_grown(s, 0)
            q = 64 * cols + 32
            for p, r in ((s[0], s[1]), (s[1], s[2]), (s[2], s[0])):
                d = r - p
                e_ties += int(((d[0] * (q[:, 1] - p[1]) - d[1] * (q[:, 0] - p[0])) == 0).sum())
            if n[2] != 0:
                for cz in range(int(s[:, 2].min() >> 6), int(s[:, 2].max() >> 6) + 1):
                    f_ties += int(((n[0] * (q[:, 0] - s[0][0]) + n[1] * (q[:, 1] - s[0][1]) + n[2] * (64 * cz + 32 - s[0][2])) == 0).sum())
        assert (e_ties > 0) >= want_e and (f_ties > 0) >= want_f, (name, e_ties, f_ties)


def check_whole(name, G, chunk, grab):
    base, calls = FL.case(name, G)
    grid = E.HostGrid(*R.scene(base)[:2])
    for (tris, lo, hi, voxel), (mat, rgb, res) in zip(calls, FL.states(name, G)[1:]):
        rc, got = FL.emul_call(grid, tris, lo, hi, voxel, chunk, grab)
        assert rc == 0
        assert FL.same_result(got, res), f"{name}/{G}: result {got} != {res}"
        assert grid.mat.tobytes() == mat.tobytes() and grid.rgb.tobytes() == rgb.tobytes(), f"{name}/{G}: {(grid.mat != mat).sum()} materials differ"
        want = E.rebuild(mat, rgb)
        for k in ("grid", "l0", "l1", "l2", "l3"):
            assert grid.derived[k].tobytes() == want[k].tobytes(), f"{name}/{G}: {k} differs from the rebuild"
    return FL.states(name, G)[-1][2]


@pytest.mark.parametrize("name,G", FL.cases())
def test_emulated_call_equals_brute_force(name, G):
    res = check_whole(name, G, 3, 1)
    assert (res["voxels"] == 0) == (name in FL.NOTHING), "the comparison would pass trivially"


@pytest.mark.parametrize("name", ["icosphere", "cube_centres", "invalid", "torus", "poke"])
def test_chunk_and_grab_sizes_change_no_byte(name):
    tris, lo, hi, voxel = FL.case(name, 128)[1][0]
    ref = E.HostGrid(*R.scene(FL.case(name, 128)[0])[:2])
    r0 = FL.emul_call(ref, tris, lo, hi, voxel)[1]
    assert FL.same_result(r0, FL.states(name, 128)[1][2])
    for chunk, grab in ((1, 1), (2, 64), (3, 8), (19, 5), (len(tris) - 1, 3)):
        g = E.HostGrid(*R.scene(FL.case(name, 128)[0])[:2])
        r = FL.emul_call(g, tris, lo, hi, voxel, chunk, grab)[1]
        assert FL.same_result(r, r0) and g.mat.tobytes() == ref.mat.tobytes() and g.rgb.tobytes() == ref.rgb.tobytes(), (chunk, grab)
    shuffled = tris[np.random.default_rng(5).permutation(len(tris))]                                       # nor does the triangles' order
    g = E.HostGrid(*R.scene(FL.case(name, 128)[0])[:2])
    assert FL.same_result(FL.emul_call(g, shuffled, lo, hi, voxel, 7, 2)[1], r0) and g.mat.tobytes() == ref.mat.tobytes()


@pytest.mark.parametrize("G", [128, 256])
def test_what_the_families_promise(G):
    ico = FL.states("icosphere", G)[-1]
    base = R.scene(FL.case("icosphere", G)[0])
    assert ico[2]["voxels"] > 3000
    for name in FL.SAME_AS_ICOSPHERE:                 # orientation does not matter; two half boxes are the whole box
        mat, rgb, res = FL.states(name, G)[-1]
        assert mat.tobytes() == ico[0].tobytes() and rgb.tobytes() == ico[1].tobytes(), name
        if name != "halves":
            assert FL.same_result(res, ico[2])
    h = FL.states("halves", G)
    assert h[1][2]["voxels"] + h[2][2]["voxels"] == ico[2]["voxels"] and h[1][2]["voxels"] > 0 and h[2][2]["voxels"] > 0
    for name in FL.NOTHING:
        mat, rgb, res = FL.states(name, G)[-1]
        assert mat.tobytes() == base[0].tobytes() and rgb.tobytes() == base[1].tobytes() and not res.tobytes().strip(b"\0"), name
    o = FL.origin(G)
    nested = FL.states("nested", G)[-1][0]
    assert nested[o + 16, o + 15, o + 16] == base[0][o + 16, o + 15, o + 16] and nested[o + 16, o + 15, o + 26] == 11 and ico[0][o + 16, o + 15, o + 16] == 11
    assert FL.states("invalid", G)[-1][2]["invalid"] == 1
    block, carved = FL.states("carve", G)[1:]
    assert (block[0][o + 3:o + 29, o + 4:o + 28, o + 5:o + 27] == 21).all() and block[2]["voxels"] == 26 * 24 * 22
    assert carved[2]["voxels"] > 1000 and (carved[0] == 21).sum() == (block[0] == 21).sum() - carved[2]["voxels"] and (carved[0] != block[0]).sum() == carved[2]["voxels"]
    assert (FL.states("negative", G)[-1][0] == -5).sum() == FL.states("negative", G)[-1][2]["voxels"] > 0
    # the cube on grid planes is exactly its index box; the one through cell centres is half-open: [entry, exit) on every axis
    # (the perturbation moves a centre towards +x, +y, +z: on a low face it is inside, on a high face outside) -- the same cells
    want = base[0].copy()
    want[o + 6:o + 19, o + 9:o + 25, o + 5:o + 22] = 11
    for name in ("cube_planes", "cube_centres"):
        mat, _, res = FL.states(name, G)[-1]
        assert mat.tobytes() == want.tobytes(), name
        assert res["voxels"] == 13 * 16 * 17 and res["lo"].tolist() == [o + 6, o + 9, o + 5] and res["hi"].tolist() == [o + 19, o + 25, o + 22], (name, res)


@pytest.mark.parametrize("name", FL.CONVEX)
def test_convex_meshes_fill_what_is_strictly_inside_and_nothing_strictly_outside(name):
    """Independent of the cascade: centres against the face planes of a convex polyhedron, in integers."""
    G = 128
    tris, lo, hi, _ = FL.case(name, G)[1][0]
    cells = V.box_cells(lo, hi)
    strictly_in, strictly_out = FL.convex_sides(V.snap(V.vertices(tris), G), cells)
    filled = FL.inside(tris, G, lo, hi).reshape(-1)
    assert strictly_in.sum() > 500 and strictly_out.sum() > 500
    assert filled[strictly_in].all(), f"{name}: {(~filled[strictly_in]).sum()} cells strictly inside are not filled"
    assert not filled[strictly_out].any(), f"{name}: {filled[strictly_out].sum()} cells strictly outside are filled"
    if name in ("cube_centres", "tetra_centres", "fan_apex"):
        assert (~strictly_in & ~strictly_out).sum() > 0                                                    # centres ON the surface: the ties decide those


def _py_setup(v):
    """the set-up record in Python's unbounded integers, in fill_emul_setup's order"""
    sign = lambda x: (x > 0) - (x < 0)
    e0, e1 = [v[1][a] - v[0][a] for a in range(3)], [v[2][a] - v[1][a] for a in range(3)]
    n = [e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]]
    sg = sign(n[2])
    out = [x for p in v for x in p] + [min(p[a] for p in v) for a in range(3)] + [max(p[a] for p in v) for a in range(3)] + n + [sg]
    for i in range(3):
        p, r = v[i], v[(i + 1) % 3]
        dx, dy = r[0] - p[0], r[1] - p[1]
        tie = -sign(dy) if dy else sign(dx)
        out += [sg * dx, sg * dy, sg * (dx * (32 - p[1]) - dy * (32 - p[0])), int(sg * tie > 0)]
    ftie = next((sign(x) for x in n if x), 0)
    out += [sg * n[0], sg * n[1], sg * sum(n[a] * (32 - v[0][a]) for a in range(3)), 64 * sg * n[2], int(sg * ftie > 0)]
    return out, n, sg


def test_int64_headroom_at_the_extremes():
    """Triangles with vertices at (+-8, +-8, +-8) at grid 256, and nearly edge-on ones whose n_z is tiny so that the first cell is
    astronomically far away: the set-up, the edge functions and the first cell against Python's unbounded integers."""
    G = 256
    sign = lambda x: (x > 0) - (x < 0)
    corners = [(x, y, z) for x in (-8.0, 8.0) for y in (-8.0, 8.0) for z in (-8.0, 8.0)]
    tris = []
    for i, j, k in ((0, 6, 5), (0, 3, 5), (1, 6, 4), (7, 0, 2), (2, 5, 7), (6, 1, 3), (4, 2, 1)):
        t = np.zeros(1, V.TRI)
        t["v0"], t["v1"], t["v2"] = corners[i], corners[j], corners[k]
        tris.append(t)
    step = 1.0 / (64 * 128)                                                                                    # one snapped unit at grid 256
    for dz in (8.0, -8.0):                                                                                     # n_z = +-1 snapped unit^2 ... the steepest plane there is
        t = np.zeros(1, V.TRI)
        t["v0"], t["v1"], t["v2"] = (-8, -8, -dz), (-8 + step, -8, dz), (-8, -8 + step, -dz)
        tris.append(t)
    worst_f = worst_first = 0
    cols = np.array([(cx, cy) for cx in (-897, -896, -1, 0, 127, 255, 1151, 1152) for cy in (-897, -896, 0, 128, 255, 1151, 1152)], np.int32)
    for t in tris:
        v = [[int(x) for x in row] for row in V.snap(V.vertices(t), G)[0]]
        want, n, sg = _py_setup(v)
        assert [int(x) for x in FL.emul_setup(G, t)] == want
        assert max(abs(x) for x in want) < 2 ** 56
        inn, first = FL.emul_columns(G, t, cols)
        for i, (cx, cy) in enumerate(cols.tolist()):
            qx, qy = 64 * cx + 32, 64 * cy + 32
            col_in = sg != 0
            for a in range(3):
                p, r = v[a], v[(a + 1) % 3]
                d = (r[0] - p[0], r[1] - p[1])
                e = d[0] * (qy - p[1]) - d[1] * (qx - p[0])
                assert abs(e) < 2 ** 37
                col_in = col_in and sg * next((sign(x) for x in (e, -d[1], d[0]) if x), 0) > 0
            assert bool(inn[i]) == col_in, (v, cx, cy)
            if col_in:
                crossed = lambda cz: sg * next(sign(x) for x in (n[0] * (qx - v[0][0]) + n[1] * (qy - v[0][1]) + n[2] * (64 * cz + 32 - v[0][2]), n[0], n[1], n[2]) if x) > 0
                f = int(first[i])
                assert crossed(f) and not crossed(f - 1), (v, cx, cy, f)
                worst_first = max(worst_first, abs(f))
                worst_f = max(worst_f, abs(n[0] * (qx - v[0][0]) + n[1] * (qy - v[0][1])))
    assert worst_f > 2 ** 49 and worst_first > 2 ** 9                                                          # (the cases are extreme ones)


def test_cells_tiles_prefix_and_toggle_layout():
    G = 128
    o = FL.origin(G)
    lo, hi = FL.default_box(G)
    # a triangle over columns o+3 .. o+20 / o+4 .. o+9 (centres within the closed bounds), one wholly above, one edge-on, one beside
    t = FL.mesh(G, [[(o + 3.5, o + 4.5, o + 6), (o + 20.5, o + 4.5, o + 6), (o + 3.5, o + 9.5, o + 8)]])
    c = FL.emul_cells(G, t[0], lo, hi)
    assert c[:4].tolist() == [o + 3, o + 4, 18, 6] and c[4:8].tolist() == [(o + 3) >> 4, (o + 4) >> 4, ((o + 20) >> 4) - ((o + 3) >> 4) + 1, 1] and c[8] == c[6] * c[7]
    above = FL.mesh(G, [[(o + 3.5, o + 4.5, o + 40.75), (o + 20.5, o + 4.5, o + 41), (o + 3.5, o + 9.5, o + 42)]])
    edge_on = FL.mesh(G, [[(o + 3.5, o + 4.5, o + 6), (o + 20.5, o + 4.5, o + 6), (o + 3.5, o + 4.5, o + 18)]])
    beside = FL.mesh(G, [[(o - 30, o + 4.5, o + 6), (o - 10, o + 4.5, o + 6), (o - 20, o + 9.5, o + 8)]])
    for u in (above, edge_on, beside):
        assert FL.emul_cells(G, u[0], lo, hi)[8] == 0
    below = FL.mesh(G, [[(o + 3.5, o + 4.5, o - 40), (o + 20.5, o + 4.5, o - 41), (o + 3.5, o + 9.5, o - 42)]])
    assert FL.emul_cells(G, below[0], lo, hi)[8] == c[8]                                                    # below the box: keeps its columns
    span = np.zeros(1, V.TRI)
    span["v0"], span["v1"], span["v2"] = (-3, -3, 0), (3, -3, 0), (0, 4, 0.1)
    assert FL.emul_cells(256, span[0], (0, 0, 0), (256, 256, 256))[8] == 256                               # a grid-spanning triangle: 16 x 16 items
    rng = np.random.default_rng(11)
    w = rng.integers(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32)
    w[3], w[4] = 0, 0x80000000
    bits = np.unpackbits(w.view(np.uint8), bitorder="little")
    got = w.copy()
    FL.lib().fill_emul_prefix(len(got), got.ctypes.data_as(C.c_void_p))
    assert np.array_equal(np.unpackbits(got.view(np.uint8), bitorder="little"), np.bitwise_xor.accumulate(bits))


def test_boundary_export_binding_and_plan():
    lib = FL.lib()
    assert lib.fill_emul_plan(0) == 1 << 18 and lib.fill_emul_plan(1) == 1 << 20 and lib.fill_emul_plan(2) >= 1
    assert "vrt_fill_triangles" in _lib.exported_symbols()
    hip = _lib.load()
    _abi.declare(hip, "vrt_")
    assert hip.vrt_fill_triangles.restype is C.c_int and len(hip.vrt_fill_triangles.argtypes) == 8 and hip.vrt_fill_triangles.argtypes[5] is C.c_uint32
    t = np.zeros(1, V.TRI)
    assert hip.vrt_fill_triangles(None, 1, t.ctypes.data_as(C.c_void_p), (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(1, 1, 1), 0, None, 0) == _abi.VRT_E_INVALID
    bad = FL.mesh(128, [[(1, 2, 3), (4, 5, 6), (7, 8, 10)]])
    bad["reserved1"] = 1
    assert FL.emul_call(E.HostGrid(*R.scene("one_voxel")[:2]), bad, (0, 0, 0), (4, 4, 4), FL.PAY)[0] == -1


def test_standalone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "fill_emul_asan")
    build = subprocess.run(V.GCC[:1] + ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DFILL_EMUL_MAIN", "-Wno-unknown-pragmas",
                                        "-o", exe, FL._SRC], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-3000:]
    assert run.stdout.startswith("ok:")
