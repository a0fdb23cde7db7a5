"""vrt_move_voxels WITHOUT a GPU: the host build of voxel_rt2_amd/csrc/vrt_move.h (tests/emul/move_emul.cpp runs the kernels' loops and
the call's passes in their order) against the brute forces of tests/move.py, byte for byte over every voxel of the grid, plus the record:
  every case           identity, translations (one overlapping its source), the 24 axis rotations about integer and half-integer pivots,
                       a mirror, 30 degrees about each axis, a shear, scale 2 and 1/2, the zero matrix, coefficients at the +-2^20 and
                       +-2^40 bounds; destination boxes tight, whole grid, cut at a grid face, missing the image, empty; selections
                       NULL, a label root, a value no cell holds, a checkerboard; all 16 flag combinations on a blocked and on a free
                       placement; negative material bytes in source and destination; one case at 256^3
  independent anchors  the 24 rotations == transposes and flips placed by hand (np.rot90 among them); translations == np.roll;
                       a copy, then the copy by the inverse rotation, restores what was cleared in between
  the arithmetic       the z step == the full map on every cell of a line, at the bounds too; the two brute forces agree
  the facade           move_transform and moved_box against hand-computed values
  the boundary         error codes, export, binding, record sizes, and a stand-alone program built with -fsanitize=address,undefined
                       (no sanitizer runs on code loaded into Python)"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import move as M
from voxel_rt2_amd import _abi, _lib


@pytest.mark.parametrize("name", M.NAMES_128 + (M.CASE_256,))
def test_emulated_call_equals_brute_force(name):
    c = M.case(name)
    mat, rgb = M.grid(c["grid"])
    sel = M.select_of(name)[0]
    want = M.expected(name)
    for staged in ((False, True) if sel is not None and name != M.CASE_256 else (False,)):
        rc, m, col, rec = M.emul_call(mat, rgb, c, sel, staged)
        assert rc == 0
        M.check(m, col, rec, want, f"{name} staged={staged}")


def test_what_the_cases_promise():
    """the case table holds what its names say: blocked and free placements, cut and missed images, lost voxels under a 30 degree turn"""
    for name in M.FLAG_NAMES:
        rec = M.expected(name)[2]
        assert (rec["blocked"] > 0) == name.endswith("_blocked"), (name, rec)
        flags = M.CASES[name]["flags"]
        if flags & M.IF_FREE and rec["blocked"]:
            assert rec["written"] == rec["erased"] == 0 and rec["hi"] == (0, 0, 0)
        elif not flags & M.KEEP:
            assert rec["written"] > 0
        assert (rec["erased"] > 0) == bool(flags & M.ERASE and not (flags & M.IF_FREE and rec["blocked"])), (name, rec)
        changed = M.expected(name)[0].tobytes() != M.grid("clutter")[0].tobytes()
        assert changed == (not flags & M.DRY and not (flags & M.IF_FREE and rec["blocked"])), name
    pieces = int((M.grid("clutter")[0][tuple(slice(l, h) for l, h in zip(*M.SRC))] > 0).sum())
    assert pieces > 80
    for name in M.ROTATION_NAMES + ("mirror", "shift_far", "shift_overlap", "identity_tight"):       # exact permutations
        rec = M.expected(name)[2]
        assert rec["written"] == rec["erased"] == pieces, (name, rec)
    assert 0 < M.expected("dst_cut_at_face")[2]["written"] < pieces and M.expected("dst_cut_at_face")[2]["erased"] == pieces
    for name in ("dst_missing", "dst_empty", "shift_off", "zero_miss", "select_nobody_shift"):
        rec = M.expected(name)[2]
        assert rec["written"] == 0 and rec["erased"] == (0 if name == "select_nobody_shift" else pieces), (name, rec)
    assert M.expected("src_empty")[2] == dict(lo=(0, 0, 0), hi=(0, 0, 0), written=0, blocked=0, erased=0)
    assert M.expected("zero_hit")[2]["written"] == 4 * 3 * 5 and M.grid("clutter")[0][63, 15, 4] > 0
    for a in "xyz":                                                                         # nearest-neighbour resampling loses and doubles voxels
        rec = M.expected(f"turn30_{a}")[2]
        assert rec["erased"] == pieces and 0.8 * pieces < rec["written"] < 1.2 * pieces, rec
    assert M.expected("scale_2")[2]["written"] > 6 * pieces and M.expected("bound_m_hit")[2]["written"] >= 1
    src = M.grid("clutter")[0][tuple(slice(l, h) for l, h in zip(*M.SRC))]
    assert (src < 0).any() and (M.grid("clutter")[0][64:72, 14:22, 3:9] < 0).any()          # negative bytes in the source and where pieces land
    root, value = M.select_of("select_root_shift")
    assert 1 < (root == value).sum() < (root >= 0).sum()


def test_the_two_brute_forces_agree():
    for name in M.BOUND_NAMES + ("shift_overlap", "rot10_int", "turn30_x", "shear", "flags03_blocked", "flags11_blocked", "select_checker_turn", "dst_cut_at_face"):
        c = M.case(name)
        if np.prod([h - l for l, h in zip(*c["dst"])]) > 200000:
            c["dst"] = ((50, 0, 0), (80, 40, 20))
        got = M.brute_py(*M.grid(c["grid"]), c, M.select_of(name)[0])
        want = M.brute(*M.grid(c["grid"]), c, M.select_of(name)[0])
        M.check(got[0], got[1], got[2], want, name)


# ---- independent anchors ------------------------------------------------------------------------------------------------------------------
def _by_hand(A, R):
    """the block A turned about its own centre by the signed permutation matrix R: axes permuted, then flipped"""
    perm = [int(np.flatnonzero(R[i])[0]) for i in range(3)]
    B = np.transpose(A, perm + list(range(3, A.ndim)))
    for i in range(3):
        if R[i, perm[i]] < 0:
            B = np.flip(B, axis=i)
    return B


def test_by_hand_is_rot90_about_the_coordinate_axes():
    A = np.arange(5 * 5 * 5).reshape(5, 5, 5)
    seen = 0
    for R in M.rotations24():
        for axes, turn in (((0, 1), M.rot("z", 90)), ((1, 2), M.rot("x", 90)), ((2, 0), M.rot("y", 90))):
            for k in range(4):
                if np.array_equal(np.rint(np.linalg.matrix_power(turn, k)).astype(int), R):
                    assert np.array_equal(_by_hand(A, R), np.rot90(A, k, axes)), (R, axes, k)
                    seen += 1
    assert seen == 3 * 4


@pytest.mark.parametrize("n", [7, 6])
def test_axis_rotations_equal_blocks_placed_by_hand(n):
    """a cube of n^3 cells turned about its own centre (half-integer for odd n, integer for even) lands on itself"""
    mat, rgb = M.grid("clutter")
    lo = (60, 12, 1)
    box = (lo, tuple(v + n for v in lo))
    sl = tuple(slice(l, h) for l, h in zip(*box))
    A, Ac, P = mat[sl], rgb[sl], mat[sl] > 0
    for R in M.rotations24():
        m, t = M.inverse_exact(R, [2 * l + n for l in lo])
        rc, got_m, got_c, rec = M.emul_call(mat, rgb, M._case("clutter", box, box, m, t, M.ERASE) | dict(value=0))
        want_m, want_c = mat.copy(), rgb.copy()
        rP = _by_hand(P, R)
        want_m[sl] = np.where(rP, _by_hand(A, R), np.where(P, 0, A))
        want_c[sl] = np.where(rP[..., None], _by_hand(Ac, R), np.where(P[..., None], 0, Ac))
        assert rc == 0 and rec["written"] == rec["erased"] == int(P.sum())
        M.check(got_m, got_c, None, (want_m, want_c, None), f"n={n} R={R.tolist()}")


@pytest.mark.parametrize("shift", [(1, 0, 0), (0, -2, 0), (0, 0, 3), (-3, 2, -1)])
def test_translations_equal_roll(shift):
    mat, rgb = M.grid("block")
    region = ((56, 8, 0), (72, 24, 16))
    sl = tuple(slice(l, h) for l, h in zip(*region))
    m, t = M.inverse_exact(M.I3, (0, 0, 0), shift)
    rc, got_m, got_c, rec = M.emul_call(mat, rgb, M._case("block", region, region, m, t, M.ERASE) | dict(value=0))
    want_m, want_c = mat.copy(), rgb.copy()
    want_m[sl], want_c[sl] = np.roll(mat[sl], shift, (0, 1, 2)), np.roll(rgb[sl], shift, (0, 1, 2))
    assert rc == 0 and rec["written"] == rec["erased"] == 512
    M.check(got_m, got_c, None, (want_m, want_c, None), f"shift {shift}")


def test_a_copy_and_the_copy_back_by_the_inverse_rotation_restore_the_block():
    mat, rgb = M.grid("block")
    src = ((60, 12, 4), (68, 20, 12))
    sl = tuple(slice(l, h) for l, h in zip(*src))
    for R in M.rotations24()[1::5]:
        there = M._forward("block", src, R, (64, 16, 8), (30, 50, 40), flags=0, exact=True) | dict(value=0)
        rc, m1, c1, r1 = M.emul_call(mat, rgb, there)
        assert rc == 0 and r1["written"] == 512 and r1["erased"] == 0 and m1[sl].tobytes() == mat[sl].tobytes()
        m1[sl], c1[sl] = 0, 0                                                               # the original cleared by hand
        back = M._forward("block", (r1["lo"], r1["hi"]), R.T, (94, 66, 48), (-30, -50, -40), flags=0, exact=True) | dict(value=0)
        rc, m2, c2, r2 = M.emul_call(m1, c1, back)
        assert rc == 0 and r2["written"] == 512 and (r2["lo"], r2["hi"]) == src
        assert m2[sl].tobytes() == mat[sl].tobytes() and c2[sl].tobytes() == rgb[sl].tobytes()


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------------
def test_the_z_step_equals_the_full_map_on_every_cell_of_a_line():
    B, T = _abi.MOVE_M_MAX, _abi.MOVE_T_MAX
    rng = np.random.default_rng(3)
    maps = [([B] * 9, [T] * 3), ([-B] * 9, [-T] * 3), ([B, -B, B, -B, B, -B, B, B, -B], [T, -T, 0]), (M.CASES["shear"]["m"], M.CASES["shear"]["t"]),
            (M.CASES["turn30_x"]["m"], M.CASES["turn30_x"]["t"])]
    maps += [(rng.integers(-B, B + 1, 9).tolist(), rng.integers(-T, T + 1, 3).tolist()) for _ in range(8)]
    for m, t in maps:
        for d in ((0, 0, 0), (255, 255, 0), (17, 200, 0), (3, 9, 100)):
            n = 256 - d[2]
            line = M.emul_line(m, t, d, n)
            for k in (0, 1, n // 2, n - 1) if n > 8 else range(n):
                S, s = M.emul_map(m, t, (d[0], d[1], d[2] + k))
                want = [sum(m[3 * a + b] * (2 * (d[0], d[1], d[2] + k)[b] + 1) for b in range(3)) + t[a] for a in range(3)]   # Python ints
                assert S == want == line[k].tolist() and s == [v >> 17 for v in want], (m, t, d, k)
            full = np.array([[sum(m[3 * a + b] * (2 * (d[0], d[1], d[2] + k)[b] + 1) for b in range(3)) + t[a] for a in range(3)] for k in range(n)], dtype=object)
            assert (line.astype(object) == full).all()
    assert max(abs(v) for v in M.emul_map([B] * 9, [T] * 3, (255, 255, 255))[0]) < 1 << 41


# ---- the facade -----------------------------------------------------------------------------------------------------------------------------
def test_move_transform_and_moved_box_against_hand_computed_values():
    from voxel_rt2_amd.renderer import Renderer
    m, t = Renderer.move_transform()
    assert m.tolist() == [[65536, 0, 0], [0, 65536, 0], [0, 0, 65536]] and t.tolist() == [0, 0, 0]
    m, t = Renderer.move_transform(shift=(1, -2, 0.5))                                      # s = d - shift
    assert t.tolist() == [-131072, 262144, -65536]
    Rz = Renderer.rotation_matrix("z", 90)                                                  # (x, y) -> (-y, x)
    assert Rz.tolist() == [[0, -1, 0], [1, 0, 0], [0, 0, 1]] and Renderer.rotation_matrix("z", -270).tolist() == Rz.tolist()
    assert Renderer.rotation_matrix((0, 2, 0), 180).tolist() == [[-1, 0, 0], [0, 1, 0], [0, 0, -1]]
    m, t = Renderer.move_transform(Rz, pivot=(64.5, 50.5, 0), shift=(0, 0, 2))              # s_x = d_y + 14, s_y = 115 - d_x, s_z = d_z - 2
    assert m.tolist() == [[0, 65536, 0], [-65536, 0, 0], [0, 0, 65536]] and t.tolist() == [14 << 17, 115 << 17, -2 << 17]
    assert M.emul_map(m.reshape(-1), t, (100, 47, 9))[1] == [61, 14, 7]
    m, t = Renderer.move_transform(Renderer.rotation_matrix("x", 30), pivot=(1, 2, 3))
    c, s = np.cos(np.pi / 6), 0.5
    assert m.tolist() == [[65536, 0, 0], [0, int(np.rint(c * 65536)), 32768], [0, -32768, int(np.rint(c * 65536))]]
    assert t.tolist() == [0, int(np.rint((2 - (2 * c + 3 * s)) * 131072)), int(np.rint((3 - (-2 * s + 3 * c)) * 131072))]
    m, t = Renderer.move_transform(np.diag([2.0, 2.0, 2.0]))
    assert m.tolist() == [[32768, 0, 0], [0, 32768, 0], [0, 0, 32768]]

    class Grid:
        voxel_grid_res = 128
    box = lambda *a, **k: Renderer.moved_box(Grid(), *a, **k)
    assert box((61, 13, 2), (68, 19, 7)) == ((60, 12, 1), (69, 20, 8))
    assert box((61, 13, 2), (68, 19, 7), shift=(0, 0, -3)) == ((60, 12, 0), (69, 20, 5))    # clipped at the grid's face
    assert box((61, 13, 2), (68, 19, 7), Rz, (64.5, 50.5, 0), (0, 0, 2)) == ((95, 46, 3), (103, 55, 10))   # x' = 115 - y in [96, 102], y' = x - 14 in [47, 54]
    assert box((61, 13, 2), (68, 19, 7), shift=(-200, 0, 0)) == ((0, 12, 1), (0, 20, 8))    # off the grid: empty
    for name in ("rot10_half", "turn30_y", "scale_2"):                                      # tests/move.py's own inversion is the same arithmetic
        assert len(M.CASES[name]["m"]) == 9
    R = M.rot("y", 30.0)
    m, t = Renderer.move_transform(R, M.CENTRE, (35, 60, 30))
    assert m.reshape(-1).tolist() == M.CASES["turn30_y"]["m"] and t.tolist() == M.CASES["turn30_y"]["t"]
    assert box(*M.SRC, R, M.CENTRE, (35, 60, 30)) == M.CASES["turn30_y"]["dst"]
    assert np.allclose(Renderer.rotation_matrix("y", 30.0), R)


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------------
def test_error_codes_of_the_emulated_call():
    mat, rgb = M.grid("clutter")
    ok = M.case("shift_near")

    def rc(**kw):
        rec = M.record_of(ok)
        for k, v in kw.items():
            rec[0][k] = v
        return M.emul_call(mat, rgb, ok, record=rec)[0]
    assert rc() == 0
    for k in ("src", "dst"):
        for lo, hi in (((2, 1, 1), (1, 2, 2)), ((-1, 0, 0), (0, 1, 1)), ((127, 127, 127), (128, 128, 129))):
            assert rc(**{k + "_lo": lo, k + "_hi": hi}) == _abi.VRT_E_INVALID, (k, lo, hi)
    B, T = _abi.MOVE_M_MAX, _abi.MOVE_T_MAX
    assert rc(m=[B] * 9) == 0 and rc(m=[-B] * 9) == 0 and rc(t=[T, -T, T]) == 0
    assert rc(m=[B + 1] + [0] * 8) == _abi.VRT_E_INVALID and rc(m=[0] * 8 + [-B - 1]) == _abi.VRT_E_INVALID
    assert rc(m=[-(1 << 31)] + [0] * 8) == _abi.VRT_E_INVALID
    assert rc(t=[0, T + 1, 0]) == _abi.VRT_E_INVALID and rc(t=[0, 0, -T - 1]) == _abi.VRT_E_INVALID and rc(t=[-(1 << 63), 0, 0]) == _abi.VRT_E_INVALID
    for flags in range(16):
        assert rc(flags=flags) == 0
    for flags in (16, 17, 0x100, 0x80000000):
        assert rc(flags=flags) == _abi.VRT_E_INVALID
    assert rc(reserved=1) == _abi.VRT_E_INVALID
    assert M.emul_call(mat, rgb, ok, want_result=False)[0] == 0                             # result may be NULL


def test_boundary_export_binding_and_records():
    assert "vrt_move_voxels" in _lib.exported_symbols()
    hip = _lib.load()
    _abi.declare(hip, "vrt_")
    assert hip.vrt_move_voxels.restype is C.c_int and len(hip.vrt_move_voxels.argtypes) == 5
    assert _abi.VOXEL_MOVE.itemsize == 120 and _abi.MOVE_RESULT.itemsize == 48
    assert [_abi.VOXEL_MOVE.fields[k][1] for k in ("src_lo", "dst_lo", "m", "select_value", "t", "flags", "reserved")] == [0, 24, 48, 84, 88, 112, 116]
    assert (_abi.MOVE_ERASE_SOURCE, _abi.MOVE_KEEP_SOLID, _abi.MOVE_DRY_RUN, _abi.MOVE_IF_FREE) == (1, 2, 4, 8)
    rec = M.record_of(M.case("shift_near"))
    assert hip.vrt_move_voxels(None, rec.ctypes.data_as(C.c_void_p), None, 0, None) == _abi.VRT_E_INVALID    # refused before any device work
    tile = np.zeros(4, np.int32)
    M.lib().move_emul_tile(tile.ctypes.data_as(C.c_void_p))
    assert tile.tolist() == [4, 4, 64, 4] and M.lib().move_emul_plan(1000, 10, 0) < 4 * 1000 + 4 * 1000 + 2048 <= M.lib().move_emul_plan(1000, 10, 1) + 2048


def test_standalone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "move_emul_asan")
    build = subprocess.run(M.GCC[:1] + ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMOVE_EMUL_MAIN", "-Wno-unknown-pragmas",
                                        "-o", exe, M._SRC], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-3000:]
    assert run.stdout.startswith("ok:")
