"""vrt_gather_probes on the host: the per-item functions of voxel_rt2_amd/csrc/vrt_probe_sh.h compiled with g++ (tests/emul/probe_emul.cpp
drives them the way the library and its two kernels do) against the expectation of tests/probe.py -- the oracle's own sampling, shadow
ray, escape test and sky value (tests/emul/probe_orc.cpp), the radiance query's host build for the rays that hit, the basis, the
products and the ordered sums in numpy float32 -- bit for bit, on every case and both views of the pyramid; forced chunks and blocks; a
permuted batch; every frame parameter a gather does not read poisoned: the same bytes.  Then what the oracle's data cover (conditions
on the inputs, not measurements), the basis against float32 known answers, the plan, the facade's host helpers (sh_irradiance,
sh_radiance, probe_lattice), and the boundary: exports, bindings, record sizes, the error codes that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import probe as P
from voxel_rt2_amd import _abi, _lib
from voxel_rt2_amd.renderer import Renderer


@pytest.mark.parametrize("case", list(P.CASES))
def test_host_build_equals_expectation(case):
    h = P.host_scene(case)
    probes = P.probes_of(case)
    for n in P.SAMPLES:
        want = P.expected_host(case, n)
        for staged in (0, 1):
            P.check(h.gather(probes, n, staged=staged), probes, want, f"{case} samples {n} staged={staged}")


@pytest.mark.parametrize("case", ["sunlit_d5", "dense_ref", "s1_256"])
def test_forced_chunks_blocks_and_a_permuted_batch(case):
    """Chunks of 1, 2 and all samples; the batch cut into blocks of 50 probes; the batch permuted: the same records, permuted."""
    h = P.host_scene(case)
    probes = P.probes_of(case)
    n = max(P.SAMPLES)
    want = P.expected_host(case, n)
    for staged in (0, 1):
        for per in (1, 2, n):
            assert h.gather(probes, n, staged=staged, per=per).tobytes() == want.tobytes(), (staged, per)
    cut = np.concatenate([h.gather(probes[at:at + 50], n) for at in range(0, len(probes), 50)])
    assert cut.tobytes() == want.tobytes()
    perm = np.random.default_rng(3).permutation(len(probes))
    assert h.gather(probes[perm], n, per=2).tobytes() == want[perm].tobytes()


def test_poison_is_live():
    """tests/test_cast_rays_host.py's check on this emulator's conversion (scene_sampled: camera_is_moving 1 plain, 0 poisoned)."""
    from test_cast_rays_host import check_probe_is_live
    h = P.host_scene("sunlit_d5")
    plain = P.probe(h.s)
    with P.poisoned():
        poisoned = P.probe(h.s)
    check_probe_is_live(plain, poisoned, (1, 0))
    assert P.lib().probe_emul_poison(0) == 0


@pytest.mark.parametrize("case", list(P.CASES))
def test_poisoned_frame_parameters_change_no_byte(case):
    """Every field of FrameParams a gather is not meant to read poisoned (tests/emul/query_emul.h): the same bytes as in the plain mode
    -- which test_host_build_equals_expectation pins to the expectation -- on both views, in the plan's chunks and in chunks of one."""
    h = P.host_scene(case)
    probes = P.probes_of(case)
    for n in P.SAMPLES:
        for staged in (0, 1):
            plain = h.gather(probes, n, staged=staged)
            with P.poisoned():
                for per in (0, 1):
                    got = h.gather(probes, n, staged=staged, per=per)
                    assert got.tobytes() == plain.tobytes(), (f"{case} samples {n} staged={staged} per={per}: "
                                                               f"{P.mismatches(got, plain).size} of {len(probes)} records differ")


def test_the_oracles_data_cover_what_they_claim():
    """From the oracle's rows alone: every sun-lit case holds samples that see the sun, that are shadowed, whose first segment escapes,
    whose first segment hits, and that escape inside the sun's cone (the samples the disc must not be counted for).  Probes inside the
    closed box see neither sky nor sun; invalid probes are all zeros."""
    for case in P.SUNLIT:
        c = P.census(case)
        print(f"probe census {case}: {c}")
        assert c["visible"] >= 20 and c["shadowed"] >= 20 and c["escapes"] >= 20 and c["hits"] >= 20 and c["escape_in_cone"] >= 8, (case, c)
    for case in P.CASES:
        fam = P.families(case)
        assert all(16 <= len(f) <= 48 for name, f in fam.items() if name != "invalid"), {k: len(v) for k, v in fam.items()}
        assert len(fam["invalid"]) == 9 and not P.valid(fam["invalid"]).any()
        got = P.expected_host(case, 3)[P.family_slices(case)["invalid"]]
        assert not P.as_floats(got).view(np.uint32).any()
    rows, sl = P.oracle_rows("sunlit_d5"), P.family_slices("sunlit_d5")
    assert (rows[sl["closed_box"], :, 10] == 0).all() and (rows[sl["closed_box"], :, 3] == 0).all()
    want = P.expected_host("sunlit_d5", 3)
    assert (want["sky"][sl["closed_box"]] == 0).all() and (want["sun"][sl["closed_box"]] == 0).all() and (want["sun_rgb"][sl["closed_box"]] == 0).all()
    assert (want["sky"][sl["open_air"]] > 0).any() and (want["sun"][sl["open_air"]] > 0).any() and (want["sh"][sl["emissive"]][:, 0] > 0).any()
    assert (want["sky"][sl["under_roof"]] < 1).any() and (want["sun"][sl["under_roof"]] < 1).any()


def test_escape_inside_the_cone_is_worth_the_sky_only():
    """The wide-sun case: for the samples that escape inside the cone the radiance query's value (disc included) differs from the
    oracle's sky-only value, and the host build's item carries the latter."""
    rows, probes = P.oracle_rows("cone"), P.probes_of("cone")
    h = P.host_scene("cone")
    pick = P.valid(probes) & (rows[:, 0, 10] == 1) & (rows[:, 0, 11] == 1)
    assert pick.sum() >= 5
    rays = np.zeros(int(pick.sum()), P.PATH_RAY)
    rays["origin"], rays["dir"], rays["stream"] = probes["pos"][pick], rows[pick, 0, 7:10], probes["stream"][pick]
    with_disc = h.query(rays, P.FIRST_FRAME)
    assert (with_disc > rows[pick, 0, 12:15]).any(axis=1).all()
    got = h.gather(probes[pick], 1)
    assert (got["sh"][:, 0] == rows[pick, 0, 12:15] * P.K4 * np.float32(0.282094792)).all() and (got["sky"] == 1).all()


def test_basis_known_answers():
    """probe_basis at the six axis directions and at (1, 1, 1) / sqrt(3) against float32 known answers: on an axis every product is
    exact, so the answers are the constants themselves; on the diagonal each is the stated left-to-right float32 expression."""
    f = np.float32
    k1, k2, k6, k8 = f(0.488602512), f(1.09254843), f(0.315391565), f(0.546274215)

    def got(x, y, z):
        out = np.zeros(9, np.float32)
        P.lib().probe_emul_basis(float(x), float(y), float(z), out.ctypes.data_as(C.c_void_p))
        return out
    y0 = f(0.282094792)
    m1 = f(0.315391565) * f(-1.0)
    two = f(0.315391565) * f(2.0)
    known = {(1, 0, 0): [y0, 0, 0, k1, 0, 0, m1, 0, k8], (-1, 0, 0): [y0, 0, 0, -k1, 0, 0, m1, 0, k8],
             (0, 1, 0): [y0, k1, 0, 0, 0, 0, m1, 0, -k8], (0, -1, 0): [y0, -k1, 0, 0, 0, 0, m1, 0, -k8],
             (0, 0, 1): [y0, 0, k1, 0, 0, 0, two, 0, 0], (0, 0, -1): [y0, 0, -k1, 0, 0, 0, two, 0, 0]}
    for d, want in known.items():
        assert (got(*d) == np.array(want, np.float32)).all(), (d, got(*d), want)
    s = f(1.0) / np.sqrt(f(3.0))                                                       # binary32: 0.57735026
    ss = s * s
    want = np.array([y0, k1 * s, k1 * s, k1 * s, k2 * ss, k2 * ss, k6 * (f(3.0) * ss - f(1.0)), k2 * ss, k8 * (ss - ss)], np.float32)
    assert got(s, s, s).tobytes() == want.tobytes() and want[8] == 0 and abs(float(want[6])) < 1e-7 and abs(float(want[4]) - 0.36418281) < 1e-7
    assert P.basis(np.array([[s, s, s]], np.float32))[0].tobytes() == want.tobytes()     # tests/probe.py's numpy basis is the same expression


def test_plan_item_cap_and_a_full_blocks_single_sample():
    lib = P.lib()
    budget, size = lib.probe_emul_items(), lib.probe_emul_item_bytes()
    assert size == 48 and P.ITEM.itemsize == 48 and budget == 1 << 18 and budget * size == 12 << 20      # the radiance plane's 12 MiB
    for n in (0, 1, 255, 1 << 18, (1 << 18) + 1, 3 << 18, 1 << 40):
        m = lib.probe_emul_rays(n)
        assert m == min(n, 1 << 18) and m <= budget                                  # one sample of a full block fits the plane
    assert lib.probe_emul_chunk(1 << 18, 1) == 1 and lib.probe_emul_chunk(1 << 18, 7) == 1 and lib.probe_emul_chunk(1 << 17, 7) == 2
    rng = np.random.default_rng(20261019)
    shapes = [(1, 1), (1, 65536), (2048, 600), (1 << 18, 4), (budget - 1, 2), (budget // 2 + 1, 5), (777, 1350)]
    shapes += [(int(rng.integers(1, (1 << 18) + 1)), int(rng.integers(1, 65537))) for _ in range(200)]
    for n, spp in shapes:
        per = lib.probe_emul_chunk(n, spp)
        assert 1 <= per <= spp and n * per <= budget, (n, spp, per)
        assert per == spp or n * (per + 1) > budget, (n, spp, per)                     # as many whole samples as fit
        cut = P.chunks(n, spp)
        assert cut[0][0] == 0 and sum(c for _, c in cut) == spp and all(a + c == b for (a, c), (b, _) in zip(cut, cut[1:])), (n, spp)
    assert P.chunks(1, 65536) == [(0, 65536)] and P.blocks(0) == [] and P.blocks(5) == [(0, 5)]
    assert len(P.blocks((1 << 18) + 1)) == 2 and len(P.chunks(1 << 18, 2)) == 2


def test_fold_is_chunk_invariant_for_every_cut_of_seven_samples():
    lib = P.lib()
    rng = np.random.default_rng(7)
    n = 4
    plane = np.zeros((7, n), P.ITEM)                                                  # [sample][probe]: a sample's probes side by side
    plane["L"] = np.abs(rng.normal(size=(7, n, 3)) * 10.0 ** rng.integers(-4, 4, size=(7, n, 3)))
    w = rng.normal(size=(7, n, 3))
    plane["w"] = w / np.linalg.norm(w, axis=2, keepdims=True)
    plane["sky"], plane["vis"] = rng.integers(0, 2, (7, n)), rng.integers(0, 2, (7, n))
    plane["sun"] = rng.uniform(0, 3, (7, n, 3))
    want = np.zeros((n, 32), np.float32)
    for s in range(7):
        want = P.fold(want, np.ascontiguousarray(plane[s]).view(np.float32).reshape(n, 12))
    want = (want / np.float32(7)).astype(np.float32)
    for cut in range(1 << 6):                                                         # a bit per boundary between consecutive samples
        bounds = [0] + [k + 1 for k in range(6) if cut >> k & 1] + [7]
        for k in range(n):
            acc = np.zeros(32, np.float32)
            for a, b in zip(bounds, bounds[1:]):
                lib.probe_emul_fold(acc.ctypes.data_as(C.c_void_p), C.c_void_p(plane.ctypes.data + (a * n + k) * 48), n, b - a, 7 if b == 7 else 0)
            assert acc.tobytes() == want[k].tobytes(), (cut, k)
    h = P.host_scene("sunlit_d5")
    probes = np.concatenate([P.families("sunlit_d5")[f][:6] for f in ("open_air", "among_blocks", "under_roof", "emissive", "invalid")])
    whole = h.gather(probes, 7, per=7)
    for per in (1, 2, 3, 4, 6, 0):
        assert h.gather(probes, 7, per=per).tobytes() == whole.tobytes(), per


def test_invalid_probes():
    ok = lambda p: bool(P.lib().probe_emul_valid(p.ctypes.data_as(C.c_void_p)))
    assert ok(P.make((0.0, 0.5, 0.0))) and ok(P.make((1e30, -1e30, 1e-40)))
    bad = P.invalid_probes()
    assert len(bad) == 9 and not P.valid(bad).any()
    for k in range(len(bad)):
        assert not ok(bad[k:k + 1]), bad[k]
    h = P.host_scene("sunlit_d5")
    good = P.families("sunlit_d5")["open_air"][:5]
    mixed = np.concatenate([good[:2], bad[5:6], good[2:4], bad[0:1], good[4:]])
    for staged in (0, 1):
        got = h.gather(mixed, 3, staged=staged, per=2)
        assert not P.as_floats(got[[2, 5]]).view(np.uint32).any()
        assert got[[0, 1, 3, 4, 6]].tobytes() == h.gather(good, 3, staged=staged).tobytes()     # and the probes around them are not disturbed


# ---- the facade's host helpers ------------------------------------------------------------------------------------------------------
def exact_basis(n):
    """The real spherical harmonics of bands 0 to 2, polar axis z, in float64 from their closed forms."""
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    pi = np.pi
    return np.stack([np.full(len(n), 0.5 / np.sqrt(pi)), np.sqrt(3 / (4 * pi)) * y, np.sqrt(3 / (4 * pi)) * z, np.sqrt(3 / (4 * pi)) * x,
                     0.5 * np.sqrt(15 / pi) * x * y, 0.5 * np.sqrt(15 / pi) * y * z, 0.25 * np.sqrt(5 / pi) * (3 * z * z - 1),
                     0.5 * np.sqrt(15 / pi) * x * z, 0.25 * np.sqrt(15 / pi) * (x * x - y * y)], axis=1)


def test_sh_irradiance_and_sh_radiance_identities():
    """Float64 polynomial identities, so the bound is derived: a handful of float64 operations a value, 1e-12 relative is three
    orders of magnitude above their rounding.  Coefficients e_i: E = A_l * Y_i(n), L = Y_i(n), over 100 random unit normals.  Constant
    radiance 1 is c = 4 pi Y0 e_0 ... projected: c0 = integral of Y0 = 4 pi Y0; its irradiance is pi on every normal."""
    rng = np.random.default_rng(100)
    n = rng.normal(size=(100, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    Y = exact_basis(n)
    A = [np.pi] + [2 * np.pi / 3] * 3 + [np.pi / 4] * 5
    for i in range(9):
        rec = np.zeros(1, _abi.SH_PROBE)
        rec["sh"][0, i] = (1.0, 1.0, 1.0)
        rec["sun_rgb"] = 5.0                                                          # left out: no light direction is passed
        e, l = Renderer.sh_irradiance(rec, n), Renderer.sh_radiance(rec, n)
        assert e.shape == (100, 3) and e.dtype == np.float64 and l.shape == (100, 3)
        tol = 1e-12 * np.abs(Y[:, i]).max()
        assert np.abs(e - (A[i] * Y[:, i])[:, None]).max() <= tol * A[i] and np.abs(l - Y[:, i][:, None]).max() <= tol, i
    # float32 records hold c0 = 4 pi Y0 only to binary32, so the constant-radiance identity is checked on a float64 structured array
    rec = np.zeros(1, np.dtype([("sh", np.float64, (9, 3)), ("sun_rgb", np.float64, 3)]))
    rec["sh"][0, 0] = 4 * np.pi * 0.5 / np.sqrt(np.pi)
    e = Renderer.sh_irradiance(rec, n)
    assert np.abs(e / np.pi - 1).max() <= 1e-12
    assert np.abs(Renderer.sh_radiance(rec, n) - 1).max() <= 1e-12
    # the sun's term: sun_rgb * max(0, n . light_direction)
    rec = np.zeros(2, _abi.SH_PROBE)
    rec["sun_rgb"] = ((1.0, 2.0, 4.0), (0.5, 0.5, 0.5))
    e = Renderer.sh_irradiance(rec, [(0, 1, 0), (0, -1, 0)], light_direction=(0, 1, 0))
    assert e.tolist() == [[1.0, 2.0, 4.0], [0.0, 0.0, 0.0]]


def test_probe_lattice_lists_exactly_the_empty_lattice_cells():
    """A hand-made 8^3 block in a 128^3 grid: a solid 4^3 core with one cell dug out, lattice steps 1, 2 and 3."""
    import sensor as S
    mat = np.zeros((128, 128, 128), np.int8)
    mat[10:14, 20:24, 30:34] = 3
    mat[12, 22, 32] = 0
    mat[8, 18, 28] = -1                                                               # not solid: material <= 0 is empty
    st = S.store(mat)
    lo, hi = (8, 18, 28), (16, 26, 36)
    for step in (1, 2, 3):
        centre, cell = st.probe_lattice(lo, hi, step)
        assert cell.dtype == np.int32 and centre.dtype == np.float32 and cell.shape == centre.shape
        want = [(x, y, z) for x in range(8, 16, step) for y in range(18, 26, step) for z in range(28, 36, step) if mat[x, y, z] <= 0]
        assert [tuple(int(v) for v in c) for c in cell] == want, step
        assert (centre == ((cell + 0.5 - 64) / 64).astype(np.float32)).all()
    _, cell = st.probe_lattice(lo, hi, 2)
    got = {tuple(int(v) for v in c) for c in cell}
    assert (12, 22, 32) in got and (8, 18, 28) in got and (10, 20, 30) not in got and len(got) == 64 - 8 + 1
    assert len(st.probe_lattice(lo, hi, 1)[0]) == 512 - 64 + 1
    assert len(st.probe_lattice((0, 0, 0), (0, 5, 5), 1)[0]) == 0 and len(st.probe_lattice(step=32)[0]) == 64
    with pytest.raises(ValueError):
        st.probe_lattice(lo, hi, 0)


def test_exports_bindings_record_sizes_and_codes_without_a_device():
    assert "vrt_gather_probes" in _lib.exported_symbols()
    assert _abi.PROBE.itemsize == 16 and _abi.SH_PROBE.itemsize == 128
    assert [_abi.PROBE.fields[k][1] for k in ("pos", "stream")] == [0, 12]
    assert [_abi.SH_PROBE.fields[k][1] for k in ("sh", "sky", "sun_rgb", "sun")] == [0, 108, 112, 124] and _abi.SH_PROBE["sh"].shape == (9, 3)
    lib = _lib.load()
    fn = lib.vrt_gather_probes
    _abi.declare(lib, "vrt_")
    assert fn.restype is C.c_int and len(fn.argtypes) == 7 and fn.argtypes[1] is C.c_int64 and fn.argtypes[4] is C.c_uint32
    s, o = np.zeros(1, _abi.PROBE), np.zeros(1, _abi.SH_PROBE)
    assert fn(None, 1, s.ctypes.data_as(C.c_void_p), 1, 0, o.ctypes.data_as(C.c_void_p), 0) == _abi.VRT_E_INVALID
    assert b"null" in lib.vrt_last_error()


def test_emulation_program_under_sanitizers(tmp_path):
    """tests/emul/probe_emul.cpp as a stand-alone program (-DPROBE_EMUL_MAIN: a scene of its own, both views, two chunkings, the
    poisoned frame parameters) built with the address and undefined-behaviour sanitizers and run."""
    exe = str(tmp_path / "probe_emul_san")
    src = os.path.join(P.HERE, "emul", "probe_emul.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-Wall", "-Werror", "-Wno-unused-function",
                    "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DPROBE_EMUL_MAIN", "-o", exe, src],
                   check=True, capture_output=True)
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "views and chunkings agree" in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.stdout, r.stderr)
