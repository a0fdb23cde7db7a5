"""vrt_gather_irradiance on the host: the per-item functions of voxel_rt2_amd/csrc/vrt_sensor.h compiled with g++ (tests/emul/sensor_emul.cpp
drives them the way the library and its two kernels do) against the expectation of tests/sensor.py -- the oracle's own sampling, shadow
ray, escape test and sky value (tests/emul/sensor_orc.cpp), the radiance query's host build for the hemisphere rays that hit, the fold
in numpy -- bit for bit, on every case and both views of the pyramid; and again with every frame parameter a gather does not read poisoned: the
same bytes.  Then what the oracle's data cover (conditions, not
measurements), the plan, the fold across chunks, invalid sensors, Renderer.surface_faces, and the boundary: exports, bindings, record
sizes, the error codes that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sensor as S
from voxel_rt2_amd import _abi, _lib


@pytest.mark.parametrize("case", list(S.CASES))
def test_host_build_equals_expectation(case):
    h = S.host_scene(case)
    sensors = S.sensors_of(case)
    for n in S.SAMPLES:
        want = S.expected_host(case, n)
        for staged in (0, 1):
            S.check(h.gather(sensors, n, staged=staged), sensors, want, f"{case} samples {n} staged={staged}")


def test_poison_is_live():
    """tests/test_cast_rays_host.py's check on this emulator's conversion (scene_sampled: camera_is_moving 1 plain, 0 poisoned)."""
    from test_cast_rays_host import check_probe_is_live
    h = S.host_scene("sunlit_d5")
    plain = S.probe(h.s)
    with S.poisoned():
        poisoned = S.probe(h.s)
    check_probe_is_live(plain, poisoned, (1, 0))
    assert S.lib().sensor_emul_poison(0) == 0


@pytest.mark.parametrize("case", list(S.CASES))
def test_poisoned_frame_parameters_change_no_byte(case):
    """Every field of FrameParams a gather is not meant to read poisoned (tests/emul/query_emul.h): the same bytes as in the plain mode
    -- which test_host_build_equals_expectation pins to the expectation -- for every sensor and sample count, on both views, in the
    plan's chunks and in chunks of one sample."""
    h = S.host_scene(case)
    sensors = S.sensors_of(case)
    for n in S.SAMPLES:
        for staged in (0, 1):
            plain = h.gather(sensors, n, staged=staged)
            with S.poisoned():
                for per in (0, 1):
                    got = h.gather(sensors, n, staged=staged, per=per)
                    assert got.tobytes() == plain.tobytes(), (f"{case} samples {n} staged={staged} per={per}: "
                                                               f"{S.mismatches(got, plain).size} of {len(sensors)} records differ")


def test_the_oracles_data_cover_what_they_claim():
    """From the oracle's data alone.  Every sun-lit case: at least 20 samples see the sun (vis_s = 1), at least 20 face it and are
    shadowed (vis_s = 0 with ndl > 0).  The wide-sun case: at least 20 samples escape inside the sun's cone -- the samples the disc must
    not be counted for.  Sensors inside the closed box see neither sky nor sun; the roof's underside faces away from the sun."""
    for case in S.SUNLIT:
        c = S.census(case)
        print(f"sensor census {case}: {c}")
        assert c["visible"] >= 20 and c["shadowed"] >= 20 and c["facing_away"] >= 20 and c["escapes"] >= 20 and c["hits"] >= 20, (case, c)
    assert S.census("cone")["escape_in_cone"] >= 20
    rows, sl = S.oracle_rows("sunlit_d5"), S.family_slices("sunlit_d5")
    assert len(S.families("sunlit_d5")["closed_box"]) >= 24 and (rows[sl["closed_box"], :, 14] == 0).all() and (rows[sl["closed_box"], :, 7] == 0).all()
    assert (rows[sl["away"], :, 6] <= 0).all() and (rows[sl["away"], :, 7] == 0).all()
    want = S.expected_host("sunlit_d5", 3)
    assert (want["sky"][sl["closed_box"]] == 0).all() and (want["sun"][sl["closed_box"]] == 0).all()
    assert (want["sun"][sl["away"]] == 0).all() and (want["sun_rgb"][sl["away"]] == 0).all()
    assert (want["sky_rgb"][sl["emissive"]] > 0).any() and (want["sun"][sl["floor"]] > 0).any() and (want["sky"][sl["overhang"]] < 1).any()
    n = S.families("sunlit_d5")["oblique"]["normal"]
    assert (np.abs(n[:, 1]) > 0.9).any() and (np.abs(n[:, 1]) <= 0.9).any()              # both branches of make_orthonormal_basis
    for case in S.CASES:                                                                 # invalid sensors: all zeros, +0
        got = S.expected_host(case, 3)[S.family_slices(case)["invalid"]]
        assert not S.as_floats(got).view(np.uint32).any()


def test_escape_inside_the_cone_is_worth_the_sky_only():
    """The wide-sun case: for the samples that escape inside the cone the radiance query's value (disc included) differs from the
    oracle's sky-only value, and the host build returns the latter."""
    rows, sensors = S.oracle_rows("cone"), S.sensors_of("cone")
    ok = S.valid(sensors)
    h = S.host_scene("cone")
    pick = ok & (rows[:, 0, 14] == 1) & (rows[:, 0, 15] == 1)
    assert pick.sum() >= 5
    rays = np.zeros(int(pick.sum()), S.PATH_RAY)
    rays["origin"], rays["dir"], rays["stream"] = rows[pick, 0, 0:3], rows[pick, 0, 11:14], sensors["stream"][pick]
    with_disc = h.query(rays, S.FIRST_FRAME)
    assert (with_disc > rows[pick, 0, 16:19]).any(axis=1).all()
    got = h.gather(sensors[pick], 1)
    assert (S.as_floats(got)[:, 0:3] == rows[pick, 0, 16:19] * S.PI32).all() and (got["sky"] == 1).all()


def test_plan_covers_every_item_once_within_the_byte_budget():
    lib = S.lib()
    budget, size = lib.sensor_emul_items(), lib.sensor_emul_item_bytes()
    assert size == 32 and budget * size <= 12 << 20 and budget >= 1 << 16        # no more than the radiance plane's 12 MiB
    rng = np.random.default_rng(20261018)
    shapes = [(1, 1), (1, 65536), (2048, 600), (1 << 18, 4), (1 << 18, 65536), (budget, 2), (budget - 1, 2), (budget // 2 + 1, 5), (777, 1350)]
    shapes += [(int(rng.integers(1, (1 << 18) + 1)), int(rng.integers(1, 65537))) for _ in range(200)]
    for n, spp in shapes:
        per = lib.sensor_emul_chunk(n, spp)
        assert 1 <= per <= spp and (n * per <= budget or per == 1), (n, spp, per)
        assert per == spp or n * (per + 1) > budget, (n, spp, per)                 # as many whole samples as fit
        cut = S.chunks(n, spp)
        assert cut[0][0] == 0 and sum(c for _, c in cut) == spp and all(a + c == b for (a, c), (b, _) in zip(cut, cut[1:])), (n, spp)
        assert all(1 <= c <= per for _, c in cut)
    assert S.chunks(1, 65536) == [(0, 65536)]                                      # one sensor x 65 536 samples: one launch
    for n in (0, 1, 255, 1 << 18, (1 << 18) + 1, 3 << 18, 1 << 40):
        m = lib.sensor_emul_rays(n)
        assert m == min(n, 1 << 18) and m <= budget                               # one sample of a block fits the plane
    assert S.blocks(0) == [] and S.blocks(5) == [(0, 5)]
    # every item exactly once: blocks x chunks x items of a launch, for a call of more than one block and more than one chunk
    n, spp = (1 << 18) + 3, 3
    seen = np.zeros((n, spp), np.uint8)
    for at, m in S.blocks(n):
        for s0, count in S.chunks(m, spp):
            i = np.arange(m * count)
            np.add.at(seen, (at + i % m, s0 + i // m), 1)
    assert (seen == 1).all() and len(S.blocks(n)) == 2 and len(S.chunks(1 << 18, spp)) == 3


def test_fold_is_chunk_invariant_for_every_cut_of_seven_samples():
    lib = S.lib()
    rng = np.random.default_rng(7)
    n = 5
    plane = (rng.normal(size=(7, n, 8)) * 10.0 ** rng.integers(-6, 6, size=(7, n, 8))).astype(np.float32)   # [sample][sensor]: a sample's sensors side by side
    want = np.zeros((n, 8), np.float32)
    for s in range(7):
        want = want + plane[s]
    want = (want / np.float32(7)).astype(np.float32)
    for cut in range(1 << 6):                                                       # a bit per boundary between consecutive samples
        bounds = [0] + [k + 1 for k in range(6) if cut >> k & 1] + [7]
        for k in range(n):
            acc = np.zeros(8, np.float32)
            for a, b in zip(bounds, bounds[1:]):
                lib.sensor_emul_fold(acc.ctypes.data_as(C.c_void_p), C.c_void_p(plane.ctypes.data + (a * n + k) * 32), n, b - a, 7 if b == 7 else 0)
            assert acc.tobytes() == want[k].tobytes(), (cut, k)
    h = S.host_scene("sunlit_d5")
    sensors = np.concatenate([S.families("sunlit_d5")[f][:6] for f in ("floor", "tops", "overhang", "emissive", "invalid")])
    whole = h.gather(sensors, 7, per=7)
    for per in (1, 2, 3, 4, 6, 0):
        assert h.gather(sensors, 7, per=per).tobytes() == whole.tobytes(), per
    acc = np.zeros((len(sensors), 8), np.float32)
    for s in range(7):
        acc = acc + S.as_floats(h.gather(sensors, 1, first_frame=S.FIRST_FRAME + s))
    assert (acc / np.float32(7)).astype(np.float32).tobytes() == S.as_floats(whole).tobytes()


def test_invalid_sensors():
    ok = lambda s: bool(S.lib().sensor_emul_valid(s.ctypes.data_as(C.c_void_p)))
    up = (0.0, 1.0, 0.0)
    assert ok(S.make((0.0, 0.5, 0.0), up)) and ok(S.make((1e30, -1e30, 0.0), (0.0, -0.0, 1e-40))) and ok(S.make((0, 0, 0), (1e20, 3e38, 0.0)))
    bad = S.invalid_sensors()
    assert len(bad) == 8 and not S.valid(bad).any()
    for k in range(len(bad)):
        assert not ok(bad[k:k + 1]), bad[k]
    h = S.host_scene("sunlit_d5")
    good = S.families("sunlit_d5")["floor"][:5]
    mixed = np.concatenate([good[:2], bad[5:6], good[2:4], bad[0:1], good[4:]])
    for staged in (0, 1):
        got = h.gather(mixed, 3, staged=staged, per=2)
        assert not S.as_floats(got[[2, 5]]).view(np.uint32).any()
        assert got[[0, 1, 3, 4, 6]].tobytes() == h.gather(good, 3, staged=staged).tobytes()     # and the sensors around them are not disturbed


def test_a_normal_too_long_for_a_ray_is_a_zero_sample():
    """A finite normal is a valid sensor however long it is, but the rays derived from it pass vrt_trace_radiance's gate before anything
    is walked.  Longer than 2^64 (about 1.8e19) its squared length overflows binary32, the hemisphere vector normal + (a vector no longer
    than 1) is divided by an infinite length, and w is all zeros: not a ray, so every term of the sample is zero.  At the largest finite
    position o = pos + normal * 1e-6 overflows as well.  A normal of 1e18 is long and still gives rays: from 1e12 above the scene, facing
    up, every sample sees the whole sky and the sun."""
    fmax = np.finfo(np.float32).max
    long_ = np.concatenate([S.make((0, 0, 0), (1e20, 3e38, 0.0)), S.make((0.1, -0.2, 0.3), (0.0, -2e19, 0.0)), S.make((0.1, 0.2, 0.3), (3e19, 0.0, -3e19)),
                            S.make((fmax, 0.0, 0.0), (fmax, 0.0, 0.0))])
    with np.errstate(over="ignore"):
        assert np.isinf((long_["normal"] * long_["normal"]).sum(axis=1, dtype=np.float32)).all()
        assert np.isinf(long_["pos"][3] + long_["normal"][3] * np.float32(1e-6)).any()
    assert S.valid(long_).all() and all(S.lib().sensor_emul_valid(long_[k:k + 1].ctypes.data_as(C.c_void_p)) for k in range(len(long_)))
    far = S.make((0.0, 0.0, 0.0), (0.0, 1e18, 0.0))
    good = S.families("sunlit_d5")["floor"][:3]
    mixed = np.concatenate([good[:1], long_[:2], good[1:2], far, long_[2:], good[2:]])
    mixed["stream"] = np.arange(len(mixed)) * 3 + 1
    h = S.host_scene("sunlit_d5")
    for staged in (0, 1):
        got = h.gather(mixed, 3, staged=staged, per=2)
        assert not S.as_floats(got[[1, 2, 5, 6]]).view(np.uint32).any()
        assert got["sky"][4] == 1 and got["sun"][4] == 1 and (got["sun_rgb"][4] > 0).all()
        assert got[[0, 3, 7]].tobytes() == h.gather(mixed[[0, 3, 7]], 3, staged=staged).tobytes()


def test_surface_faces_against_a_triple_loop():
    """A 12^3 corner of a 128^3 grid holding a voxel on the grid's boundary, an enclosed voxel with no exposed face, and a one-voxel gap."""
    rng = np.random.default_rng(12)
    mat = np.zeros((128, 128, 128), np.int8)
    mat[:12, :12, :12] = rng.integers(0, 3, (12, 12, 12)) * (rng.random((12, 12, 12)) < 0.45)
    mat[0, 0, 0] = 1                                     # on the boundary
    mat[4:7, 4:7, 4:7] = 1                               # (5, 5, 5) is enclosed
    mat[8, 8, 7], mat[8, 8, 8], mat[8, 8, 9] = 1, 0, 1   # a one-voxel gap
    mat[12, 3, 3] = 1                                    # just outside the box: hides the +x face of (11, 3, 3) if that is solid
    mat[11, 3, 3] = 1
    st = S.store(mat)
    lo, hi = (0, 0, 0), (12, 12, 12)
    cell, face, centre, normal = st.surface_faces(lo, hi)
    assert cell.dtype == np.int32 and face.dtype == np.int8 and centre.dtype == np.float32 and normal.dtype == np.float32
    steps = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
    want = set()
    for x in range(12):
        for y in range(12):
            for z in range(12):
                if mat[x, y, z] <= 0:
                    continue
                for k, (dx, dy, dz) in enumerate(steps):
                    a, b, c = x + dx, y + dy, z + dz
                    if not (0 <= a < 128 and 0 <= b < 128 and 0 <= c < 128) or mat[a, b, c] <= 0:
                        want.add((x, y, z, k))
    got = [tuple(int(v) for v in c) + (int(f),) for c, f in zip(cell, face)]
    assert len(got) == len(set(got)) and set(got) == want
    assert (0, 0, 0, 0) in want and (0, 0, 0, 2) in want and not any(g[:3] == (5, 5, 5) for g in got)
    assert (8, 8, 7, 5) in want and (8, 8, 9, 4) in want and (11, 3, 3, 1) not in want
    for (x, y, z, k), c, n in zip(got, centre, normal):
        assert tuple(n) == steps[k]
        assert tuple(c) == tuple(np.float32((v + 0.5 - 64) / 64 + 0.5 * d / 64) for v, d in zip((x, y, z), steps[k]))
    whole = st.surface_faces()
    assert len(whole[0]) == len(cell) + 5                # the whole grid adds (12, 3, 3): every face but -x


def test_exports_bindings_record_sizes_and_codes_without_a_device():
    assert "vrt_gather_irradiance" in _lib.exported_symbols()
    assert _abi.SENSOR.itemsize == 32 and _abi.IRRADIANCE.itemsize == 32
    assert [_abi.SENSOR.fields[k][1] for k in ("pos", "stream", "normal", "reserved")] == [0, 12, 16, 28]
    assert [_abi.IRRADIANCE.fields[k][1] for k in ("sky_rgb", "sky", "sun_rgb", "sun")] == [0, 12, 16, 28]
    lib = _lib.load()
    fn = lib.vrt_gather_irradiance
    _abi.declare(lib, "vrt_")
    assert fn.restype is C.c_int and len(fn.argtypes) == 7 and fn.argtypes[1] is C.c_int64 and fn.argtypes[4] is C.c_uint32
    s, o = np.zeros(1, _abi.SENSOR), np.zeros(1, _abi.IRRADIANCE)
    assert fn(None, 1, s.ctypes.data_as(C.c_void_p), 1, 0, o.ctypes.data_as(C.c_void_p), 0) == _abi.VRT_E_INVALID
    assert b"null" in lib.vrt_last_error()


def test_emulation_program_under_sanitizers(tmp_path):
    """tests/emul/sensor_emul.cpp as a stand-alone program (-DSENSOR_EMUL_MAIN: a scene of its own, both views, two chunkings) built with
    the address and undefined-behaviour sanitizers and run."""
    exe = str(tmp_path / "sensor_emul_san")
    src = os.path.join(S.HERE, "emul", "sensor_emul.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-Wall", "-Werror", "-Wno-unused-function",
                    "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DSENSOR_EMUL_MAIN", "-o", exe, src],
                   check=True, capture_output=True)
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "views and chunkings agree" in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.stdout, r.stderr)
