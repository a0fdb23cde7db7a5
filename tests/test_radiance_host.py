"""vrt_trace_radiance on the host: the per-item functions of voxel_rt2_amd/csrc/vrt_radiance.h compiled with g++ (tests/emul/radiance_emul.cpp
drives them the way the library and its two kernels do) against the oracle's render body (tests/emul/radiance_orc.cpp), bit for bit, on
every case of tests/radiance.py and both views of the pyramid; and again with every frame parameter a query does not read poisoned: the
same bytes.  Then what the oracle's records cover (a condition, not a measurement),
the chunk plan, the fold across chunks, invalid rays, and the boundary: exports, bindings, record sizes, the error codes that need no
device."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import radiance as X
from voxel_rt2_amd import _abi, _lib

HOST_CASES = [c for c in X.CASES if c != "one_voxel_d2"]


@pytest.fixture(scope="module")
def host_scene():
    live = {}

    def get(case):
        if case not in live:
            live[case] = X.HostScene(case)
        return live[case]
    return get


def test_the_oracles_records_cover_what_they_claim():
    """Over the sunlit poses together at least a tenth of the rays hit voxels first, a tenth the floor, a tenth the sky; at depth 8 at
    least one path in a hundred is still alive at the last segment: the paths that take more voxel walks with max_depth 8 than with 7."""
    kinds = X.first_hit_kinds("sunlit_d8")
    shares = [float((kinds == k).mean()) for k in (2, 1, 0)]
    print(f"radiance census sunlit: voxel {shares[0]:.3f} floor {shares[1]:.3f} sky {shares[2]:.3f} of {kinds.size} rays")
    assert min(shares) >= 0.10, shares
    w8, w7 = X.walks("sunlit_d8", 8), X.walks("sunlit_d8", 7)
    assert (w8 >= w7).all()
    alive, total = int((w8 > w7).sum()), w8.size
    print(f"radiance census sunlit depth 8: {alive} of {total} paths alive at the last segment")
    assert 100 * alive >= total, (alive, total)
    d8 = X.expected("sunlit_d8")
    lit = np.concatenate([w[1]["rgb"] for _, w in d8.values()])
    assert (lit > 0).any(axis=1).mean() > 0.5 and np.isfinite(lit).all()


@pytest.mark.parametrize("case", HOST_CASES)
def test_host_build_equals_oracle(host_scene, case):
    h = host_scene(case)
    for pose, (rays, want) in X.expected(case).items():
        for n, rec in want.items():
            for staged in (0, 1):
                X.check(h.trace(rays, n, staged=staged), rays, rec, f"{case} pose {pose} samples {n} staged={staged}")


def test_poison_is_live(host_scene):
    """tests/test_cast_rays_host.py's check on this emulator's conversion (scene_sampled: camera_is_moving 1 plain, 0 poisoned)."""
    from test_cast_rays_host import check_probe_is_live
    h = host_scene("sunlit_d5")
    plain = X.probe(h.s)
    with X.poisoned():
        poisoned = X.probe(h.s)
    check_probe_is_live(plain, poisoned, (1, 0))
    assert X.lib().radiance_emul_poison(0) == 0


@pytest.mark.parametrize("case", HOST_CASES)
def test_poisoned_frame_parameters_change_no_byte(host_scene, case):
    """Every field of FrameParams a radiance query is not meant to read (the matrices, camera_pos, inv_res, the jitter, W, H, the rows
    and stripes, render_scale, max_accum_frames, exposure, frame; camera_is_moving flipped) poisoned: the same bytes as in the plain mode
    -- which test_host_build_equals_oracle pins to the oracle -- for every pose and sample count, on both views, in the plan's chunks
    and in chunks of one sample."""
    h = host_scene(case)
    for pose, (rays, want) in X.expected(case).items():
        for n in want:
            for staged in (0, 1):
                plain = h.trace(rays, n, staged=staged)
                with X.poisoned():
                    for per in (0, 1):
                        got = h.trace(rays, n, staged=staged, per=per)
                        assert got.tobytes() == plain.tobytes(), (f"{case} pose {pose} samples {n} staged={staged} per={per}: "
                                                                   f"{X.mismatches(got, plain).size} of {len(rays)} records differ")


def test_black_sun_and_sky_cases_are_what_they_claim():
    assert not any(X.scene("s1_black_sun")[2]["light_color"]) and X.CASES["s1_black_sun"][1] == 8
    assert X.scene("sky")[2]["use_physical_sky"] == 1 and X.config("sky").sky_res == 64
    a, b = X.expected("dense")["opposite"][1][2], X.expected("dense_ref")["opposite"][1][2]
    print(f"reference indexing dense/opposite: {X.mismatches(a, b).size} of {len(a)} records differ from the default mode's")
    sky = np.concatenate([w[2]["rgb"] for _, w in X.expected("sky").values()])
    assert (sky > 0).all(axis=1).mean() > 0.5


def test_chunk_plan_covers_every_sample_once_in_order_within_the_budget():
    lib = X.lib()
    budget = lib.radiance_emul_items()
    assert budget >= 1 << 16 and budget * 12 <= 1 << 26
    rng = np.random.default_rng(20251018)
    shapes = [(1, 1), (1, 65536), (2048, 600), (1 << 18, 4), (1 << 18, 3), (1 << 18, 65536), (budget, 2), (budget - 1, 2), (budget // 2 + 1, 5), (777, 1350)]
    shapes += [(int(rng.integers(1, 1 << 18)), int(rng.integers(1, 65537))) for _ in range(200)]
    for n, spp in shapes:
        per = lib.radiance_emul_chunk(n, spp)
        assert 1 <= per <= spp and (n * per <= budget or per == 1), (n, spp, per)
        assert per == spp or n * (per + 1) > budget, (n, spp, per)                     # as many as fit
        cut = X.chunks(n, spp)
        assert cut[0][0] == 0 and sum(c for _, c in cut) == spp and all(a + c == b for (a, c), (b, _) in zip(cut, cut[1:])), (n, spp)
        assert all(1 <= c <= per for _, c in cut)
    for n in (0, 1, 255, 1 << 18, (1 << 18) + 1, 1 << 40):
        m = lib.radiance_emul_rays(n)
        assert m == min(n, 1 << 18) and m * 1 <= budget
    assert len(X.chunks(2048, 600)) > 1                                                # what tests/test_gpu_radiance.py relies on
    assert lib.radiance_emul_staged(1 << 30, -1) and not lib.radiance_emul_staged(1, -1)


def test_fold_over_chunks_equals_fold_over_one(host_scene):
    h = host_scene("sunlit_d5")
    rays = np.concatenate([X.expected("sunlit_d5")[p][0] for p in ("default", "gap", "street")])
    whole = h.trace(rays, 7, per=7)
    for per in (1, 2, 3, 4, 6):
        assert h.trace(rays, 7, per=per).tobytes() == whole.tobytes(), per
    assert h.trace(rays, 7, per=0).tobytes() == whole.tobytes()
    # ... and is the ordered binary32 sum of the single samples, divided once
    acc = np.zeros((len(rays), 3), np.float32)
    for s in range(7):
        acc = acc + h.trace(rays, 1, first_frame=X.FIRST_FRAME + s)["rgb"]
    assert (acc / np.float32(7)).astype(np.float32).tobytes() == np.ascontiguousarray(whole["rgb"]).tobytes()
    assert (whole["rgb"] > 0).any()


def test_query_chunk_equals_the_two_former_plans():
    """plan_query_chunk(cap, n, s) under the radiance cap and under the sensor cap (radiance_emul_chunk, sensor_emul_chunk) against the
    formula the two former plan functions held, written out here."""
    import sensor as S
    assert X.lib().radiance_emul_items() == 1 << 20 and S.lib().sensor_emul_items() == (1 << 20) * 12 // 32 == 393216
    for chunk, cap in ((X.lib().radiance_emul_chunk, 1 << 20), (S.lib().sensor_emul_chunk, 393216)):
        for n in (1, 2, 255, 4096, 1 << 18):
            for spp in (1, 2, 257, 4096):
                fit = cap // n
                assert chunk(n, spp) == (1 if fit < 1 else fit if fit < spp else spp), (cap, n, spp)


def test_views_and_chunkings_agree_on_96_rays_of_5_samples(host_scene):
    """The plan's chunk, chunks of one sample and chunks of two, on both views of the pyramid: the same bytes."""
    h = host_scene("sunlit_d5")
    rays = np.concatenate([X.expected("sunlit_d5")[p][0] for p in ("default", "gap", "street")])[:96]
    assert len(rays) == 96
    whole = h.trace(rays, 5, staged=0, per=0)
    assert (whole["rgb"] > 0).any() and np.isfinite(whole["t"]).any()
    for staged in (0, 1):
        for per in (0, 1, 2):
            assert h.trace(rays, 5, staged=staged, per=per).tobytes() == whole.tobytes(), (staged, per)


def ray(o=(0.0, 0.5, 0.0), d=(0.0, -1.0, 0.0), stream=3, reserved=0):
    r = np.zeros(1, X.PATH_RAY)
    with np.errstate(invalid="ignore"):
        r["origin"], r["dir"], r["stream"], r["reserved"] = o, d, stream, reserved
    return r


def test_invalid_rays(host_scene):
    ok = lambda r: bool(X.lib().radiance_emul_valid(r.ctypes.data_as(C.c_void_p)))
    nan, inf = np.nan, np.inf
    assert ok(ray()) and ok(ray(stream=0xFFFFFFFF)) and ok(ray(d=(0.0, -0.0, 1e-40))) and ok(ray(d=(1e20, -1e20, 3e38))) and ok(ray(o=(1e30, -1e30, 0.0)))
    for bad in (nan, inf, -inf):
        for axis in range(3):
            v = [0.25, 0.5, -0.75]
            v[axis] = bad
            assert not ok(ray(o=v)) and not ok(ray(d=v)), (bad, axis)
    assert not ok(ray(d=(0.0, 0.0, 0.0))) and not ok(ray(d=(-0.0, 0.0, -0.0))) and not ok(ray(reserved=1))
    h = host_scene("sunlit_d5")
    good = X.expected("sunlit_d5")["default"][0][:5]
    mixed = np.concatenate([good[:2], ray(d=(0.0, 0.0, 0.0)), good[2:4], ray(o=(nan, 0.0, 0.0)), good[4:]])
    for staged in (0, 1):
        got = h.trace(mixed, 3, staged=staged, per=2)
        for k in (2, 5):
            assert got[k]["rgb"].tolist() == [0.0, 0.0, 0.0] and got[k]["t"] == np.float32(inf) and not np.signbit(got[k]["rgb"]).any()
        assert got[[0, 1, 3, 4, 6]].tobytes() == h.trace(good, 3, staged=staged).tobytes()     # and the rays around them are not disturbed


def test_exports_bindings_record_sizes_and_codes_without_a_device():
    assert "vrt_trace_radiance" in _lib.exported_symbols()
    assert _abi.PATH_RAY.itemsize == 32 and _abi.RADIANCE.itemsize == 16 and _abi.RADIANCE_MAX_SAMPLES == 65536
    assert [_abi.PATH_RAY.fields[k][1] for k in ("origin", "stream", "dir", "reserved")] == [0, 12, 16, 28]
    assert [_abi.RADIANCE.fields[k][1] for k in ("rgb", "t")] == [0, 12]
    lib = _lib.load()
    fn = lib.vrt_trace_radiance
    _abi.declare(lib, "vrt_")
    assert fn.restype is C.c_int and len(fn.argtypes) == 7 and fn.argtypes[1] is C.c_int64 and fn.argtypes[4] is C.c_uint32
    r, o = np.zeros(1, _abi.PATH_RAY), np.zeros(1, _abi.RADIANCE)
    assert fn(None, 1, r.ctypes.data_as(C.c_void_p), 1, 0, o.ctypes.data_as(C.c_void_p), 0) == _abi.VRT_E_INVALID
    assert b"null" in lib.vrt_last_error()


def test_emulation_program_under_sanitizers(tmp_path):
    """tests/emul/radiance_emul.cpp as a stand-alone program (-DRADIANCE_EMUL_MAIN: a scene of its own, both views, two chunkings) built
    with the address and undefined-behaviour sanitizers and run: the per-item functions, the chunk loop and the fold touch no memory
    they should not and rely on no undefined arithmetic."""
    exe = str(tmp_path / "radiance_emul_san")
    src = os.path.join(X.HERE, "emul", "radiance_emul.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-Wall", "-Werror", "-Wno-unused-function",
                    "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DRADIANCE_EMUL_MAIN", "-o", exe, src],
                   check=True, capture_output=True)
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "views and chunkings agree" in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.stdout, r.stderr)


def test_tone_map_follows_the_reference_curve():
    """Renderer.tone_map -- the presentation of images that do not come from the camera -- against the reference's own uchimura values
    (tests/golden/reference/functions.npz, recorded from math_utils.py:163-186): exposure, the curve, gamma 2.2, clamped to [0, 1].  The
    bound: the recorded values are binary32 results of about ten binary32 operations (relative error of a few 2^-24 each, the power of
    1.33 and the gamma leave it below 1e-6 of a value in [0, 1]); tone_map computes in double and rounds once.  1e-6 is 1/4000 of an
    8-bit level."""
    from voxel_rt2_amd.renderer import Renderer
    v = np.load(os.path.join(X.HERE, "golden", "reference", "functions.npz"))
    x, y = v["uchimura_in"], v["uchimura_out"]
    ok = np.isfinite(x) & (x >= 0) & np.isfinite(y)
    assert ok.sum() >= 100 and x[ok].max() > 1.0 and (x[ok] < 0.22).any()               # toe, linear part and shoulder
    want = np.clip(np.power(np.clip(y[ok].astype(np.float64), 0.0, None), 1.0 / 2.2), 0.0, 1.0)
    for exposure in (1.0, 2.0):
        me = types.SimpleNamespace(exposure=exposure)
        hdr = np.repeat((x[ok] / np.float32(exposure))[:, None], 3, axis=1).reshape(-1, 1, 3)
        exact = (hdr[:, 0, 0] * np.float32(exposure)) == x[ok]                           # where the division by the exposure loses nothing
        got = Renderer.tone_map(me, hdr)
        assert got.shape == (int(ok.sum()), 1, 4) and got.dtype == np.float32 and (got[..., 3] == 1).all() and exact.sum() >= 100
        assert np.abs(got[exact, 0, :3] - want[exact, None]).max() <= 1e-6
    odd = Renderer.tone_map(types.SimpleNamespace(exposure=1.0), np.array([[[-1.0, np.inf, 0.0]]], np.float32))[0, 0]
    assert odd.tolist() == [0.0, 1.0, 0.0, 1.0]                                          # negative light is black, unbounded light white
