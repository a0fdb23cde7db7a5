"""vrt_cast_rays on the host: the row function of voxel_rt2_amd/csrc/vrt_cast.h compiled with g++ (tests/emul/cast_emul.cpp runs the
loop of k_cast_rays) against the oracle's next_hit -- every ray family on every scene of tests/cast.py, both views of the pyramid,
any-hit rays as a wave of like rays and as part of a mixed wave, the reference's indexing off and on; and all of it again with every
frame parameter a cast does not read poisoned: the same bytes.  Then the validity gate on literal
rays, the switch-over and grid-size functions, the boundary (exports, bindings, record sizes, NULL-context codes) and the box
arithmetic of vrt_fetch_voxels against numpy slices."""
import ctypes as C

import numpy as np
import pytest

import cast as K
import edit as E
import rays as R
from voxel_rt2_amd import _abi, _lib


@pytest.fixture(scope="module")
def host_scene():
    live = {}

    def get(name, reference_indexing=False):
        if (name, reference_indexing) not in live:
            live[name, reference_indexing] = K.HostScene(name, reference_indexing)
        return live[name, reference_indexing]
    return get


def test_families_are_what_they_claim():
    K.check_census()


@pytest.mark.parametrize("scene,fam", K.cases())
def test_row_function_equals_oracle(host_scene, scene, fam):
    rays, want, _ = K.family(scene, fam)
    for staged in (0, 1):
        for mode in (0, 1):
            K.check(host_scene(scene).cast(rays, staged, mode), rays, want, f"{scene}/{fam} staged={staged} mode={mode}")


@pytest.mark.parametrize("scene", ["sunlit", "dense", "s1_256"])
def test_row_function_with_reference_indexing(host_scene, scene):
    """With the reference's reading of cells outside the grid the oracle is asked in that mode too, and nothing is culled.  (The modes
    differ on rays that leave a dense grid a rounding error short of its far face; how many of these rays do is printed, not asserted:
    tests/test_ray_probe.py pins that reading on the reference's own recorded rays.)"""
    full, _ = K.oracles(scene)
    rays = np.concatenate([K.family(scene, f)[0] for f in ("random", "planes", "axis")])
    plain = np.concatenate([K.family(scene, f)[1] for f in ("random", "planes", "axis")])
    full._lib.orc_set_reference_indexing(C.c_void_p(full._ctx), 1)
    try:
        want_inf, _ = K.expected_inf(scene, rays)
        _, want = K.with_t_max(rays, want_inf, rays["t_max"])
    finally:
        full._lib.orc_set_reference_indexing(C.c_void_p(full._ctx), 0)
    G = K.scene(scene)[0].shape[0]
    outside = ((want["cell"] < -1) | (want["cell"] >= G) | ((want["cell"] == -1) & (want["kind"][:, None] == _abi.HIT_VOXEL))).any(axis=1)
    print(f"reference indexing {scene}: {K.mismatches(want, plain).size} of {len(rays)} records differ from the default mode's, {int(outside.sum())} hits outside the grid")
    for staged in (0, 1):
        K.check(host_scene(scene, True).cast(rays, staged), rays, want, f"{scene} reference indexing staged={staged}")


def check_probe_is_live(plain, poisoned, moving):
    """frame_params_probe (tests/emul/query_emul.h) in the two modes: functions that read what no query reads tell them apart.
    camera_ray_dir, pixel_texcoord and the three plain floats are NaN on the poisoned record; launch_tile_rows reads the stripe fields'
    poison where the plain record gives 0 rows; W, frame and camera_is_moving hold their poison.  moving: (plain, poisoned) values of
    camera_is_moving for this emulator's conversion."""
    (pf, pi), (qf, qi) = plain, poisoned
    assert np.isnan(qf).all(), qf
    assert pi.tolist() == [0, 0, 0, moving[0]] and qi.tolist() == [0x7FFFFFFF, 0x7FFFFFFF, -1, moving[1]], (pi, qi)
    assert (pf[5:] == 0).all()                                              # exposure, max_accum_frames, camera_pos.y of the plain record


def test_poison_is_live(host_scene):
    h = host_scene("sunlit")
    plain = K.probe(h.s)
    with K.poisoned():
        poisoned = K.probe(h.s)
    check_probe_is_live(plain, poisoned, (0, 1))
    assert K.lib().cast_emul_poison(0) == 0                                 # and the mode is back to plain


@pytest.mark.parametrize("scene,fam", K.cases())
def test_poisoned_frame_parameters_change_no_byte(host_scene, scene, fam):
    """Every field of FrameParams a cast is not meant to read (the camera, the pixel grid, the launch's rows and stripes, the frame
    counter, the light, the sky switch, ...) poisoned: the same bytes as with those fields zero, for every family, both views of the
    pyramid and both ways a wave treats any-hit rays.  (The plain mode is what test_row_function_equals_oracle pins to the oracle.)"""
    rays, _, _ = K.family(scene, fam)
    h = host_scene(scene)
    for staged in (0, 1):
        for mode in (0, 1):
            plain = h.cast(rays, staged, mode)
            with K.poisoned():
                got = h.cast(rays, staged, mode)
            assert got.tobytes() == plain.tobytes(), f"{scene}/{fam} staged={staged} mode={mode}: {K.mismatches(got, plain).size} of {len(rays)} records differ"


@pytest.mark.parametrize("scene", ["sunlit", "dense", "s1_256"])
def test_poisoned_frame_parameters_change_no_byte_with_reference_indexing(host_scene, scene):
    rays = np.concatenate([K.family(scene, f)[0] for f in ("random", "planes", "axis")])
    h = host_scene(scene, True)
    for staged in (0, 1):
        plain = h.cast(rays, staged)
        with K.poisoned():
            got = h.cast(rays, staged)
        assert got.tobytes() == plain.tobytes(), f"{scene} staged={staged}: {K.mismatches(got, plain).size} of {len(rays)} records differ"


def ray(o=(0.0, 0.5, 0.0), d=(0.0, -1.0, 0.0), t_max=np.inf, flags=0):
    r = np.zeros(1, K.RAY)
    with np.errstate(invalid="ignore"):
        r["origin"], r["dir"], r["t_max"], r["flags"] = o, d, t_max, flags
    return r


def test_validity_gate_on_literal_rays():
    ok = lambda r: bool(K.lib().cast_emul_valid(r.ctypes.data_as(C.c_void_p)))
    nan, inf = np.nan, np.inf
    assert ok(ray()) and ok(ray(t_max=1e-40)) and ok(ray(t_max=3.0)) and ok(ray(flags=1)) and ok(ray(flags=0xFFFFFFFF))
    assert ok(ray(d=(0.0, -0.0, 1e-40))) and ok(ray(d=(1e20, -1e20, 3e38))) and ok(ray(o=(1e30, -1e30, 0.0)))
    for bad in (nan, inf, -inf):
        for axis in range(3):
            v = [0.25, 0.5, -0.75]
            v[axis] = bad
            assert not ok(ray(o=v)) and not ok(ray(d=v)), (bad, axis)
    assert not ok(ray(d=(0.0, 0.0, 0.0))) and not ok(ray(d=(-0.0, 0.0, -0.0)))
    for t in (nan, 0.0, -0.0, -1e-40, -1.0, -inf):
        assert not ok(ray(t_max=t)), t
    # what an invalid ray gets, and a valid one that finds nothing nearer than t_max: the miss record of include/vrt_api.h
    h = K.HostScene("sunlit")
    for r in (ray(d=(0.0, 0.0, 0.0)), ray(t_max=nan), ray(o=(0.0, 0.5, 0.0), d=(0.0, 1.0, 0.0)), ray(t_max=1e-3)):
        for staged in (0, 1):
            got = h.cast(r, staged)[0]
            assert got.tobytes() == K.miss_record(1)[0].tobytes(), (r, got)
    # and one known hit: straight down onto the top of a sunlit block (voxel y = 56 is the top layer of the block at x, z = 64..69)
    got = h.cast(ray(o=(66.5 / 64 - 1, 0.5, 66.25 / 64 - 1)), 0)[0]
    assert got["kind"] == _abi.HIT_VOXEL and got["cell"].tolist()[0::2] == [66, 66] and got["normal"].tolist() == [0.0, 1.0, 0.0] and got["mat_id"] > 0
    assert np.float32(0.5) - got["t"] == np.float32((got["cell"][1] + 1) / 64 - 1)
    shadow = h.cast(ray(o=(66.5 / 64 - 1, 0.5, 66.25 / 64 - 1), flags=1), 0)[0]
    assert shadow["t"] == got["t"] and shadow["cell"].tolist() == got["cell"].tolist() and shadow["kind"] == got["kind"]
    assert shadow["normal"].tolist() == shadow["albedo"].tolist() == [0.0, 0.0, 0.0] and shadow["mat_id"] == 0


def test_switch_over_and_grid_size():
    lib = K.lib()
    n0 = K.switch_over()
    assert n0 >= 1 and not lib.cast_emul_staged(n0 - 1, -1) and lib.cast_emul_staged(n0, -1) and lib.cast_emul_staged(1 << 40, -1)
    assert not lib.cast_emul_staged(1, -1)                                  # a pick never pays for staging
    assert lib.cast_emul_staged(1, 1) and not lib.cast_emul_staged(1 << 30, 0)   # the development switch overrides
    assert lib.cast_emul_chunk() >= 256 and lib.cast_emul_chunk() * 80 <= 1 << 26
    assert lib.cast_emul_blocks(1, 256, 4) == 1 and lib.cast_emul_blocks(256, 256, 4) == 1 and lib.cast_emul_blocks(257, 256, 4) == 2
    assert lib.cast_emul_blocks(1 << 24, 256, 4) == 1024 and lib.cast_emul_blocks(1 << 40, 256, 7) == 1792
    assert lib.cast_emul_blocks(1 << 24, 256, 0) == 256


def test_exports_bindings_and_record_sizes():
    assert {"vrt_cast_rays", "vrt_fetch_voxels"} <= set(_lib.exported_symbols())
    assert _abi.RAY.itemsize == 32 and _abi.HIT.itemsize == 48
    assert [_abi.RAY.fields[k][1] for k in ("origin", "t_max", "dir", "flags")] == [0, 12, 16, 28]
    assert [_abi.HIT.fields[k][1] for k in ("t", "kind", "cell", "normal", "albedo", "mat_id")] == [0, 4, 8, 20, 32, 44]
    assert (_abi.HIT_MISS, _abi.HIT_FLOOR, _abi.HIT_VOXEL, _abi.RAY_ANY_HIT) == (0, 1, 2, 1)
    lib = _lib.load()
    cast, fetch = lib.vrt_cast_rays, lib.vrt_fetch_voxels
    assert cast.restype is C.c_int and len(cast.argtypes) == 5 and cast.argtypes[1] is C.c_int64
    assert fetch.restype is C.c_int and len(fetch.argtypes) == 6
    r, h = np.zeros(1, _abi.RAY), np.zeros(1, _abi.HIT)
    assert cast(None, 1, r.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p), 0) == _abi.VRT_E_INVALID
    assert b"null" in lib.vrt_last_error()
    lo, hi = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(1, 1, 1)
    m, c = np.zeros((1, 1, 1), np.int8), np.zeros((1, 1, 1, 3), np.uint8)
    assert fetch(None, lo, hi, m.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), 0) == _abi.VRT_E_INVALID
    assert b"null" in lib.vrt_last_error()


def fetch(mat, rgb, lo, hi):
    shape = tuple(max(h - l, 0) for l, h in zip(lo, hi))
    bm, bc = np.full(shape, 99, np.int8), np.full(shape + (3,), 99, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lo_, hi_ = np.array(lo, np.int32), np.array(hi, np.int32)
    rc = K.lib().cast_emul_fetch(mat.shape[0], p(lo_), p(hi_), p(mat), p(rgb), p(bm) if bm.size else None, p(bc) if bc.size else None)
    return rc, bm, bc


@pytest.mark.parametrize("name", E.SEQUENCES)
def test_fetch_box_arithmetic_on_the_named_boxes(name):
    mat, rgb = E.grids(name)[-1]
    for lo, hi, _, _ in E.sequence(name)[1]:
        if E.touched(lo, hi, 0) > 64 ** 3:
            lo, hi = tuple(l + 3 for l in lo), tuple(l + 3 + s for l, s in zip(lo, (40, 7, 33)))      # (a part of the whole-grid boxes)
        rc, bm, bc = fetch(mat, rgb, lo, hi)
        s = tuple(slice(l, h) for l, h in zip(lo, hi))
        assert rc == 0 and bm.tobytes() == mat[s].tobytes() and bc.tobytes() == rgb[s].tobytes(), (name, lo, hi)


@pytest.mark.parametrize("G,base,n,seed", [(128, "sunlit", 120, 1), (256, "s1_256", 16, 3)])
def test_fetch_box_arithmetic_on_random_boxes(G, base, n, seed):
    from test_voxel_edit_host import random_box
    rng = np.random.default_rng([20251018, seed])
    mat, rgb = R.scene(base)[:2]
    for _ in range(n):
        lo, hi = random_box(rng, G)
        rc, bm, bc = fetch(mat, rgb, lo, hi)
        s = tuple(slice(l, h) for l, h in zip(lo, hi))
        assert rc == 0 and bm.tobytes() == mat[s].tobytes() and bc.tobytes() == rgb[s].tobytes(), (lo, hi)
    for lo, hi in (((-1, 0, 0), (0, 1, 1)), ((0, 0, G), (1, 1, G + 1)), ((5, 5, 5), (6, 4, 6))):
        assert fetch(mat, rgb, lo, hi)[0] == -1, (lo, hi)
