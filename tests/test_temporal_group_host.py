"""temporal_group_pixel (the accumulation of several render launches in one pass, voxel_rt2_amd/csrc/vrt_temporal.h) against the
passes it stands for: K consecutive temporal_pixel passes with the histories and HDR buffers swapped between them.  Both are the
product's device headers compiled for the host (tests/emul/group_emul.cpp); every stored value is compared as uint32.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_SO = os.path.join(HERE, "emul", "_group_emul.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(HERE, "emul", "group_emul.cpp")
        csrc = os.path.join(ROOT, "voxel_rt2_amd", "csrc")
        deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
        if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
            # the flags of tests/emu.py
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-shared",
                            "-Wno-unknown-pragmas", "-o", _SO, src], check=True, capture_output=True)
        _lib = C.CDLL(_SO)
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _awkward(rng, a, frac=0.03):
    """NaN, +-inf, negative values and -0 sprinkled over a float32 array."""
    flat = a.reshape(-1)
    specials = np.array([np.nan, np.inf, -np.inf, -1.5, -1e-30, -0.0, 0.0, 1e30], dtype=np.float32)
    n = max(1, int(flat.size * frac))
    flat[rng.integers(0, flat.size, n)] = specials[rng.integers(0, specials.size, n)]
    return a


def make_case(seed, W, H, row0, row1, g, skip_slices=()):
    """Random planes for len(g) slices.  Slices in `skip_slices` carry matrices under which exactly the pixels whose depth is 0.5
    unproject to the origin (the near_zero3 branch), and a third of their pixels have that depth."""
    rng = np.random.default_rng(seed)
    K, npix = len(g), (row1 - row0) * W
    f32 = np.float32
    view_inv = np.zeros((K, 16), f32)
    proj_inv = np.zeros((K, 16), f32)
    depth = rng.uniform(0.55, 0.999, (K, npix)).astype(f32)
    for s in range(K):
        # a jittered projection and a camera of its own per slice
        if s in skip_slices:
            p = np.zeros((4, 4), f32)
            p[:3, 2] = rng.uniform(0.5, 2.0, 3)     # xyz = c * (2 depth - 1): zero at depth 0.5 only
            p[3, 3] = 1.0
            vm = np.zeros((4, 4), f32)
            vm[:3, :3] = rng.normal(size=(3, 3))
            vm[3, 3] = 1.0                           # no translation: the origin stays the origin
            depth[s, rng.random(npix) < 0.33] = 0.5
        else:
            p = (np.eye(4) + rng.normal(scale=0.2, size=(4, 4))).astype(f32)
            p[3] = (rng.normal(scale=0.01), rng.normal(scale=0.01), rng.normal(scale=0.1), 1.0)
            vm = (np.eye(4) + rng.normal(scale=0.3, size=(4, 4))).astype(f32)
            vm[:3, 3] = rng.normal(scale=2.0, size=3)
        proj_inv[s] = p.reshape(-1)
        view_inv[s] = vm.reshape(-1)
    col_d = _awkward(rng, rng.uniform(0.0, 4.0, (K, 4, npix, 3)).astype(f32))
    col_s = _awkward(rng, rng.uniform(0.0, 4.0, (K, 4, npix, 3)).astype(f32))
    refl = rng.uniform(0.0, 30.0, (K, 4, npix)).astype(f32)
    refl[rng.random(refl.shape) < 0.4] = 0.0          # "no reflection": left out of the window's mean
    refl = _awkward(rng, refl, 0.01)
    hist_d = rng.uniform(0.0, 4.0, (npix, 4)).astype(f32)
    hist_s = rng.uniform(0.0, 4.0, (npix, 4)).astype(f32)
    hist_d[:, 3] = rng.integers(0, 40, npix)          # running sample counts, fresh pixels (0) among them
    hist_s[:, 3] = rng.integers(0, 40, npix)
    max_accum = rng.choice(np.array([8.0, 16.0, 32.0, 1e9], f32), K).astype(f32)
    return dict(W=W, H=H, row0=row0, row1=row1, g=np.asarray(g, np.int32), view_inv=view_inv, proj_inv=proj_inv, max_accum=max_accum,
                col_d=col_d, col_s=col_s, depth=depth, refl=refl, hist_d=hist_d, hist_s=hist_s)


def run(case, r0, r1, grouped):
    npix = (case["row1"] - case["row0"]) * case["W"]
    out = [np.full((npix, 4), 7.0, np.float32), np.full((npix, 4), 7.0, np.float32), np.full((npix, 3), 7.0, np.float32),
           np.full((npix,), 7.0, np.float32)]
    rc = lib().tg_run(case["W"], case["H"], case["row0"], case["row1"], r0, r1, len(case["g"]), _ptr(case["g"]), _ptr(case["view_inv"]),
                      _ptr(case["proj_inv"]), _ptr(case["max_accum"]), _ptr(case["col_d"]), _ptr(case["col_s"]), _ptr(case["depth"]),
                      _ptr(case["refl"]), _ptr(case["hist_d"]), _ptr(case["hist_s"]), int(grouped), *[_ptr(o) for o in out])
    assert rc == 0
    return out


def check(case, r0, r1):
    single, grouped = run(case, r0, r1, False), run(case, r0, r1, True)
    for name, a, b in zip(("diffuse history", "specular history", "HDR", "filtered reflection depth"), single, grouped):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{name} differs"
    return single


G_OF = {1: (3,), 2: (4, 1), 3: (2, 4, 3), 4: (1, 4, 2, 3), 8: (4, 1, 3, 2, 4, 4, 1, 2)}   # mixed sample counts per slice


@pytest.mark.parametrize("K", [1, 2, 3, 4, 8])
def test_group_equals_consecutive_passes(K):
    assert lib().tg_max_group() >= 8
    # 67 columns: more than a wave's 64 would cover, edge columns and rows included (the whole frame is processed)
    case = make_case(100 + K, 67, 21, 0, 21, G_OF[K])
    single = check(case, 0, 21)
    assert not np.array_equal(single[0].view(np.uint32), case["hist_d"].view(np.uint32))   # (the passes did something)


@pytest.mark.parametrize("K", [2, 3, 4, 8])
def test_group_with_skipped_pixels_in_some_slices(K):
    skip = {2: (0,), 3: (1,), 4: (0, 3), 8: (2, 5, 7)}[K]   # the last slice among them for K = 4 and 8: HDR = its scrubbed sample
    case = make_case(200 + K, 40, 17, 0, 17, G_OF[K], skip_slices=skip)
    single = check(case, 0, 17)
    # the branch was taken for some pixels of the last skipping slice and not for others
    s = skip[-1]
    skipped = case["depth"][s] == np.float32(0.5)
    assert skipped.any() and not skipped.all()


@pytest.mark.parametrize("K", [1, 2, 3, 4, 8])
def test_group_on_a_row_shard(K):
    # buffers hold rows 6..20 of a 32-row frame (own rows 8..18 + a 2-row halo), the passes run over the own rows
    case = make_case(300 + K, 33, 32, 6, 20, G_OF[K], skip_slices=(0,) if K > 1 else ())
    check(case, 8, 18)


def test_group_of_one_sample_slices():
    # the reference's loop shape: one sample per launch, a new jitter (matrices) each
    case = make_case(400, 64, 9, 0, 9, (1,) * 8)
    check(case, 0, 9)
