"""vrt_denoise: the expectation in numpy float32, builders of synthetic planes and the host build of the per-pixel functions
(voxel_rt2_amd/csrc/vrt_denoise.h through tests/emul/denoise_emul.cpp).  Test infrastructure shared by tests/test_denoise_host.py (no GPU)
and tests/test_gpu_denoise.py.  Everything is compared bit for bit, any NaN equal to any NaN; no tolerance, no pixel left out.

expected() is written from the text of include/vrt_api.h and from nothing else: the taps in the specified order (dy outside, dx inside),
one shifted-array step per tap, every expression left to right in float32.  `planes` is a dict of the arrays vrt_fetch_buffer and
vrt_fetch_hdr return: pos float32[H][W][3], normal uint16[H][W][2] (the two binary16 halves of the oct code), mat uint32[H][W][1],
hist_d / hist_s float32[H][W][4], hdr float32[H][W][3]."""
import ctypes as C
import os

import numpy as np

import radiance as X

HERE = X.HERE
ROOT = X.ROOT
f = np.float32
K = (f(0.375), f(0.25), f(0.0625))
DEFAULTS = (5, 0.25, 0.5, 64.0)                      # include/vrt_api.h: iterations, plane_tolerance, sigma_l, full_at
ROUNDING = 64.0 * 2.0 ** -24                         # relative, per iteration: 25 products, 25 sums and one division (the issue's bound)


def same_f32(a, b):
    a, b = np.ascontiguousarray(a, f), np.ascontiguousarray(b, f)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def check(got, want, label):
    bad = np.argwhere(~same_f32(got, want).all(axis=-1))
    assert bad.size == 0, (f"{label}: {len(bad)} of {want.shape[0] * want.shape[1]} pixels differ: " +
                           "; ".join(f"(v={v}, u={u}) got={got[v, u]} want={want[v, u]}" for v, u in bad[:3]))


# ---- the expectation ------------------------------------------------------------------------------------------------------------------
def dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def lum(c):
    return f(0.2125) * c[..., 0] + f(0.7154) * c[..., 1] + f(0.0721) * c[..., 2]


def oct_decode(code):
    """math_utils.py:209-215 on uint16[..][2], the two binary16 halves of a code: float32[..][3]."""
    a = np.ascontiguousarray(code, np.uint16).view(np.float16).astype(f)
    with np.errstate(all="ignore"):
        ex, ey = a[..., 0] * f(2) - f(1), a[..., 1] * f(2) - f(1)
        vz = f(1) - np.abs(ex) - np.abs(ey)
        t = np.where(-vz > 0, -vz, f(0))                                               # max(-v.z, 0); a NaN is ignored
        vx, vy = ex + np.where(ex >= 0, -t, t), ey + np.where(ey >= 0, -t, t)
        inv = f(1) / np.sqrt(vx * vx + vy * vy + vz * vz)
        return np.stack([inv * vx, inv * vy, inv * vz], axis=-1)


def unpack(planes):
    """(P, N, id, A, Hd, Hs, HDR) of the fetched planes."""
    M = np.ascontiguousarray(planes["mat"], np.uint32).reshape(planes["mat"].shape[:2])
    A = np.stack([((M >> np.uint32(sh)) & np.uint32(255)).astype(f) / f(255) for sh in (8, 16, 24)], axis=-1)
    return (np.asarray(planes["pos"], f), oct_decode(planes["normal"]), M & np.uint32(255), A, np.asarray(planes["hist_d"], f), np.asarray(planes["hist_s"], f),
            np.asarray(planes["hdr"], f))


def expected(planes, params, moving, dx):
    """float32[H][W][3]: what vrt_denoise(params = (iterations, plane_tolerance, sigma_l, full_at)) returns for the planes."""
    iterations, plane_tolerance, sigma_l, full_at = int(params[0]), f(params[1]), f(params[2]), f(params[3])
    P, N, ident, A, Hd, Hs, HDR = unpack(planes)
    H, W = ident.shape
    with np.errstate(all="ignore"):
        # 1. split and demodulate
        surface = ~(P[..., 0] * P[..., 0] + P[..., 1] * P[..., 1] + P[..., 2] * P[..., 2] < f(1e-7))
        Ap = np.fmax(A, f(0.00392156886))
        U = {"d": Hd[..., :3] if moving else Hd[..., :3] / Ap, "s": Hs[..., :3]}
        count = {"d": Hd[..., 3], "s": Hs[..., 3]}
        tol = plane_tolerance * f(dx)
        # 2. the iterations
        Xs = dict(U)
        for i in range(iterations):
            s = 1 << i
            total = {k: np.zeros((H, W, 3), f) for k in Xs}
            wsum = {k: np.zeros((H, W), f) for k in Xs}
            lp = {k: lum(Xs[k]) for k in Xs}
            for dy in range(-2, 3):
                for dx_ in range(-2, 3):
                    oy, ox = dy * s, dx_ * s
                    if abs(oy) >= H or abs(ox) >= W:
                        continue                                                       # every such tap lies outside the frame
                    p = (slice(max(0, -oy), H - max(0, oy)), slice(max(0, -ox), W - max(0, ox)))      # the centres whose tap is inside
                    q = (slice(max(0, oy), H - max(0, -oy)), slice(max(0, ox), W - max(0, -ox)))      # ... and their taps
                    ok = surface[p] & surface[q] & (ident[q] == ident[p]) & (dot3(N[p], N[q]) >= f(0.9)) & (np.abs(dot3(N[p], P[q] - P[p])) <= tol)
                    for k in Xs:
                        w = (K[abs(dx_)] * K[abs(dy)]) * count[k][q]
                        if i >= 1 and sigma_l > 0:
                            lq = lum(Xs[k][q])
                            t = np.abs(lq - lp[k][p]) / (sigma_l * ((lp[k][p] + lq) * f(0.5)) + f(0.001))
                            w = w / (f(1) + t * t)
                        total[k][p] = np.where(ok[..., None], total[k][p] + w[..., None] * Xs[k][q], total[k][p])
                        wsum[k][p] = np.where(ok, wsum[k][p] + w, wsum[k][p])
            Xs = {k: np.where((surface & (wsum[k] > 0))[..., None], total[k] / wsum[k][..., None], Xs[k]) for k in Xs}
        # 3. fade and recompose
        R = {}
        for k in Xs:
            a = np.fmin(count[k] / full_at, f(1)) if full_at > 0 else np.zeros((H, W), f)
            R[k] = Xs[k] + (U[k] - Xs[k]) * a[..., None]
        out = (R["d"] * (A if moving else Ap)) + R["s"]
        out = np.where(surface[..., None], out, HDR)
    assert out.dtype == f
    return np.ascontiguousarray(out)


# ---- synthetic planes -------------------------------------------------------------------------------------------------------------------
DX = 1.0 / 64.0
KINDS = ("edge", "apart_1", "apart_02", "two_ids", "flat")


def oct_encode(n):
    """The code of unit vector n as uint16[2] (math_utils.py:202-207), through numpy's float16 rounding (to nearest even)."""
    n = np.asarray(n, np.float64)
    n = n / np.abs(n).sum()
    x, y = n[0], n[1]
    if n[2] <= 0:
        x, y = (1 - abs(n[1])) * (1 if n[0] >= 0 else -1), (1 - abs(n[0])) * (1 if n[1] >= 0 else -1)
    return np.array([x * 0.5 + 0.5, y * 0.5 + 0.5], np.float16).view(np.uint16)


def pack_mat(ident, albedo255):
    r, g, b = (np.asarray(albedo255[..., k], np.uint32) for k in range(3))
    return (np.asarray(ident, np.uint32) | (r << np.uint32(8)) | (g << np.uint32(16)) | (b << np.uint32(24)))[..., None]


def geometry(kind, W, H, dx=DX):
    """pos, normal, id of a W x H frame whose left and right halves are two faces: `edge` a floor and a wall that meet; `apart_1` /
    `apart_02` two parallel faces 1 / 0.2 voxels apart (rejected / accepted at tolerance 0.25); `two_ids` one plane, two material ids;
    `flat` one plane.  A pixel is 0.37 voxels wide."""
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    right = u >= (W + 1) // 2
    pitch = 0.37 * dx
    pos = np.stack([0.1 + u * pitch, np.full((H, W), 0.25), -0.2 + v * pitch], axis=-1)
    up, side = oct_encode((0, 1, 0)), oct_encode((-1, 0, 0))
    normal = np.broadcast_to(up, (H, W, 2)).copy()
    ident = np.full((H, W), 11, np.uint32)
    if kind == "edge":
        edge_x = 0.1 + ((W + 1) // 2) * pitch
        pos[right] = np.stack([np.full((H, W), edge_x), 0.25 + (u - (W + 1) // 2 + 0.5) * pitch, -0.2 + v * pitch], axis=-1)[right]
        normal[right] = side
    elif kind in ("apart_1", "apart_02"):
        pos[..., 1] += np.where(right, (1.0 if kind == "apart_1" else 0.2) * dx, 0.0)
    elif kind == "two_ids":
        ident[right] = 3
    else:
        assert kind == "flat"
    return pos.astype(f), normal, ident


def synthetic(kind, W, H, seed=0, dx=DX, features=True):
    """Planes of the kind's geometry with independent noise on both signals.  features: sky holes (position 0, HDR of its own), pixels
    whose count is 0, an albedo channel of 0, counts that differ across the frame."""
    rng = np.random.default_rng(20261019 + seed)
    pos, normal, ident = geometry(kind, W, H, dx)
    albedo = rng.integers(40, 256, (H, W, 3))
    count = np.full((H, W), 4.0)
    if features:
        pos[rng.random((H, W)) < 0.06] = 0.0
        albedo[rng.random((H, W)) < 0.1, rng.integers(0, 3)] = 0
        count = rng.integers(1, 9, (H, W)).astype(np.float64)
        count[rng.random((H, W)) < 0.08] = 0.0
    hist_d = np.concatenate([rng.random((H, W, 3)) * 2.0, count[..., None]], axis=-1).astype(f)
    scount = count.copy()
    if features:
        scount[rng.random((H, W)) < 0.05] += 3.0                                       # the two signals' counts need not agree
    hist_s = np.concatenate([rng.random((H, W, 3)) * 0.3, scount[..., None]], axis=-1).astype(f)
    planes = dict(pos=pos, normal=normal, mat=pack_mat(ident, albedo), hist_d=hist_d, hist_s=hist_s, hdr=(rng.random((H, W, 3)) * 9.0 + 20.0).astype(f))
    for a in planes.values():
        a.setflags(write=False)
    return planes


def lit(geo, level_d, level_s=0.0, count=4.0, albedo=255):
    """Planes of geometry `geo` = (pos, normal, id) with constant albedo and count and the given per-pixel diffuse / specular levels."""
    pos, normal, ident = geo
    H, W = ident.shape
    one = np.ones((H, W, 1))
    hist_d = np.concatenate([np.broadcast_to(np.asarray(level_d, np.float64), (H, W))[..., None] * np.ones(3), count * one], axis=-1).astype(f)
    hist_s = np.concatenate([np.broadcast_to(np.asarray(level_s, np.float64), (H, W))[..., None] * np.ones(3), count * one], axis=-1).astype(f)
    return dict(pos=pos, normal=normal, mat=pack_mat(ident, np.full((H, W, 3), albedo)), hist_d=hist_d, hist_s=hist_s, hdr=np.zeros((H, W, 3), f))


# ---- the host build -------------------------------------------------------------------------------------------------------------------
_EMUL = os.path.join(HERE, "emul", "_denoise_emul.so")
_libs = {}


def lib():
    if "emul" not in _libs:
        so = X._build(_EMUL, os.path.join(HERE, "emul", "denoise_emul.cpp"), [os.path.join(ROOT, "voxel_rt2_amd", "csrc"), os.path.join(ROOT, "include"),
                                                                               os.path.join(HERE, "emul")],
                      ["-Werror", "-I" + os.path.join(ROOT, "voxel_rt2_amd", "csrc")])
        lib = C.CDLL(so)
        lib.denoise_emul_run.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_float, C.c_void_p]
        lib.denoise_emul_normal.argtypes = [C.c_uint32, C.c_void_p]
        lib.denoise_emul_normal.restype = None
        lib.denoise_emul_encode.argtypes = [C.c_float] * 3
        lib.denoise_emul_encode.restype = C.c_uint32
        _libs["emul"] = lib
    return _libs["emul"]


def host(planes, params, moving, dx):
    """The host build of vrt_denoise.h on the planes: float32[H][W][3]."""
    H, W = planes["mat"].shape[:2]
    arrays = [np.ascontiguousarray(planes["pos"], f), np.ascontiguousarray(planes["normal"], np.uint16), np.ascontiguousarray(planes["mat"], np.uint32),
              np.ascontiguousarray(planes["hist_d"], f), np.ascontiguousarray(planes["hist_s"], f), np.ascontiguousarray(planes["hdr"], f)]
    out = np.full((H, W, 3), np.nan, f)
    rc = lib().denoise_emul_run(W, H, *[a.ctypes.data_as(C.c_void_p) for a in arrays], int(params[0]), float(params[1]), float(params[2]), float(params[3]),
                                int(bool(moving)), float(dx), out.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return out
