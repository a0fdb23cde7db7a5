"""Rays for vrt_cast_rays: scenes, ray families from a fixed seed, the expected records and the host build of the row function
(voxel_rt2_amd/csrc/vrt_cast.h through tests/emul/cast_emul.cpp).  Test infrastructure shared by tests/test_cast_rays_host.py (no GPU)
and tests/test_gpu_cast_rays.py.  Everything is compared bit for bit, any NaN equal to any NaN (mismatches()).

Expected values come from the oracle alone.  For a ray with t_max = inf:
  A = Oracle.next_hit(origin, dir, shadow) on the scene           -> t, and normal / albedo / mat_id of a full hit;
  F = the same call on a context with the same parameters and no voxels -> the floor's distance f (inf: none);
  V = orc_unit_raytrace_n on world_to_voxel(origin), evaluated in float32 as orc_renderer.h:185-187 states it -> the walk's distance and cell;
  v = float32(V.distance * voxel_size).  The reference accepts the voxel iff v < closest, closest being f (pathtracer.py:203-205), so
  kind = VOXEL iff v < f, else FLOOR iff f < inf, else MISS; expected() asserts that A's t is the distance of that kind.
For a finite t_max the record is A's if t < t_max, else the miss record.  Why that is exact: the reference starts from closest = t_max
and both of its tests are strict `t < closest`, the floor's first -- (1) whatever it accepts is below t_max, and the nearer of floor
and voxel is accepted iff it is below t_max, a tie going to the floor with either start; (2) a floor at f >= t_max that it skips cannot
hide a voxel at v < t_max from the run with inf, since v < f there too.
Invalid rays (include/vrt_api.h) are never shown to the oracle: their record is the miss record."""
import contextlib
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import edit as E
import orc
import rays as R
from voxel_rt2_amd import _abi, host, scenes

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_SO = os.path.join(HERE, "emul", "_cast_emul.so")
_lib = None
RAY, HIT = _abi.RAY, _abi.HIT
INF = np.float32(np.inf)

# `tie`: floor_height exactly 48 dx - 1 with voxels standing on that plane (their bottom faces in it) and voxels hanging under it (their
# top faces in it).  `*_e0` / `*_e50`: sunlit with voxel_edges 0 and 0.5, for the darkening counts the default 0.06 does not reach.
SCENES = ("sunlit", "s1", "one_voxel", "dense", "s1_256", "empty", "tie", "sunlit_e0", "sunlit_e50")
CENSUS = ("sunlit", "s1", "dense", "s1_256")
FAMILIES = ("random", "planes", "axis", "inside", "floor", "edges", "invalid", "tmax")
TIE_FLOOR = -0.25


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "tie":
        mat, rgb = scenes.empty()
        x, z = np.meshgrid(np.arange(36, 92), np.arange(36, 92), indexing="ij")
        on = (x + z) % 3 != 0                                               # standing on the plane, the floor showing between them
        mat[x[on], 48, z[on]] = 11
        rgb[x[on], 48, z[on]] = (40, 200, 90)
        mat[96:116, 47, 40:80] = 21                                          # hanging under it
        rgb[96:116, 47, 40:80] = (200, 90, 40)
        mat[60:64, 49:53, 60:64] = 1                                         # and something to hit from the side
        rgb[60:64, 49:53, 60:64] = (90, 40, 200)
        return mat, rgb, dict(R.FLOOR, floor_height=TIE_FLOOR)
    if name in ("sunlit_e0", "sunlit_e50"):
        mat, rgb, params = R.scene("sunlit")
        return mat, rgb, dict(params, voxel_edges=0.0 if name == "sunlit_e0" else 0.5)
    return R.scene(name)


def config(name, width=16, height=8, **kw):
    mat, _, params = scene(name)
    return host.make_config(width, height, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=2, grid_res=mat.shape[0], **kw)


def families_of(name):
    if name in ("sunlit_e0", "sunlit_e50"):
        return ("edges", "inside")
    return tuple(f for f in FAMILIES if not (name == "empty" and f in ("inside", "edges")))


def cases():
    return [(s, f) for s in SCENES for f in families_of(s)]


# ---- the ray families (world units) ------------------------------------------------------------------------------------------
def _unit(rng, n):
    d = rng.standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _rays(o, d, t_max=np.inf, flags=0):
    r = np.zeros(len(o), RAY)
    with np.errstate(over="ignore", invalid="ignore"):
        r["origin"], r["dir"], r["t_max"], r["flags"] = o, d, t_max, flags
    return r


def _solids(mat, rng, n):
    """n solid voxels (array indices), or None in a grid without any"""
    solid = np.argwhere(mat > 0)
    return solid[rng.integers(0, len(solid), n)].astype(np.float64) if len(solid) else None


def _world(G, p):
    return p * (2.0 / G) - 1.0


def random_rays(rng, G, mat, fh, n=3000):
    """Origins in and around the box [-1.5, 1.5]^3, unit directions: a third anywhere, a third towards a solid voxel, a third towards a
    point of the floor disc."""
    o = rng.uniform(-1.5, 1.5, (n, 3))
    d = _unit(rng, n)
    cells = _solids(mat, rng, n)
    k = np.arange(n) % 3
    if cells is not None:
        aim = _world(G, cells + rng.uniform(0.0, 1.0, (n, 3))) - o
        d[k == 1] = (aim / np.linalg.norm(aim, axis=1, keepdims=True))[k == 1]
    ang, rad = rng.uniform(0, 2 * np.pi, n), 9.5 * np.sqrt(rng.uniform(0, 1, n))
    aim = np.stack([rad * np.cos(ang), np.full(n, fh), rad * np.sin(ang)], axis=1) - o
    d[k == 2] = (aim / np.linalg.norm(aim, axis=1, keepdims=True))[k == 2]
    o[(k == 2) & (np.arange(n) % 2 == 0), 1] = np.abs(o[(k == 2) & (np.arange(n) % 2 == 0), 1]) + fh + 0.01   # above the floor: they see it
    return _rays(o, d)


def plane_origins(rng, G, mat, n=2000):
    """One, two or three origin coordinates exactly on grid planes k dx - 1 (exact in binary32), k = 0 and k = G included."""
    o = rng.uniform(-1.0, 1.0, (n, 3))
    k = rng.integers(0, G + 1, (n, 3))
    k = np.where(rng.random((n, 3)) < 0.15, np.where(rng.random((n, 3)) < 0.5, 0, G), k)
    pinned = np.zeros((n, 3), bool)
    for j in range(n):
        pinned[j, rng.permutation(3)[:1 + j % 3]] = True
    o = np.where(pinned, k * (2.0 / G) - 1.0, o)
    d = _unit(rng, n)
    cells = _solids(mat, rng, n)
    if cells is not None:
        aim = _world(G, cells + 0.5) - o
        d[::2] = (aim / np.maximum(np.linalg.norm(aim, axis=1, keepdims=True), 1e-9))[::2]
    return _rays(o, d)


def axis_parallel(rng, G, mat, n=2000):
    """One or two direction components +0.0 or -0.0, not normalised; origins in the grid's slabs, around them, on grid planes."""
    d = rng.uniform(-1.0, 1.0, (n, 3))
    d[rng.random((n, 3)) < 0.2] *= 37.0
    zeros = np.zeros((n, 3), bool)
    zeros[np.arange(n), rng.integers(0, 3, n)] = True
    second = rng.random(n) < 0.5
    zeros[np.arange(n)[second], rng.integers(0, 3, n)[second]] = True
    d = np.where(zeros, np.where(rng.random((n, 3)) < 0.5, 0.0, -0.0), d)
    o = rng.uniform(-1.4, 1.4, (n, 3))
    cells = _solids(mat, rng, n)
    if cells is not None:                                                    # in line with a solid voxel on the axes that are left
        o = np.where(rng.random((n, 1)) < 0.6, np.where(zeros, _world(G, cells + rng.uniform(0.0, 1.0, (n, 3))), o), o)
    on_plane = rng.random((n, 3)) < 0.25
    o = np.where(on_plane, np.round((o + 1.0) * (G / 2.0)) * (2.0 / G) - 1.0, o)
    return _rays(o, d)


def inside_solids(rng, G, mat, n=1500):
    """Origins inside solid voxels: the centre, a random interior point, a point on the voxel's own face."""
    cells = _solids(mat, rng, n)
    frac = rng.uniform(0.0, 1.0, (n, 3))
    kind = rng.integers(0, 3, n)
    frac[kind == 0] = 0.5
    face = kind == 2
    frac[face, rng.integers(0, 3, int(face.sum()))] = 0.0
    return _rays(_world(G, cells + frac), _unit(rng, n) * np.where(rng.random((n, 1)) < 0.2, 3.0, 1.0))


def floor_cases(rng, fh, n=2000):
    """Origin on the plane and below it, dir.y = +-0, grazing dir.y of 1e-7 ... 1e-3, hits just inside and just outside the radius-10
    disc (pathtracer.py:183: the distance that counts is that of (x - y, z - y) from the origin, y being the plane's height)."""
    k = np.arange(n) % 5
    o = rng.uniform(-1.5, 1.5, (n, 3))
    o[:, 1] = fh + np.abs(rng.uniform(0.01, 1.5, n))
    d = _unit(rng, n)
    d[:, 1] = -np.abs(d[:, 1])
    o[k == 0, 1] = np.float32(fh)                                            # on the plane, going up and down
    d[k == 0, 1] *= rng.choice((-1.0, 1.0), int((k == 0).sum()))
    o[k == 1, 1] = fh - np.abs(rng.uniform(1e-4, 1.0, int((k == 1).sum())))    # below it, going up and down
    d[k == 1, 1] *= rng.choice((-1.0, 1.0), int((k == 1).sum()))
    d[k == 2, 1] = rng.choice((0.0, -0.0), int((k == 2).sum()))              # parallel to it
    o[(k == 2) & (np.arange(n) % 2 == 0), 1] = np.float32(fh)                # ... and in it
    g = k == 3                                                               # grazing
    d[g, 1] = -(10.0 ** rng.uniform(-7.0, -3.0, int(g.sum())))
    o[g, 1] = fh + 10.0 ** rng.uniform(-6.0, -1.0, int(g.sum()))
    e = k == 4                                                               # the disc's edge: aim at a point with |(x - y, z - y)| = 10 +- delta
    ang = rng.uniform(0, 2 * np.pi, n)
    rad = 10.0 + rng.choice((-1e-2, -1e-4, -1e-6, 1e-6, 1e-4, 1e-2), n)
    aim = np.stack([rad * np.cos(ang) + fh, np.full(n, fh), rad * np.sin(ang) + fh], axis=1)
    o[e] = (aim + np.stack([rng.uniform(-1, 1, n), rng.uniform(0.2, 2.0, n), rng.uniform(-1, 1, n)], axis=1))[e]
    d[e] = ((aim - o) / np.linalg.norm(aim - o, axis=1, keepdims=True))[e]
    return _rays(o, d)


def edge_aimed(rng, G, mat, n=3000):
    """Rays at points of solid voxels' faces that lie within a few per cent of one, two or three of the voxel's edges -- face centres,
    edges and corners -- from a little way outside the face."""
    cells = _solids(mat, rng, n)
    frac = rng.uniform(0.15, 0.85, (n, 3))
    near = rng.choice((0.01, 0.03, 0.2, 0.97, 0.99, 0.8), (n, 3))
    how = np.arange(n) % 4                                                   # coordinates near an edge besides the face's own
    for j in range(n):
        axes = rng.permutation(3)
        frac[j, axes[0]] = rng.choice((0.0, 1.0))                            # the face
        frac[j, axes[1:1 + min(how[j], 2)]] = near[j, axes[1:1 + min(how[j], 2)]]
    target = cells + frac
    out = np.where(frac == 0.0, -1.0, np.where(frac == 1.0, 1.0, 0.0))       # away from the face
    o = target + out * rng.uniform(0.3, 30.0, (n, 1)) + rng.uniform(-0.2, 0.2, (n, 3)) * np.abs(out).sum(axis=1, keepdims=True)
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return _rays(_world(G, o), d)


def invalid_rays(rng, n=400):
    """The invalid classes -- a non-finite origin or direction component, a direction of zeros, t_max NaN, 0 or negative -- and, every
    fourth ray, a valid ray next to them: a subnormal or huge component, a tiny positive or infinite t_max."""
    base = random_rays(rng, 128, np.zeros((1, 1, 1), np.int8), -0.3, n)
    bad = np.array([np.inf, -np.inf, np.nan], np.float32)
    for j in range(n):
        c = j % 8
        if c == 0:
            base["origin"][j, rng.integers(0, 3)] = bad[rng.integers(0, 3)]
        elif c == 1:
            base["dir"][j, rng.integers(0, 3)] = bad[rng.integers(0, 3)]
        elif c == 2:
            base["dir"][j] = rng.choice((0.0, -0.0), 3)
        elif c == 3:
            base["t_max"][j] = (np.nan, 0.0, -0.0, -1.0, -np.inf)[rng.integers(0, 5)]
        elif c == 4:
            base["dir"][j, rng.integers(0, 3)] = (1e-40, -1e-40, 1e20, -1e20)[rng.integers(0, 4)]
        elif c == 5:
            base["t_max"][j] = (1e-40, 1e-6, 3.0, np.inf)[rng.integers(0, 4)]
        elif c == 6:
            base["dir"][j] = rng.choice((0.0, -0.0), 3)
            base["dir"][j, rng.integers(0, 3)] = 1e-30                       # one component is enough
    return base


def tie_rays(rng, n=1200):
    """The tie scene only: dyadic origins and directions, so that the floor's distance and the voxel's are computed without rounding --
    from below onto the bottom faces of the voxels standing on the plane, from above onto the top faces of those hanging under it."""
    q = lambda a, s: np.round(a * s) / s
    o, d = np.empty((n, 3)), np.empty((n, 3))
    up = np.arange(n) % 2 == 0
    o[:, 0] = q(rng.uniform(-0.45, 0.45, n), 256)
    o[:, 2] = q(rng.uniform(-0.45, 0.45, n), 256)
    o[~up, 0] = q(rng.uniform(0.5, 0.8, int((~up).sum())), 256)              # over the hanging voxels
    o[~up, 2] = q(rng.uniform(-0.35, 0.2, int((~up).sum())), 256)
    o[:, 1] = np.where(up, TIE_FLOOR - q(rng.uniform(0.05, 0.5, n), 64), TIE_FLOOR + q(rng.uniform(0.05, 0.5, n), 64))
    d[:, 1] = np.where(up, 1.0, -1.0) * rng.choice((1.0, 0.5, 2.0), n)
    d[:, 0] = rng.choice((0.0, 0.0, 0.125, -0.125, 0.25), n)
    d[:, 2] = rng.choice((0.0, 0.0, 0.125, -0.25), n)
    return _rays(o, d)


# ---- the expectation -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracles(name):
    """(the scene's oracle, an oracle with the same parameters and no voxels)"""
    mat, rgb, params = scene(name)
    full, floor = orc.Oracle(config(name), threads=1), orc.Oracle(config(name), threads=1)
    orc.setup(full, mat, rgb, params)
    orc.setup(floor, *scenes.empty(mat.shape[0]), params)
    return full, floor


def valid(rays):
    with np.errstate(invalid="ignore"):
        return (np.isfinite(rays["origin"]).all(axis=1) & np.isfinite(rays["dir"]).all(axis=1) & (rays["dir"] != 0).any(axis=1) &
                (rays["t_max"] > 0))


def _next_hit(o, rays, idx, shadow):
    """closest[n], normal / albedo[n, 3], mat_id[n] of Oracle.next_hit for the rays idx"""
    out = np.zeros((len(rays), 9), np.float32)
    fn, ctx, buf = orc.lib().orc_unit_next_hit, C.c_void_p(o._ctx), np.zeros(9, np.float32)
    og, dr = np.ascontiguousarray(rays["origin"]), np.ascontiguousarray(rays["dir"])
    pb = orc.fptr(buf)
    for k in idx:
        fn(ctx, C.c_void_p(og.ctypes.data + 12 * int(k)), C.c_void_p(dr.ctypes.data + 12 * int(k)), int(shadow), pb)
        out[k] = buf
    return out


def expected_inf(name, rays):
    """The records for t_max = inf (flags as the rays carry them) and the darkening count of every voxel hit (-1 elsewhere)."""
    mat = scene(name)[0]
    G = mat.shape[0]
    full, floor = oracles(name)
    ok = np.flatnonzero(valid(rays))
    want = np.zeros(len(rays), HIT)
    want["t"], want["cell"] = INF, -1
    f = _next_hit(floor, rays, ok, False)[:, 0]
    half = np.float32(G // 2)
    eye = (half * rays["origin"] + half).astype(np.float32)                  # voxel_inv_size * pos - voxel_grid_offset, in float32
    walk = R.REC
    v = np.zeros(len(rays), walk)
    sel = np.ascontiguousarray(np.concatenate([eye[ok], rays["dir"][ok]], axis=1), np.float32)
    got = np.zeros(len(ok), walk)
    orc.lib().orc_unit_raytrace_n(C.c_void_p(full._ctx), len(ok), orc.fptr(sel), orc.fptr(got))
    v[ok] = got
    with np.errstate(invalid="ignore", over="ignore"):
        vt = (v["dist"] * np.float32(2.0 / G)).astype(np.float32)
        voxel = np.zeros(len(rays), bool)
        voxel[ok] = vt[ok] < f[ok]
    kind = np.where(voxel, _abi.HIT_VOXEL, np.where(np.isfinite(f), _abi.HIT_FLOOR, _abi.HIT_MISS))
    any_hit = (rays["flags"] & _abi.RAY_ANY_HIT) != 0
    a = _next_hit(full, rays, ok[~any_hit[ok]], False)
    a[ok[any_hit[ok]]] = _next_hit(full, rays, ok[any_hit[ok]], True)[ok[any_hit[ok]]]
    t_of_kind = np.where(voxel, vt, f)
    assert R.same_f32(a[ok, 0], t_of_kind[ok]).all(), f"{name}: next_hit's distance is not that of the kind derived from floor and walk"
    hit = np.zeros(len(rays), bool)
    hit[ok] = kind[ok] != _abi.HIT_MISS
    want["t"][hit], want["kind"][hit] = a[hit, 0], kind[hit]
    want["cell"][voxel] = v["cell"][voxel]
    full_hit = hit & ~any_hit
    want["normal"][full_hit], want["albedo"][full_hit], want["mat_id"][full_hit] = a[full_hit, 1:4], a[full_hit, 4:7], a[full_hit, 8].astype(np.int32)
    # census only: how many of the hit point's voxel coordinates lie within voxel_edges of an edge (voxel_world.py:47-50)
    b = np.float32(scene(name)[2]["voxel_edges"])
    with np.errstate(invalid="ignore", over="ignore"):
        uv = np.clip((eye + v["dist"][:, None] * rays["dir"]).astype(np.float32) - v["cell"].astype(np.float32), np.float32(0), np.float32(1))
        count = ((uv < b) | (uv > np.float32(1.0) - b)).sum(axis=1)
    return want, np.where(voxel, count, -1)


def miss_record(n):
    want = np.zeros(n, HIT)
    want["t"], want["cell"] = INF, -1
    return want


def with_t_max(rays, want_inf, t_max):
    """The rays with another t_max and what they expect: the record for inf if t < t_max, else the miss record (header)."""
    r = rays.copy()
    r["t_max"] = t_max
    want = want_inf.copy()
    with np.errstate(invalid="ignore"):
        gone = ~(want_inf["t"] < r["t_max"])
    want[gone] = miss_record(int(gone.sum()))
    return r, want


@functools.lru_cache(maxsize=None)
def family(name, fam):
    """(rays, expected records, darkening counts) of one family on one scene: generated once, from a seed of its own, and left alone.
    Every other ray of a family is an any-hit ray, except in `tmax`, where the flag changes every fourth."""
    mat, _, params = scene(name)
    G, fh = mat.shape[0], params["floor_height"]
    rng = np.random.default_rng([20251018, SCENES.index(name), FAMILIES.index(fam)])
    if fam == "tmax":     # the rays of `random` and `edges` that hit, with t_max just below, at and just above the oracle's t, and far off
        src = [family(name, f) for f in ("random", "edges") if f in families_of(name)]
        rays, want = np.concatenate([s[0] for s in src]), np.concatenate([s[1] for s in src])
        pick = np.flatnonzero(np.isfinite(want["t"]))[:3000]
        rays, want = rays[pick].copy(), want[pick]
        rays["flags"] = (np.arange(len(rays)) // 4) % 2
        want, count = expected_inf(name, rays)
        t = want["t"]
        choice = np.arange(len(rays)) % 4
        t_max = np.select([choice == 0, choice == 1, choice == 2], [np.nextafter(t, np.float32(0)), t, np.nextafter(t, INF)], np.float32(2.0) * t)
        rays, want = with_t_max(rays, want, t_max.astype(np.float32))
    else:
        rays = {"random": lambda: random_rays(rng, G, mat, fh), "planes": lambda: plane_origins(rng, G, mat), "axis": lambda: axis_parallel(rng, G, mat),
                "inside": lambda: inside_solids(rng, G, mat), "floor": lambda: floor_cases(rng, fh), "edges": lambda: edge_aimed(rng, G, mat),
                "invalid": lambda: invalid_rays(rng)}[fam]()
        if name == "tie" and fam == "floor":
            rays = np.concatenate([rays, tie_rays(rng)])
        rays["flags"] = np.arange(len(rays)) % 2
        want, count = expected_inf(name, rays)
        rays, want = with_t_max(rays, want, rays["t_max"])                   # (the `invalid` family carries finite ones)
    assert len(rays) <= 4000
    for a in (rays, want, count):
        a.setflags(write=False)
    return rays, want, count


def census(name):
    """Over every family of the scene: valid rays, and of their expected records voxel hits, floor hits, misses; voxel hits (full hits
    only: an any-hit ray shows no colour) by darkening count 0, 1, >= 2; exact floor / voxel ties among the valid rays."""
    out = dict(valid=0, voxel=0, floor=0, miss=0, dark0=0, dark1=0, dark2=0, ties=0)
    full, floor = oracles(name)
    for fam in families_of(name):
        rays, want, count = family(name, fam)
        ok = valid(rays)
        out["valid"] += int(ok.sum())
        for k, key in ((_abi.HIT_VOXEL, "voxel"), (_abi.HIT_FLOOR, "floor"), (_abi.HIT_MISS, "miss")):
            out[key] += int((ok & (want["kind"] == k)).sum())
        shown = (want["kind"] == _abi.HIT_VOXEL) & ((rays["flags"] & 1) == 0)
        out["dark0"] += int((shown & (count == 0)).sum())
        out["dark1"] += int((shown & (count == 1)).sum())
        out["dark2"] += int((shown & (count >= 2)).sum())
        if name == "tie" and fam == "floor":                                 # the floor's distance == the walk's, bit for bit, and the floor was kept
            G = scene(name)[0].shape[0]
            idx = np.flatnonzero(ok & (want["kind"] == _abi.HIT_FLOOR))
            eye = (np.float32(G // 2) * rays["origin"][idx] + np.float32(G // 2)).astype(np.float32)
            got = np.zeros(len(idx), R.REC)
            sel = np.ascontiguousarray(np.concatenate([eye, rays["dir"][idx]], axis=1), np.float32)
            orc.lib().orc_unit_raytrace_n(C.c_void_p(full._ctx), len(idx), orc.fptr(sel), orc.fptr(got))
            vt = (got["dist"] * np.float32(2.0 / G)).astype(np.float32)
            f = _next_hit(floor, rays, idx, False)[idx, 0]
            out["ties"] += int((vt == f).sum())
    return out


def check_census(report=print):
    """The oracle's answers alone: no comparison passes on misses, on one kind of hit or on undarkened colours alone."""
    for name in CENSUS:
        c = census(name)
        report(f"cast census {name:8s} {c}")
        for key in ("voxel", "floor", "miss"):
            assert 10 * c[key] >= c["valid"], (name, key, c)
        for key in ("dark0", "dark1", "dark2"):
            assert c[key] >= 100, (name, key, c)
    c = census("tie")
    report(f"cast census tie      {c}")
    assert c["ties"] >= 50, c
    for name, key in (("sunlit_e0", "dark0"), ("sunlit_e50", "dark2")):
        c = census(name)
        report(f"cast census {name:10s} {c}")
        assert c[key] >= 1000, (name, c)
    assert scene("tie")[2]["floor_height"] == 48 * (1 / 64) - 1
    for name in SCENES:
        rays, _, _ = family(name, "invalid") if "invalid" in families_of(name) else (np.zeros(0, RAY), None, None)
        assert name.startswith("sunlit_e") or 100 <= (~valid(rays)).sum() <= len(rays) - 100, name


# ---- comparison ----------------------------------------------------------------------------------------------------------------
def mismatches(got, want):
    """Indices of the records that differ in any field: floats by their bits, any NaN equal to any NaN."""
    bad = ~R.same_f32(got["t"], want["t"]) | (got["kind"] != want["kind"]) | (got["cell"] != want["cell"]).any(axis=1) | (got["mat_id"] != want["mat_id"])
    bad |= ~R.same_f32(got["normal"], want["normal"]).all(axis=1) | ~R.same_f32(got["albedo"], want["albedo"]).all(axis=1)
    return np.flatnonzero(bad)


def describe(rays, got, want, idx):
    return "; ".join(f"ray {k} {rays[k]} got={got[k]} want={want[k]}" for k in idx[:3])


def check(got, rays, want, label):
    bad = mismatches(got, want)
    assert bad.size == 0, f"{label}: {bad.size} of {len(rays)} records differ: {describe(rays, got, want, bad)}"


# ---- the host build of the row function -----------------------------------------------------------------------------------------
class CastScene(C.Structure):
    _fields_ = [("grid_res", C.c_int32), ("ref_oob", C.c_int32), ("floor_material", C.c_int32), ("pad", C.c_int32),
                ("floor_height", C.c_float), ("floor_color", C.c_float * 3), ("voxel_edges", C.c_float), ("cull", C.c_float * 8),
                ("grid", C.c_void_p), ("l0", C.c_void_p), ("l1", C.c_void_p), ("l2", C.c_void_p), ("l3", C.c_void_p)]


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(HERE, "emul", "cast_emul.cpp")
        csrc = os.path.join(ROOT, "voxel_rt2_amd", "csrc")
        deps = [src, os.path.join(HERE, "emul", "query_emul.h"), os.path.join(ROOT, "include", "vrt_api.h"), os.path.join(ROOT, "include", "vrt_detmath.h")]
        deps += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]   # (query_emul.h reads the sampled queries' headers too)
        if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-shared", "-Wall", "-Werror",
                            "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", _SO, src], check=True, capture_output=True)
        _lib = C.CDLL(_SO)
        _lib.cast_emul_rays.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]
        _lib.cast_emul_valid.argtypes = [C.c_void_p]
        _lib.cast_emul_staged.argtypes = [C.c_longlong, C.c_int]
        _lib.cast_emul_chunk.restype = C.c_longlong
        _lib.cast_emul_blocks.argtypes = [C.c_longlong, C.c_int, C.c_int]
        _lib.cast_emul_fetch.argtypes = [C.c_int] + [C.c_void_p] * 6
        _lib.cast_emul_poison.argtypes = [C.c_int]
        _lib.cast_emul_probe.argtypes = [C.c_void_p] * 3
        _lib.cast_emul_probe.restype = None
    return _lib


@contextlib.contextmanager
def poisoned(emul=None):
    """The emulator hands the device functions frame parameters whose unread fields are poisoned (tests/emul/query_emul.h) while this is
    open.  emul: the emulator's library and the prefix of its exports (this module's by default)."""
    so, prefix = emul or (lib(), "cast")
    was = getattr(so, prefix + "_emul_poison")(1)
    try:
        yield
    finally:
        getattr(so, prefix + "_emul_poison")(was)


def probe(scene_record, emul=None):
    """(float32[8], int32[4]) of frame_params_probe (tests/emul/query_emul.h) on the frame parameters of the emulator's current mode."""
    so, prefix = emul or (lib(), "cast")
    out, ints = np.zeros(8, np.float32), np.zeros(4, np.int32)
    getattr(so, prefix + "_emul_probe")(C.byref(scene_record), orc.fptr(out), orc.fptr(ints))
    return out, ints


def switch_over():
    """The smallest batch vrt_cast_rays walks on the staged pyramid (plan_cast_staged, vrt_plan.h)."""
    lo, hi = 0, 1 << 40
    assert not lib().cast_emul_staged(lo, -1) and lib().cast_emul_staged(hi, -1)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if lib().cast_emul_staged(mid, -1) else (mid, hi)
    return hi


class HostScene:
    """The scene as k_cast_rays reads it, built in numpy (tests/edit.py: rebuild; tests/rays.py: grown_box), for cast_emul_rays."""

    def __init__(self, name, reference_indexing=False):
        mat, rgb, params = scene(name)
        self.keep = E.rebuild(mat, rgb)
        s = self.s = CastScene()
        s.grid_res, s.ref_oob, s.floor_material = mat.shape[0], int(reference_indexing), int(params["floor_material"])
        s.floor_height, s.voxel_edges = params["floor_height"], params["voxel_edges"]
        s.floor_color[:] = params["floor_color"]
        lo, hi, active = R.grown_box(mat)
        s.cull[:] = list(lo) + list(hi) + [1.0, 0.0] if active and not reference_indexing else [-1e30] * 3 + [1e30] * 3 + [0.0, 0.0]
        for k in ("grid", "l0", "l1", "l2", "l3"):
            setattr(s, k, self.keep[k].ctypes.data)

    def cast(self, rays, staged, mode=0):
        out = np.zeros(len(rays), HIT)
        rays = np.ascontiguousarray(rays)
        assert lib().cast_emul_rays(C.byref(self.s), int(staged), int(mode), len(rays), orc.fptr(rays), orc.fptr(out)) == 0
        return out
