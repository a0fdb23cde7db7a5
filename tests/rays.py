"""Single rays for the walk probes (vrt_trace_probe on the device, emu_trace_probe on the host build of the same code): scenes, ray
families from a fixed seed, the oracle's answers (orc_unit_raytrace_n) and the comparison rules.  Test infrastructure shared by
tests/test_ray_probe.py (no GPU) and tests/test_gpu_ray_probe.py.

Everything is compared bit for bit, any NaN equal to any NaN.  Rules (those of test_oracle_rays_equal_reference_source):
  box off: distance bits and step count on every ray; cell and normal where the distance is finite -- on a miss they are whatever
           the last step left outside the grid, where the default mode reads "empty" and nothing downstream looks;
  box on : distance bits on every ray, cell and normal where the distance is finite; no step counts (culling shortens walks);
  the three walks (branchy, flat, record) agree with each other on every field of every ray, box on and box off;
  box on, on the scenes of CULLING, the box-aimed family: some rays that the walk steps through come back culled as include/vrt_api.h
           says (distance inf, cell -1, normal 0, 0 steps); at grid 128 the walks take fewer steps in all, at 256 every ray that is
           not culled whole takes exactly the steps it takes with the box off."""
import ctypes as C
import functools
import os

import numpy as np

import orc
from voxel_rt2_amd import host, scenes

HERE = os.path.dirname(os.path.abspath(__file__))
REC = np.dtype([("dist", np.float32), ("cell", np.int32, 3), ("normal", np.float32, 3), ("iters", np.int32)])
assert REC.itemsize == 32
WALKS = {"branchy": 0, "flat": 1, "record": 2}
BOX = 4
SCENES = ("sunlit", "s1", "dense", "sponge256", "empty", "one_voxel", "s1_256")
# the scenes whose grown box lies inside the grid and is a box: rays are culled there (at 256^3 whole rays only).  Not `dense` and
# `sponge256` (the box holds the grid: cull[6] == 0) and not `empty`: its lo = 2^20 - 8 > hi reads as a huge box in cull_ray's
# min / max, so its rays are walked (and miss)
CULLING = ("sunlit", "s1", "one_voxel", "s1_256")
FAMILIES = ("axis", "boundary", "box", "odd", "long")
DELTAS = (1e-5, 1e-4, 1e-3, 1e-2, 1.0)
FLOOR = dict(exposure=1.0, voxel_edges=0.06, floor_height=-0.3, floor_color=(0.7, 0.6, 0.5), floor_material=1,
             background_color=(0.2, 0.3, 0.5), light_direction=(0.3, 1.0, 0.2), light_cone=0.1, light_color=(1.0, 0.9, 0.8),
             use_physical_sky=0, use_clouds=0)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(mat, rgb, params): the builders of voxel_rt2_amd.scenes; `empty` and `one_voxel` as test_degenerate_grids builds them."""
    if name in ("empty", "one_voxel"):
        mat, rgb = scenes.empty()
        if name == "one_voxel":
            mat[127, 64, 0] = 11
            rgb[127, 64, 0] = (255, 64, 32)
        return mat, rgb, FLOOR
    return scenes.SCENES[name](0)


def config(name):
    mat, _, params = scene(name)
    return host.make_config(16, 8, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=2, grid_res=mat.shape[0])


def grown_box(mat):
    """k_cull_box (vrt_scene_kernels.hip) from the voxel array: bounds of the solids at 4x4x4 brick granularity, +- 8 voxels.
    Returns lo[3], hi[3] (lo > hi without solids) and whether the box leaves part of the grid out (cull[6])."""
    G = mat.shape[0]
    bricks = (mat > 0).reshape(G // 4, 4, G // 4, 4, G // 4, 4).any(axis=(1, 3, 5))
    lo, hi = np.full(3, float(1 << 20) - 8.0), np.full(3, -float(1 << 20) + 8.0)
    for a in range(3):
        idx = np.flatnonzero(bricks.any(axis=tuple(k for k in range(3) if k != a)))
        if idx.size:
            lo[a], hi[a] = idx[0] * 4 - 8.0, idx[-1] * 4 + 4 + 8.0
    return lo, hi, bool((lo > 0).any() or (hi < G).any())


def _unit(rng, n):
    d = rng.standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _rays(o, d):
    return np.ascontiguousarray(np.concatenate([o, d], axis=1), dtype=np.float32)


def axis_parallel(rng, G, n=3000):
    """One or two direction components +0.0 or -0.0; origins inside the grid's slabs, outside them, and (a third of the
    coordinates) exactly on integer planes, 0 and G among them."""
    d = rng.uniform(-1.0, 1.0, (n, 3))
    d[rng.random((n, 3)) < 0.2] *= 37.0                                   # not normalised
    zeros = np.zeros((n, 3), bool)
    zeros[np.arange(n), rng.integers(0, 3, n)] = True
    second = rng.random(n) < 0.4
    zeros[np.arange(n)[second], rng.integers(0, 3, n)[second]] = True
    d = np.where(zeros, np.where(rng.random((n, 3)) < 0.5, 0.0, -0.0), d)
    o = rng.uniform(-0.3 * G, 1.3 * G, (n, 3))
    inside = rng.random(n) < 0.5
    o[inside] = rng.uniform(0.0, G, (int(inside.sum()), 3))
    on_plane = rng.random((n, 3)) < 1.0 / 3.0
    o = np.where(on_plane, np.round(o), o)
    face = rng.random((n, 3)) < 0.05
    o = np.where(face, np.where(rng.random((n, 3)) < 0.5, 0.0, float(G)), o)
    return _rays(o, d)


def boundary_origins(rng, G, mat, n=3000):
    """Origins exactly on cell boundaries; on the grid's faces, edges and corners (one, two or three coordinates 0 or G); inside
    solid voxels (centre, random interior point, a point on the voxel's own face)."""
    k = n // 3
    o1 = rng.uniform(0.0, G, (k, 3))
    o1 = np.where(rng.random((k, 3)) < 0.6, np.round(o1), o1)
    o2 = rng.uniform(0.0, G, (k, 3))
    pinned = np.zeros((k, 3), bool)
    for j in range(k):
        pinned[j, rng.permutation(3)[:1 + j % 3]] = True
    o2 = np.where(pinned, np.where(rng.random((k, 3)) < 0.5, 0.0, float(G)), np.where(rng.random((k, 3)) < 0.5, np.round(o2), o2))
    solid = np.argwhere(mat > 0)
    if len(solid):
        cells = solid[rng.integers(0, len(solid), n - 2 * k)].astype(np.float64)
        frac = rng.uniform(0.0, 1.0, cells.shape)
        kind = rng.integers(0, 3, len(cells))
        frac[kind == 0] = 0.5
        on_face = kind == 2
        frac[on_face, rng.integers(0, 3, int(on_face.sum()))] = 0.0
        o3 = cells + frac
    else:
        o3 = np.round(rng.uniform(0.0, G, (n - 2 * k, 3)))
    o = np.concatenate([o1, o2, o3])
    return _rays(o, _unit(rng, len(o)) * np.where(rng.random((len(o), 1)) < 0.2, 5.0, 1.0))


def box_aimed(rng, G, mat, n=4000):
    """Rays through points on the faces, edges and corners of the grown box, displaced from them by +-1e-5 ... +-1 voxel, from
    origins inside the box, between box and grid, and outside the grid.  Where the box is not a box inside the grid (no solids:
    lo > hi; a dense grid: it holds the grid, cull[6] == 0) the grid's own faces stand in for it."""
    lo, hi, active = grown_box(mat)
    if (lo > hi).any() or not active:
        lo, hi = np.zeros(3), np.full(3, float(G))
    target = rng.uniform(lo, hi, (n, 3))
    pinned = np.zeros((n, 3), bool)
    for j in range(n):
        pinned[j, rng.permutation(3)[:1 + j % 3]] = True                   # face, edge, corner in turn
    side = np.where(rng.random((n, 3)) < 0.5, lo, hi)
    delta = rng.choice(DELTAS, (n, 3)) * rng.choice((-1.0, 1.0), (n, 3))
    target = np.where(pinned, side + delta, target)
    glo, ghi = np.minimum(lo, 0.0), np.maximum(hi, float(G))
    solid = np.argwhere(mat > 0)
    kind = np.arange(n) % 4
    o = np.empty((n, 3))
    for j in range(n):
        for _ in range(64):
            if kind[j] == 0:                                                # inside the box
                p = rng.uniform(lo, hi)
                break
            if kind[j] == 1:                                                # between box and grid (anywhere in the grid if the box holds it)
                p = rng.uniform(0.0, G, 3)
                if ((p < lo) | (p > hi)).any() or ((lo <= 0).all() and (hi >= G).all()):
                    break
            elif kind[j] == 2 or not len(solid):                            # outside the grid
                p = rng.uniform(glo - 0.5 * G, ghi + 0.5 * G)
                if ((p < 0) | (p > G)).any():
                    break
            else:                                                           # in line with the target and a solid voxel behind it: inside or outside the grid
                p = target[j] - (solid[rng.integers(0, len(solid))] + 0.5 - target[j]) * rng.uniform(0.1, 2.0)
                break
        o[j] = p
    d = target - o
    unit = rng.random(n) < 0.5
    d[unit] /= np.linalg.norm(d[unit], axis=1, keepdims=True)
    return _rays(o, d)


def odd_directions(rng, G, mat, n=2000):
    """Directions that are not unit vectors (lengths 1e-3 ... 1e3), with components of 1e-40 (subnormal), 1e-20 and 1e20, and with
    inf and NaN components; origins in and around the grid, every other ray towards a solid voxel before its components are replaced."""
    o = rng.uniform(-0.2 * G, 1.2 * G, (n, 3))
    d = _unit(rng, n)
    solid = np.argwhere(mat > 0)
    if len(solid):
        aim = solid[rng.integers(0, len(solid), n)] + rng.uniform(0.0, 1.0, (n, 3)) - o
        d[::2] = (aim / np.linalg.norm(aim, axis=1, keepdims=True))[::2]
    d = d * 10.0 ** rng.uniform(-3.0, 3.0, (n, 1))
    special = np.array([1e-40, -1e-40, 1e-20, -1e-20, 1e20, -1e20, np.inf, -np.inf, np.nan])
    for j in range(n // 4, n):
        for a in rng.permutation(3)[:1 + j % 2]:
            d[j, a] = special[rng.integers(0, len(special))]
    with np.errstate(over="ignore"):
        return _rays(o, d)


def long_walk_candidates(rng, G, mat, n=30000):
    """Where walks get long: through the hull of the solids at a shallow angle to an axis plane and straight across it."""
    lo, hi, _ = grown_box(mat)
    a, b = rng.uniform(lo, hi, (n, 3)), rng.uniform(lo, hi, (n, 3))
    flat = rng.random(n) < 0.5
    ax = rng.integers(0, 3, n)
    b[flat, ax[flat]] = a[flat, ax[flat]] + rng.uniform(-2.0, 2.0, int(flat.sum()))
    d = b - a
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-9)
    o = a - d * rng.uniform(0.0, 1.5 * G, (n, 1))
    return _rays(o, d)


def recorded():
    """The 600 rays of tests/golden/reference/rays_sunlit.npz, as the reference's own raytracer.py computed them."""
    v = np.load(os.path.join(HERE, "golden", "reference", "rays_sunlit.npz"))
    want = np.zeros(len(v["distance"]), REC)
    want["dist"], want["cell"], want["normal"], want["iters"] = v["distance"], v["cell"], v["normal"], v["iters"]
    return _rays(v["origin"], v["direction"]), want


@functools.lru_cache(maxsize=None)
def oracle(name):
    o = orc.Oracle(config(name), threads=1)
    mat, rgb, params = scene(name)
    orc.setup(o, mat, rgb, params)
    return o


def oracle_trace(name, rays):
    out = np.zeros(len(rays), REC)
    orc.lib().orc_unit_raytrace_n(C.c_void_p(oracle(name)._ctx), len(rays), orc.fptr(rays), orc.fptr(out))
    return out


@functools.lru_cache(maxsize=None)
def family(name, fam):
    """(rays, the oracle's records) of one family on one scene: generated once, from a seed of its own, and left alone."""
    mat = scene(name)[0]
    G = mat.shape[0]
    rng = np.random.default_rng([20240607, SCENES.index(name), FAMILIES.index(fam)])
    if fam == "long":     # the oracle searches; the 200 longest stay, and so does every 512-step ray with a finite distance
        cand = long_walk_candidates(rng, G, mat)
        got = oracle_trace(name, cand)
        keep = np.zeros(len(cand), bool)
        keep[np.argsort(-got["iters"], kind="stable")[:200]] = True
        keep |= (got["iters"] >= 512) & np.isfinite(got["dist"])
        rays = np.ascontiguousarray(cand[keep])
    else:
        rays = {"axis": lambda: axis_parallel(rng, G), "boundary": lambda: boundary_origins(rng, G, mat),
                "box": lambda: box_aimed(rng, G, mat), "odd": lambda: odd_directions(rng, G, mat)}[fam]()
    want = oracle_trace(name, rays)
    rays.setflags(write=False)
    want.setflags(write=False)
    return rays, want


def cases():
    """(scene, family) pairs: every family on every scene but `sponge256`, which is there for the long walks: the oracle is asked
    to search it and `s1`."""
    return [(s, f) for s in SCENES for f in FAMILIES if (f == "long") == (s == "sponge256") or (s, f) == ("s1", "long")]


def counts(name, fam):
    _, want = family(name, fam)
    d = want["dist"]
    return dict(rays=len(d), hits=int(np.isfinite(d).sum()), misses=int(np.isinf(d).sum()), nans=int(np.isnan(d).sum()),
                max_iters=int(want["iters"].max()), full_512_finite=int(((want["iters"] >= 512) & np.isfinite(d)).sum()))


def check_guards(report=print):
    """The oracle's results alone: the families are what they claim to be, so no comparison passes on nothing."""
    for s, f in cases():
        c = counts(s, f)
        report(f"rays {s:10s} {f:9s} {c}")
        assert c["rays"] > 0, (s, f)
    box = counts("sunlit", "box")
    assert 4 * box["hits"] >= box["rays"] and 4 * box["misses"] >= box["rays"], box
    for s in SCENES:
        if s != "sponge256":
            assert counts(s, "axis")["nans"] >= 10, (s, counts(s, "axis"))
    for s in CULLING:                                                       # a box inside the grid, the 256^3 scene's too
        lo, hi, active = grown_box(scene(s)[0])
        assert active and (lo < hi).all() and ((lo > 0) | (hi < scene(s)[0].shape[0])).sum() >= 2, (s, lo, hi)
    assert scene("s1_256")[0].shape[0] == 256
    assert not grown_box(scene("dense")[0])[2] and not grown_box(scene("sponge256")[0])[2]    # cull[6] == 0
    assert (grown_box(scene("empty")[0])[0] > grown_box(scene("empty")[0])[1]).all()
    lo, hi, _ = grown_box(scene("one_voxel")[0])
    assert np.array_equal(hi - lo, [20.0, 20.0, 20.0])                      # one brick and the margin


def same_f32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def mismatches(got, want, *, iters, cells="finite"):
    """Indices of rays whose record differs from `want` under the rules in the header.  cells: "finite" | "all"."""
    bad = ~same_f32(got["dist"], want["dist"])
    if iters:
        bad |= got["iters"] != want["iters"]
    where = np.isfinite(want["dist"]) if cells == "finite" else np.ones(len(want), bool)
    bad |= where & ((got["cell"] != want["cell"]).any(axis=1) | ~same_f32(got["normal"], want["normal"]).all(axis=1))
    return np.flatnonzero(bad)


def describe(rays, got, want, idx):
    return "; ".join(f"ray {k} o={rays[k, :3].tolist()} d={rays[k, 3:].tolist()} got={got[k]} want={want[k]}" for k in idx[:3])


def check_probe(probe, rays, want, *, box_modes=(False, True), cells="finite", label="", culls=None):
    """probe(mode, rays) -> records.  Runs the three walks with the box off and on and applies the rules of the header.
    culls: None, or the grid size of a scene of CULLING whose box-aimed family `rays` is."""
    by_box = {}
    for box in box_modes:
        first = None
        for walk, code in WALKS.items():
            got = probe(code | (BOX if box else 0), rays)
            bad = mismatches(got, want, iters=not box, cells=cells)
            assert bad.size == 0, f"{label} {walk} box={'on' if box else 'off'}: {bad.size} of {len(rays)} rays differ: {describe(rays, got, want, bad)}"
            if first is None:
                first = got
            else:   # the walks agree on every field, misses included
                diff = np.flatnonzero(~same_f32(got["dist"], first["dist"]) | (got["iters"] != first["iters"]) | (got["cell"] != first["cell"]).any(axis=1) |
                                      ~same_f32(got["normal"], first["normal"]).all(axis=1))
                assert diff.size == 0, f"{label} {walk} vs branchy, box={'on' if box else 'off'}: {diff.size} rays differ: {describe(rays, got, first, diff)}"
        by_box[box] = first
    if culls:
        off, on = by_box[False], by_box[True]
        whole = (on["iters"] == 0) & (on["cell"] == -1).all(axis=1) & (on["normal"] == 0).all(axis=1) & np.isinf(on["dist"]) & (off["iters"] > 0)
        assert whole.sum() >= len(rays) // 100, f"{label}: the box culled {int(whole.sum())} of {len(rays)} rays that the walk steps through"
        if culls == 128:
            assert on["iters"].sum() < off["iters"][~whole].sum(), f"{label}: no walk ends where it leaves the box"
        else:
            assert np.array_equal(on["iters"][~whole], off["iters"][~whole]), f"{label}: at 256^3 only whole rays are culled"
        return int(whole.sum()), int(off["iters"].sum()), int(on["iters"].sum())
