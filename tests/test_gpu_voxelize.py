"""vrt_voxelize_triangles ON THE DEVICE: a context whose prepared grid was voxelised into (E) against a fresh context given the brute
force's final grid through vrt_upload_voxels + vrt_prepare (F), bit for bit -- no tolerance anywhere, every comparison is tobytes()
equality, no cell left out:
  (a) vrt_fetch_voxels over the WHOLE grid == the brute force's arrays (tests/voxelize.py: every triangle x every cell of the box);
  (b) the HDR frame after the same accumulate calls, under both schedules of the render stage;
  (c) vrt_trace_probe records of rays aimed at and around the box, in the three walks with the culling box off and on -- the step count
      is the only thing that sees a coarse bit left set, the culled records the only thing that sees a culling box that did not follow;
  (d) the result record (tight box, count, invalid) == the brute force's.
The families (tests/voxelize.py), each the smallest case of something that can go wrong, at 128^3 and 256^3:
  points           on a grid vertex / edge / face / inside a cell: 8, 4, 2, 1 cells -- closed cubes, a point is a hull
  segments         along a grid line, along a body diagonal through grid vertices: the degenerate hull's cross axes
  in_plane         a triangle in a grid plane: both layers
  sliver           1/64 thin, crossing bricks diagonally: nothing but exact arithmetic finds its cells
  huge             vertices at +-8: int64 headroom, thousands of items clipped to one box
  outside          outside the box, outside the grid, touching the box's boundary plane from outside (covers the boundary cells inside)
  unaligned        tests/edit.py's UNALIGNED box: brick, 16- and 64-cell boundaries cut the box
  stack, stack_reversed   identical triangles, different payloads: the highest index wins, whichever wave comes last
  negative         a negative material byte; invalid: NaN, inf, 8 + 1 ulp between valid triangles
  cube12           a closed cube from box_of_voxels' corners: every face in a grid plane
  carve_last       mat = 0 removes the last voxel (the grid becomes empty, the culling box follows), then a triangle adds one elsewhere
  ico_*            a 20-triangle icosphere on sunlit, dense and s1_256
Then: the oracle on the final grid, the device path, a real chunk boundary on the host path, a real batch boundary on the device path, one triangle spanning a 256^3 grid, ordering
against queries and launches in flight, a following vrt_update_voxels and plain vrt_prepare, the sky tables, the error codes, the facade
(Renderer.voxelize_triangles / mesh_box) and examples/voxelize_mesh.py."""
import ctypes as C
import os
import runpy

import numpy as np
import pytest

import edit as E
import orc
import rays as R
import voxelize as V
from voxel_rt2_amd import _abi, _lib, host
from voxel_rt2_amd._session import NativeError, NativeSession

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, DEPTH, SEED = 64, 48, 4, 7
MODES = [w | b for b in (0, R.BOX) for w in R.WALKS.values()]


def config(base, sky_res=0):
    mat, _, params = R.scene(base)
    return host.make_config(W, H, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=DEPTH, seed=SEED, grid_res=mat.shape[0],
                            sky_res=sky_res)


def fresh(base, mat, rgb, cls=None):
    s = NativeSession(_lib.load(), "vrt_", config(base)) if cls is None else cls(config(base))
    orc.setup(s, mat, rgb, R.scene(base)[2])
    return s


def frame(s):
    s.accumulate(4)
    s.accumulate(4)
    return s.fetch_hdr()


def probe(s, mode, rays):
    out = np.zeros(len(rays), R.REC)
    rc = _lib.load().vrt_trace_probe(C.c_void_p(s._ctx), int(mode), len(rays), orc.fptr(rays), orc.fptr(out))
    assert rc == 0, _lib.load().vrt_last_error()
    return out


def rays_around(mat, lo, hi, seed):
    """tests/rays.py's families aimed at the clip box (grown by the culling margin, as the generator does), from cell boundaries of a
    sample of the final grid's solids, and axis-parallel ones"""
    G = mat.shape[0]
    aim = np.zeros_like(mat)
    aim[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
    rng = np.random.default_rng([20261020, seed])
    thin = np.zeros_like(mat)
    solid = np.argwhere(mat > 0)
    if len(solid):
        pick = solid[rng.integers(0, len(solid), 2000)]
        thin[pick[:, 0], pick[:, 1], pick[:, 2]] = 1
    return np.ascontiguousarray(np.concatenate([R.box_aimed(rng, G, aim, n=800), R.boundary_origins(rng, G, thin, n=300), R.axis_parallel(rng, G, n=200)]))


def whole_grid(s):
    g = int(s.cfg.grid_res)
    return s.fetch_voxels((0, 0, 0), (g, g, g))


def assert_grid(s, mat, rgb, label):
    m, c = whole_grid(s)
    assert m.tobytes() == mat.tobytes(), f"{label}: {(m != mat).sum()} materials differ from the brute force's"
    assert c.tobytes() == rgb.tobytes(), f"{label}: {(c != rgb).any(axis=-1).sum()} colours differ from the brute force's"


def voxelised(name, G, via=None):
    """base grid -> prepare -> every call of the case -> reset; the result records on the way"""
    base, calls = V.case(name, G)
    s = fresh(base, *R.scene(base)[:2])
    results = [(via or NativeSession.voxelize_triangles)(s, *call) for call in calls]
    s.reset()
    return s, results


@pytest.mark.parametrize("schedule", ["pool", "fused"])
@pytest.mark.parametrize("name,G", V.cases())
def test_voxelised_context_equals_fresh_context(name, G, schedule, monkeypatch):
    monkeypatch.setenv("VRT_RENDER", schedule)
    base, calls = V.case(name, G)
    states = V.states(name, G)
    mat, rgb, _ = states[-1]
    e, results = voxelised(name, G)
    f = fresh(base, mat, rgb)
    try:
        for got, (_, _, want) in zip(results, states[1:]):
            assert V.same_result(got, want), f"{name}/{G}: result {got} != {want}"
        if schedule == "pool":                        # (grid and probes do not depend on the schedule)
            assert_grid(e, mat, rgb, f"{name}/{G}")
            rays = rays_around(mat, *calls[-1][1:], seed=V.cases().index((name, G)))
            for mode in MODES:
                got, want = probe(e, mode, rays), probe(f, mode, rays)
                bad = np.flatnonzero((got.view(np.uint8).reshape(len(rays), -1) != want.view(np.uint8).reshape(len(rays), -1)).any(axis=1))
                assert got.tobytes() == want.tobytes(), f"{name}/{G} mode {mode}: {bad.size} of {len(rays)} records differ: {R.describe(rays, got, want, bad)}"
        a, b = frame(e), frame(f)
        assert a.tobytes() == b.tobytes(), f"{name}/{G} ({schedule}): {(a != b).sum()} of {a.size} values differ"
    finally:
        e.close()
        f.close()


@pytest.mark.parametrize("name", ["ico_sunlit", "carve_last"])
def test_voxelised_context_equals_oracle_on_the_final_grid(name):
    base = V.case(name, 128)[0]
    mat, rgb, _ = V.states(name, 128)[-1]
    e, _ = voxelised(name, 128)
    o = fresh(base, mat, rgb, cls=lambda cfg: orc.Oracle(cfg, threads=4))
    try:
        a, b = frame(e), frame(o)
        assert a.tobytes() == b.tobytes(), f"{name}: {(a != b).sum()} of {a.size} values differ from the oracle's"
    finally:
        e.close()
        o.close()


@pytest.mark.parametrize("name,G", [("stack", 128), ("ico_s1_256", 256), ("invalid", 128)])
def test_device_path_equals_host_path(name, G):
    import torch
    keep = []

    def from_torch(s, tris, lo, hi):
        t = torch.from_numpy(np.ascontiguousarray(tris).view(np.uint8).reshape(-1).copy()).cuda()
        torch.cuda.synchronize()                      # the tensor is written on torch's stream, read on the context's
        keep.append(t)
        return s.voxelize_triangles(t, lo, hi)
    (d, rd), (h, rh) = voxelised(name, G, via=from_torch), voxelised(name, G)
    try:
        assert all(V.same_result(x, y) for x, y in zip(rd, rh)) and V.same_result(rd[-1], V.states(name, G)[-1][2])
        (m0, c0), (m1, c1) = whole_grid(d), whole_grid(h)
        assert m0.tobytes() == m1.tobytes() and c0.tobytes() == c1.tobytes()
        assert frame(d).tobytes() == frame(h).tobytes()
    finally:
        d.close()
        h.close()


def test_host_path_across_a_chunk_boundary():
    """n = one chunk + 2: almost every triangle lies outside the box (a point far away in the grid), the last of the first chunk and the
    first of the second overlap inside it, and the very last is a third layer over part of both."""
    chunk = int(V.lib().vox_emul_plan(0))
    o = V.origin(128)
    lo, hi = (o, o, o), (o + 32, o + 32, o + 32)
    tris = np.repeat(V.triangles(128, [[(3.5, 3.5, 3.5)] * 3], [V.payload((1, 2, 3), 11)]), chunk + 2)
    over = V.triangles(128, np.array([[(3, 4, 5.5), (27, 6, 9.25), (11, 26, 20)], [(5, 3, 7.5), (25, 9, 8.25), (13, 24, 21)], [(3, 4, 9), (20, 20, 9), (3, 20, 9)]]) + o,
                       [V.payload((250, 10, 10), 21), V.payload((10, 250, 10), 2), V.payload((10, 10, 250), 54)])
    tris[chunk - 1], tris[chunk], tris[chunk + 1] = over[0], over[1], over[2]
    mat0, rgb0, _ = R.scene("sunlit")
    few = tris[[0, chunk - 1, chunk, chunk + 1]]      # the same outcome: the far points are all one triangle outside the box
    mat, rgb, want = V.brute(mat0, rgb0, few, lo, hi)
    assert want["voxels"] > 100 and len({int(x) for x in np.unique(mat[o:o + 32, o:o + 32, o:o + 32])} & {21, 2, 54}) == 3
    e = fresh("sunlit", mat0, rgb0)
    try:
        got = e.voxelize_triangles(tris, lo, hi)
        assert V.same_result(got, want), (got, want)
        assert_grid(e, mat, rgb, "chunk boundary")
    finally:
        e.close()


def test_device_path_across_a_batch_boundary():
    """n = one batch + 2 on the device path: the set-up and rasterise passes run twice, numbering owners base + index + 1, and ONE resolve
    with base 0 reads the payloads from the caller's array.  Almost every triangle is a point outside the box; the last of the first batch
    and the first of the second overlap inside it, and the very last is a third layer over part of both."""
    import torch
    batch = int(V.lib().vox_emul_plan(1))
    o = V.origin(128)
    lo, hi = (o, o, o), (o + 32, o + 32, o + 32)
    tris = np.repeat(V.triangles(128, [[(3.5, 3.5, 3.5)] * 3], [V.payload((1, 2, 3), 11)]), batch + 2)
    over = V.triangles(128, np.array([[(3, 4, 5.5), (27, 6, 9.25), (11, 26, 20)], [(5, 3, 7.5), (25, 9, 8.25), (13, 24, 21)], [(3, 4, 9), (20, 20, 9), (3, 20, 9)]]) + o,
                       [V.payload((250, 10, 10), 21), V.payload((10, 250, 10), 2), V.payload((10, 10, 250), 54)])
    tris[batch - 1], tris[batch], tris[batch + 1] = over[0], over[1], over[2]
    tris["v1"][7, 2] = np.nan                          # and an invalid one in the first batch: counted once
    mat0, rgb0, _ = R.scene("sunlit")
    few = tris[[0, 7, batch - 1, batch, batch + 1]]   # the same outcome: the far points are all one triangle outside the box
    mat, rgb, want = V.brute(mat0, rgb0, few, lo, hi)
    assert want["voxels"] > 100 and want["invalid"] == 1 and len({int(x) for x in np.unique(mat[o:o + 32, o:o + 32, o:o + 32])} & {21, 2, 54}) == 3
    e = fresh("sunlit", mat0, rgb0)
    try:
        t = torch.from_numpy(tris.view(np.uint8).reshape(-1)).cuda()
        torch.cuda.synchronize()                      # the tensor is written on torch's stream, read on the context's
        got = e.voxelize_triangles(t, lo, hi)
        assert V.same_result(got, want), (got, want)
        assert_grid(e, mat, rgb, "batch boundary")
    finally:
        e.close()


def test_one_triangle_spanning_a_256_grid():
    """The whole grid as the box, one triangle through it diagonally: 4096 work items.  The brute force looks at the cells within two
    voxels of the triangle's plane (every other cell is separated on the normal's axis by more than a cell's reach) -- all of them."""
    G = 256
    mat0, rgb0, _ = R.scene("s1_256")
    t = np.zeros(1, V.TRI)
    t["v0"], t["v1"], t["v2"], t["voxel"] = (-1.5, -1.25, -1.0), (1.5, 1.0, 1.25), (1.25, -1.5, 0.75), V.payload((200, 120, 40), 11)
    s = V.snap(V.vertices(t), G)[0]
    n = np.cross(s[1] - s[0], s[2] - s[1])
    x = np.arange(G, dtype=np.int64)
    d = (n[0] * (64 * x + 32))[:, None, None] + (n[1] * (64 * x + 32))[None, :, None] + (n[2] * (64 * x + 32))[None, None, :] - n @ s[0]
    near = np.argwhere(np.abs(d) <= 2 * 64 * np.abs(n).sum())                                 # centre within two cells' reach of the plane
    assert 100000 < len(near) < 2000000
    mat, rgb, want = V.brute(mat0, rgb0, t, (0, 0, 0), (G, G, G), cells=near)
    assert want["voxels"] > 50000
    e = fresh("s1_256", mat0, rgb0)
    try:
        got = e.voxelize_triangles(t, (0, 0, 0), (G, G, G))
        assert V.same_result(got, want), (got, want)
        assert_grid(e, mat, rgb, "spanning triangle")
    finally:
        e.close()


def test_queries_and_launches_are_ordered_against_the_call():
    """A vrt_cast_rays queued (device path, no synchronisation) before the call sees the old grid, one queued after it the new; six
    accumulate calls in flight see the old grid; then a vrt_update_voxels and a plain vrt_prepare still leave what a fresh context has."""
    import torch
    name = "cube12"
    base, calls = V.case(name, 128)
    tris, lo, hi = calls[0]
    (mat0, rgb0, _), (mat1, rgb1, _) = V.states(name, 128)
    o = V.origin(128)
    rays = np.zeros(64, _abi.RAY)
    rays["origin"] = V.world(128, [(o + 7.5 + (k % 8), 127.5, o + 6.5 + k // 8) for k in range(64)])      # straight down onto the cube's top
    rays["dir"], rays["t_max"] = (0, -1, 0), np.inf

    def six(s):
        for _ in range(6):
            s.accumulate(4)
    e, u, f = fresh(base, mat0, rgb0), fresh(base, mat0, rgb0), fresh(base, mat1, rgb1)
    try:
        want_old, want_new = u.cast_rays(rays), f.cast_rays(rays)
        assert want_old.tobytes() != want_new.tobytes()
        t_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).cuda()
        before, after = (torch.zeros(64 * _abi.HIT.itemsize, dtype=torch.uint8, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        six(e)
        e.cast_rays(t_rays, before)
        e.voxelize_triangles(tris, lo, hi)
        e.cast_rays(t_rays, after)
        e.sync()
        assert before.cpu().numpy().tobytes() == want_old.tobytes() and after.cpu().numpy().tobytes() == want_new.tobytes()
        six(u)
        a, b = e.fetch_hdr(), u.fetch_hdr()
        assert a.tobytes() == b.tobytes(), f"launches queued before the call saw it: {(a != b).sum()} of {a.size} values differ"
        edit = E._pattern((o + 2, o + 20, o + 3), (o + 9, o + 31, o + 12), seed=9, m=21)
        e.update_voxels(*edit)
        mat2, rgb2 = E.apply_numpy(mat1, rgb1, edit)
        f.update_voxels(*edit)
        six(f)                                        # (the frame counter goes on through a reset: as many launches on both)
        e.prepare()
        assert_grid(e, mat2, rgb2, "after a following edit and prepare")
        e.reset()
        f.reset()
        assert frame(e).tobytes() == frame(f).tobytes()
    finally:
        for s in (e, u, f):
            s.close()


def test_physical_sky_tables_survive_a_voxelisation():
    cloud = np.load(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "data", "cloud_texture.npy"))
    mat, rgb, params = R.scene("s6")
    v, faces = V.icosphere((56.3, 40.6, 64.9), 9.2)
    tris, lo, hi = V.triangles(128, v[faces]), (44, 28, 52), (70, 54, 78)
    final = V.brute(mat, rgb, tris, lo, hi)

    def session(m, c):
        s = NativeSession(_lib.load(), "vrt_", config("s6", sky_res=64))
        orc.setup(s, m, c, params, cloud=cloud)
        for _ in range(2):
            s.sky_accumulate_clouds(2)
        for sl in range(4):
            s.sky_compute_slice(sl, 4)
        return s
    e, f = session(mat, rgb), session(*final[:2])
    try:
        before = [e.fetch_buffer(w) for w in (_abi.BUF_SKY_SCATTERING, _abi.BUF_SKY_TRANSMITTANCE, _abi.BUF_TRANS_LUT)]
        assert before[0].max() > 0 and before[1].max() > 0
        assert V.same_result(e.voxelize_triangles(tris, lo, hi), final[2])
        after = [e.fetch_buffer(w) for w in (_abi.BUF_SKY_SCATTERING, _abi.BUF_SKY_TRANSMITTANCE, _abi.BUF_TRANS_LUT)]
        for x, y in zip(before, after):
            assert x.tobytes() == y.tobytes()
        e.reset()
        a, b = frame(e), frame(f)
        assert a.tobytes() == b.tobytes(), f"{(a != b).sum()} of {a.size} values differ"
    finally:
        e.close()
        f.close()


def test_error_codes_empty_calls_and_a_null_result():
    lib = _lib.load()
    mat, rgb, params = R.scene("sunlit")
    one = V.triangles(128, [[(60.5, 70.5, 60.5)] * 3])
    poison = np.full(1, -1, np.int64).repeat(5).view(np.uint8)[:40].copy()

    def call(s, lo, hi, tris=one, n=None, on_device=0, result="fresh"):
        res = poison.copy() if isinstance(result, str) else result
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        rc = lib.vrt_voxelize_triangles(C.c_void_p(s._ctx), len(tris) if n is None else n, p(tris), None if lo is None else (C.c_int32 * 3)(*lo),
                                        None if hi is None else (C.c_int32 * 3)(*hi), p(res), on_device)
        return rc, res
    s = NativeSession(lib, "vrt_", config("sunlit"))
    try:
        assert call(s, (1, 1, 1), (2, 2, 2))[0] == _abi.VRT_E_STATE                   # before vrt_prepare
        orc.setup(s, mat, rgb, params)
        s.upload_voxels(mat, rgb)
        assert call(s, (1, 1, 1), (2, 2, 2))[0] == _abi.VRT_E_STATE                   # after an upload that no prepare has followed
        with pytest.raises(NativeError):
            s.voxelize_triangles(one, (1, 1, 1), (2, 2, 2))
        with pytest.raises(NativeError):              # an empty array meets the same checks of box and state
            s.voxelize_triangles(one[:0], (1, 1, 1), (2, 2, 2))
        s.prepare()
        import torch
        with pytest.raises(ValueError):               # a tensor in host memory never reaches the device path
            s.voxelize_triangles(torch.from_numpy(one.view(np.uint8).reshape(-1).copy()), (56, 66, 56), (64, 74, 64))
        with pytest.raises(NativeError):
            s.voxelize_triangles(one[:0], (2, 1, 1), (1, 2, 2))
        assert not s.voxelize_triangles(one[:0], (0, 0, 0), (128, 128, 128)).tobytes().strip(b"\0")
        assert not s.voxelize_triangles(torch.zeros(0, dtype=torch.uint8, device="cuda"), (0, 0, 0), (128, 128, 128)).tobytes().strip(b"\0")
        for lo, hi in (((2, 1, 1), (1, 2, 2)), ((-1, 0, 0), (0, 1, 1)), ((127, 127, 127), (128, 128, 129)), ((0, 200, 0), (1, 201, 1))):
            assert call(s, lo, hi)[0] == _abi.VRT_E_INVALID, (lo, hi)
        assert call(s, None, (1, 1, 1))[0] == call(s, (0, 0, 0), None)[0] == call(s, (0, 0, 0), (1, 1, 1), tris=None, n=1)[0] == _abi.VRT_E_INVALID
        assert call(s, (0, 0, 0), (1, 1, 1), n=-1)[0] == call(s, (0, 0, 0), (1, 1, 1), n=2 ** 32 - 1)[0] == _abi.VRT_E_INVALID
        assert call(s, (0, 0, 0), (1, 1, 1), on_device=2)[0] == call(s, (0, 0, 0), (1, 1, 1), on_device=-1)[0] == _abi.VRT_E_INVALID
        for field in ("reserved0", "reserved1"):
            bad = one.copy()
            bad[field] = 7
            assert call(s, (0, 0, 0), (128, 128, 128), tris=bad)[0] == _abi.VRT_E_INVALID
        for lo, hi, n in (((5, 5, 5), (5, 9, 9), None), ((128, 128, 128), (128, 128, 128), None), ((0, 0, 0), (128, 128, 128), 0)):
            rc, res = call(s, lo, hi, n=n)
            assert rc == _abi.VRT_OK and not res.any(), (lo, hi, n)                   # nothing done, the result zeroed
        assert_grid(s, mat, rgb, "after the refused and the empty calls")
        rc, _ = call(s, (56, 66, 56), (64, 74, 64), result=None)                      # a NULL result
        assert rc == _abi.VRT_OK
        m, c = whole_grid(s)
        assert m[60, 70, 60] == 11 and (m != mat).sum() == 1
        rc, res = call(s, (56, 66, 56), (64, 74, 64))
        r = res.view(_abi.VOXELIZE_RESULT)[0]
        assert rc == _abi.VRT_OK and r["lo"].tolist() == [60, 70, 60] and r["hi"].tolist() == [61, 71, 61] and r["voxels"] == 1 and r["invalid"] == 0
    finally:
        s.close()


def test_reserved_words_make_a_triangle_invalid_on_the_device_path():
    import torch
    tris, lo, hi = V.case("stack", 128)[1][0]
    tris = tris.copy()
    tris["reserved1"][4], tris["reserved0"][3] = 1, 0x80000000
    mat, rgb, want = V.brute(*R.scene("sunlit")[:2], tris, lo, hi)
    assert want["invalid"] == 2
    e = fresh("sunlit", *R.scene("sunlit")[:2])
    try:
        t = torch.from_numpy(tris.view(np.uint8).reshape(-1).copy()).cuda()
        torch.cuda.synchronize()
        assert V.same_result(e.voxelize_triangles(t, lo, hi), want)
        assert_grid(e, mat, rgb, "reserved words")
    finally:
        e.close()


def test_renderer_voxelize_triangles_equals_authoring_the_grid():
    from voxel_rt2_amd.renderer import Renderer

    def renderer():
        r = Renderer(dx=1 / 64, image_res=(W, H), up=(0, 1, 0), voxel_edges=0.06, exposure=1.5, max_depth=DEPTH, seed=SEED, sky_res=0)
        r.set_directional_light((0.6, 1.0, 0.4), 0.1, (1.0, 0.95, 0.85))
        r.background_color[None] = (0.35, 0.5, 0.75)
        r.floor_height[None] = -0.3
        return r
    first = [((x, -3, z), 11, (0.8, 0.3, 0.2)) for x in range(-6, 7) for z in range(-6, 7)]
    v, faces = V.icosphere((0.05, 0.12, -0.03), 0.11, 1)                                  # world units: 80 triangles
    cube = V.world(128, V.cube12((70, 66, 60), (75, 72, 66)))
    e, f = renderer(), renderer()
    try:
        with pytest.raises(NativeError):
            e.voxelize_triangles(v, faces)
        for vox in first:
            e.set_voxel(*vox)
        e.prepare_data()
        e.set_voxel((9, -3, 9), 2, (1.0, 1.0, 1.0))                                       # not yet sent: goes first
        base_m, base_c = e.voxel_material.copy(), e.voxel_color.copy()
        box = e.mesh_box(v)
        assert e.mesh_box(np.concatenate([v, [[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0]]])) == box      # non-finite vertices are left out
        assert e.mesh_box([[np.nan] * 3]) == ((0, 0, 0), (0, 0, 0)) and e.mesh_box([[-0.5, 0.0, 0.25]]) == ((31, 63, 79), (33, 65, 81))
        colors = np.stack([np.arange(80) * 3, 255 - np.arange(80) * 2, np.full(80, 90)], axis=1)
        mats = np.where(np.arange(80) % 2, 11, 21)
        r1 = e.voxelize_triangles(v, faces, color=colors, mat=mats, lo=box[0], hi=box[1])
        r2 = e.voxelize_triangles(cube, color=(10, 20, 30), mat=0)                        # the whole grid as the box; carves
        assert r1["voxels"] > 300 and r1["invalid"] == 0 and r2["voxels"] > 0 and e.current_spp == 0
        whole = e.voxelize_triangles(v, faces, color=colors, mat=mats)
        assert V.same_result(whole, r1)                                                   # mesh_box left nothing of the mesh out
        m, c = e.session.fetch_voxels((0, 0, 0), (128, 128, 128))
        assert e.voxel_material.tobytes() == m.tobytes() and e.voxel_color.tobytes() == c.tobytes()     # the host mirror is in step
        assert m[9 + 64, -3 + 64, 9 + 64] == 2
        f.set_voxel_arrays(m, c)
        f.prepare_data()
        for r in (e, f):
            r.accumulate(4)
        assert e.fetch_hdr().tobytes() == f.fetch_hdr().tobytes() and e.fetch_hdr().std() > 0
        # and what the three calls wrote is the brute force's grid
        tr, ct = np.zeros(80, V.TRI), np.zeros(12, V.TRI)
        tr["v0"], tr["v1"], tr["v2"] = (np.asarray(v, np.float32)[faces][:, k] for k in range(3))
        tr["voxel"] = [V.payload(tuple(int(x) for x in colors[k]), int(mats[k])) for k in range(80)]
        ct["v0"], ct["v1"], ct["v2"], ct["voxel"] = cube[:, 0], cube[:, 1], cube[:, 2], V.payload((10, 20, 30), 0)
        bm, bc, br = V.brute(base_m, base_c, tr, *box)
        assert V.same_result(br, r1)
        bm, bc, br = V.brute(bm, bc, ct, (64, 60, 56), (80, 76, 72))                      # (the cube's bounds grown: no other cell can be covered)
        assert V.same_result(br, r2)
        bm, bc, _ = V.brute(bm, bc, tr, *box)
        assert bm.tobytes() == m.tobytes() and bc.tobytes() == c.tobytes()
    finally:
        e.session.close()
        f.session.close()


def test_voxelize_mesh_example_runs(tmp_path, monkeypatch):
    import sys
    for k, v in (("VRT_RES", "64x40"), ("VRT_FRAMES", "2"), ("VRT_SKY_RES", "32"), ("VRT_MAX_DEPTH", "2"), ("VRT_OUT", str(tmp_path / "mesh.png"))):
        monkeypatch.setenv(k, v)
    monkeypatch.syspath_prepend(ROOT)
    sys.modules.pop("scene", None)
    mod = runpy.run_path(os.path.join(ROOT, "examples", "voxelize_mesh.py"), run_name="voxelize_mesh")
    r, results = mod["main"]()
    try:
        assert (tmp_path / "mesh.png").exists()
        assert all(res["voxels"] > 0 and res["invalid"] == 0 for res in results.values())
        m, c = r.session.fetch_voxels((0, 0, 0), (r.voxel_grid_res,) * 3)
        assert r.voxel_material.tobytes() == m.tobytes() and r.voxel_color.tobytes() == c.tobytes()
        assert results["carve"]["voxels"] > 0 and (m == 54).sum() > 0 and (m == 2).sum() > 0
    finally:
        r.session.close()
