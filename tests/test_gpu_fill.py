"""vrt_fill_triangles ON THE DEVICE: a context whose prepared grid was filled (E) against a fresh context given the brute force's final
grid through vrt_upload_voxels + vrt_prepare (F), bit for bit -- no tolerance anywhere, every comparison is tobytes() equality:
  (a) vrt_fetch_voxels over the WHOLE grid == the brute force's arrays (tests/fill.py: every triangle x every cell of the box);
  (b) a small HDR frame after the same accumulate calls;
  (c) vrt_trace_probe records of rays aimed at and around the box, culling box off and on -- the step count is the only thing that sees
      a coarse bit left set, the culled records the only thing that sees a culling box that did not follow;
  (d) the result record (tight box, count of the inside cells, invalid) == the brute force's;
on the host path and on the device path.  The families (tests/fill.py), each the smallest case of something that can go wrong, at
128^3, in a 36 x 34 x 47 box (two toggle words a column, the meshes across the word boundary):
  cube_planes      faces in grid planes;  cube_centres: faces through cell centres -- depth, edge and vertex ties, the half-open interval
  tetra_centres    every vertex on a cell centre;  fan_apex: six triangles around an apex exactly over a centre: one owns the column
  icosphere, torus a convex solid, one with a hole;  nested: a hollow ball;  overlap: XOR of two solids
  reversed, mixed  orientation does not matter;  duplicated, flat: cancel, nothing is written
  hemisphere       an open mesh;  invalid: one NaN triangle in a closed mesh, skipped and counted
  slivers          a tetrahedron 1/64 thick, sub-voxel ones around and beside a centre
  below, above     a closed mesh under / over a flat box: writes nothing;  poke: through all six sides of a small box
  halves           the box in two calls along z == the box at once;  carve: mat = 0 out of a solid block;  negative: a negative byte
Then: 256^3, a real chunk boundary on the host path and a real batch boundary on the device path (a closed cube's twelve triangles
straddle it), a grid-spanning pair of triangles under a full-grid box, ordering against queries, launches in flight,
vrt_update_voxels and vrt_voxelize_triangles on the same stream, the scratch buffer taken in turns with the surface pass, the error
codes, the facade (shell=True included) and examples/fill_mesh.py."""
import ctypes as C
import os
import runpy

import numpy as np
import pytest

import distance as D
import edit as E
import fill as FL
import orc
import rays as R
import voxelize as V
from voxel_rt2_amd import _abi, _lib, host
from voxel_rt2_amd._session import NativeError, NativeSession

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, DEPTH, SEED = 64, 48, 4, 7
MODES = [R.WALKS["record"], R.WALKS["branchy"] | R.BOX, R.WALKS["flat"] | R.BOX]   # (each walk once, the culling box off and on)


def config(base):
    mat, _, params = R.scene(base)
    return host.make_config(W, H, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=DEPTH, seed=SEED, grid_res=mat.shape[0], sky_res=0)


def fresh(base, mat, rgb):
    s = NativeSession(_lib.load(), "vrt_", config(base))
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
    """tests/rays.py's families aimed at the clip box, from cell boundaries of a sample of the final grid's solids, and axis-parallel ones"""
    G = mat.shape[0]
    aim = np.zeros_like(mat)
    aim[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
    rng = np.random.default_rng([20261020, 77, seed])
    thin = np.zeros_like(mat)
    solid = np.argwhere(mat > 0)
    if len(solid):
        pick = solid[rng.integers(0, len(solid), 2000)]
        thin[pick[:, 0], pick[:, 1], pick[:, 2]] = 1
    return np.ascontiguousarray(np.concatenate([R.box_aimed(rng, G, aim, n=500), R.boundary_origins(rng, G, thin, n=200), R.axis_parallel(rng, G, n=100)]))


def whole_grid(s):
    g = int(s.cfg.grid_res)
    return s.fetch_voxels((0, 0, 0), (g, g, g))


def assert_grid(s, mat, rgb, label):
    m, c = whole_grid(s)
    assert m.tobytes() == mat.tobytes(), f"{label}: {(m != mat).sum()} materials differ from the brute force's"
    assert c.tobytes() == rgb.tobytes(), f"{label}: {(c != rgb).any(axis=-1).sum()} colours differ from the brute force's"


def on_device(keep):
    import torch

    def call(s, tris, lo, hi, voxel):
        t = torch.from_numpy(np.ascontiguousarray(tris).view(np.uint8).reshape(-1).copy()).cuda()
        torch.cuda.synchronize()                      # the tensor is written on torch's stream, read on the context's
        keep.append(t)
        return s.fill_triangles(t, lo, hi, voxel)
    return call


def filled(name, G, via=NativeSession.fill_triangles):
    """base grid -> prepare -> every call of the case -> reset; the result records on the way"""
    base, calls = FL.case(name, G)
    s = fresh(base, *R.scene(base)[:2])
    results = [via(s, *call) for call in calls]
    s.reset()
    return s, results


def check_family(name, G):
    base, calls = FL.case(name, G)
    states = FL.states(name, G)
    mat, rgb, _ = states[-1]
    keep = []
    (h, rh), (d, rd), f = filled(name, G), filled(name, G, on_device(keep)), fresh(base, mat, rgb)
    try:
        rays = rays_around(mat, *calls[-1][1:3], seed=FL.GENERIC.index(name))
        want_frame, want_probe = frame(f), [probe(f, mode, rays) for mode in MODES]
        for path, e, results in (("host", h, rh), ("device", d, rd)):
            for got, (_, _, want) in zip(results, states[1:]):
                assert FL.same_result(got, want), f"{name}/{G} {path} path: result {got} != {want}"
            assert_grid(e, mat, rgb, f"{name}/{G} {path} path")
            for mode, want in zip(MODES, want_probe):
                got = probe(e, mode, rays)
                bad = np.flatnonzero((got.view(np.uint8).reshape(len(rays), -1) != want.view(np.uint8).reshape(len(rays), -1)).any(axis=1))
                assert got.tobytes() == want.tobytes(), f"{name}/{G} {path} path, mode {mode}: {bad.size} of {len(rays)} records differ: {R.describe(rays, got, want, bad)}"
            a = frame(e)
            assert a.tobytes() == want_frame.tobytes(), f"{name}/{G} {path} path: {(a != want_frame).sum()} of {a.size} values differ"
    finally:
        for s in (h, d, f):
            s.close()


@pytest.mark.parametrize("name", FL.GENERIC)
def test_filled_context_equals_fresh_context(name):
    check_family(name, 128)


@pytest.mark.parametrize("name", ["cube_centres", "icosphere"])
def test_filled_context_equals_fresh_context_256(name):
    check_family(name, 256)


def straddling(n_before):
    """n_before + 6 triangles: almost all of them one small triangle beside the box (no column of it), one of them invalid; the twelve
    of a closed cube inside the box sit at n_before - 6 .. n_before + 5.  -> (triangles, the few that matter, lo, hi)"""
    o = FL.origin(128)
    lo, hi = FL.default_box(128)
    far = FL.mesh(128, [[(3.5, 3.5, 3.5), (5.5, 3.5, 3.5), (3.5, 5.5, 4.5)]])
    tris = np.repeat(far, n_before + 6)
    cube = FL.mesh(128, np.asarray(V.cube12((6.5, 9.5, 5.5), (19.5, 25.5, 22.5))) + o)
    tris[n_before - 6:n_before + 6] = cube
    tris["v1"][7, 2] = np.nan
    return tris, np.concatenate([tris[[0, 7]], cube]), lo, hi


def test_host_path_across_a_chunk_boundary():
    """n = one chunk + 6: six of a closed cube's triangles toggle in the first chunk, six in the second; nothing is resolved between them."""
    tris, few, lo, hi = straddling(int(FL.lib().fill_emul_plan(0)))
    mat0, rgb0, _ = R.scene("sunlit")
    mat, rgb, want = FL.brute(mat0, rgb0, few, lo, hi, FL.PAY)
    assert want["voxels"] == 13 * 16 * 17 and want["invalid"] == 1
    e = fresh("sunlit", mat0, rgb0)
    try:
        got = e.fill_triangles(tris, lo, hi, FL.PAY)
        assert FL.same_result(got, want), (got, want)
        assert_grid(e, mat, rgb, "chunk boundary")
    finally:
        e.close()


def test_device_path_across_a_batch_boundary():
    import torch
    tris, few, lo, hi = straddling(int(FL.lib().fill_emul_plan(1)))
    mat0, rgb0, _ = R.scene("sunlit")
    mat, rgb, want = FL.brute(mat0, rgb0, few, lo, hi, FL.PAY)
    assert want["voxels"] == 13 * 16 * 17 and want["invalid"] == 1
    e = fresh("sunlit", mat0, rgb0)
    try:
        t = torch.from_numpy(tris.view(np.uint8).reshape(-1)).cuda()
        torch.cuda.synchronize()                      # the tensor is written on torch's stream, read on the context's
        got = e.fill_triangles(t, lo, hi, FL.PAY)
        assert FL.same_result(got, want), (got, want)
        assert_grid(e, mat, rgb, "batch boundary")
    finally:
        e.close()


def test_a_grid_spanning_pair_of_triangles_under_a_full_grid_box():
    """The whole 128^3 grid as the box, a triangle larger than the grid and a tilted copy above it: 64 work items each, four toggle
    words a column; what lies between the two is inside (an open mesh: defined)."""
    G = 128
    mat0, rgb0, _ = R.scene("sunlit")
    t = np.zeros(2, V.TRI)
    t["v0"], t["v1"], t["v2"] = [(-3, -3, -0.6), (-3, -3, 0.1)], [(3, -3, -0.4), (3, -3, 0.3)], [(0, 4, -0.5), (0, 4, 0.65)]
    mat, rgb, want = FL.brute(mat0, rgb0, t, (0, 0, 0), (G, G, G), FL.PAY)
    assert 300000 < want["voxels"] < 1500000 and want["lo"].tolist()[:2] == [0, 0] and want["hi"].tolist()[:2] == [G, G]
    assert [int(FL.emul_cells(G, t[k], (0, 0, 0), (G, G, G))[8]) for k in range(2)] == [64, 64]
    e = fresh("sunlit", mat0, rgb0)
    try:
        got = e.fill_triangles(t, (0, 0, 0), (G, G, G), FL.PAY)
        assert FL.same_result(got, want), (got, want)
        assert_grid(e, mat, rgb, "spanning pair")
    finally:
        e.close()


def test_queries_launches_and_other_edits_are_ordered_against_the_call():
    """A vrt_cast_rays queued (device path, no synchronisation) before the call sees the old grid, one queued after it the new; six
    accumulate calls in flight see the old grid (frames are untouched until the call); then a vrt_update_voxels, a
    vrt_voxelize_triangles of the mesh's surface, a carving fill and a plain vrt_prepare leave what the same steps leave in numpy."""
    import torch
    name = "cube_planes"
    base, calls = FL.case(name, 128)
    tris, lo, hi, voxel = calls[0]
    (mat0, rgb0, _), (mat1, rgb1, _) = FL.states(name, 128)
    o = FL.origin(128)
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
        e.fill_triangles(tris, lo, hi, voxel)
        e.cast_rays(t_rays, after)
        e.sync()
        assert before.cpu().numpy().tobytes() == want_old.tobytes() and after.cpu().numpy().tobytes() == want_new.tobytes()
        six(u)
        a, b = e.fetch_hdr(), u.fetch_hdr()
        assert a.tobytes() == b.tobytes(), f"launches queued before the call saw it: {(a != b).sum()} of {a.size} values differ"
        edit = E._pattern((o + 2, o + 20, o + 3), (o + 9, o + 31, o + 12), seed=9, m=21)
        surface = tris.copy()
        surface["voxel"] = V.payload((250, 240, 30), 2)
        v, faces = V.icosphere((o + 12.3, o + 16.2, o + 13.4), 5.2)
        bite, carve = FL.mesh(128, v, faces), int(V.payload((0, 0, 0), 0))
        e.update_voxels(*edit)
        e.voxelize_triangles(surface, lo, hi)
        e.fill_triangles(bite, lo, hi, carve)
        mat2, rgb2 = E.apply_numpy(mat1, rgb1, edit)
        mat2, rgb2, _ = V.brute(mat2, rgb2, surface, lo, hi)
        mat2, rgb2, r = FL.brute(mat2, rgb2, bite, lo, hi, carve)
        assert r["voxels"] > 300 and (mat2 == 2).sum() > 500
        e.prepare()
        assert_grid(e, mat2, rgb2, "after an edit, a surface pass, a carving fill and prepare")
        g = fresh(base, mat2, rgb2)
        try:
            six(g)                                    # (the frame counter goes on through a reset: as many launches on both)
            e.reset()
            g.reset()
            assert frame(e).tobytes() == frame(g).tobytes()
        finally:
            g.close()
    finally:
        for s in (e, u, f):
            s.close()


@pytest.mark.parametrize("path", ["host", "device"])
def test_fill_and_surface_pass_take_turns_in_the_shared_scratch(path):
    """The two triangle edits cut one buffer of the context up with one layout (plan_tri_layout), whose head region is toggle words for
    one and ownership words for the other.  On a fresh 128^3 context per path: a fill into 5 x 7 x 40 (nv = 1400, no multiple of 256; two
    toggle words a column), a surface pass into 24^3 (the buffer grows, the head is laid out the other way), a fill into 9 x 5 x 33 (the
    larger buffer under the first layout again), a vrt_update_voxels of a 3^3 host box, and a vrt_distance_field over the union.  After
    every step the whole grid and the step's result equal what the host emulations leave for the same steps, byte for byte."""
    import torch
    device = path == "device"
    mat0, rgb0, _ = R.scene("sunlit")
    fill1 = (FL.mesh(128, [(40.3, 50.4, 31.2), (44.6, 51.1, 45.7), (41.2, 56.5, 52.3), (43.1, 53.3, 68.6)], FL.TET), (40, 50, 30), (45, 57, 70))
    surface = (V.triangles(128, [[(45.2, 53.1, 41.3), (66.7, 55.4, 47.9), (50.3, 74.8, 62.2)], [(67.5, 75.5, 40.5), (44.5, 75.5, 63.5), (67.5, 52.5, 63.5)],
                                 [(30.0, 60.2, 50.1), (90.0, 61.7, 52.4), (55.1, 64.9, 90.0)]]), (44, 52, 40), (68, 76, 64))
    fill2 = (FL.mesh(128, [(38.4, 54.3, 29.1), (46.5, 55.2, 36.6), (39.7, 58.6, 48.2), (45.2, 56.1, 60.3)], FL.TET), (38, 54, 28), (47, 59, 61))
    box = E._pattern((43, 55, 50), (46, 58, 53), seed=5, m=23)
    lo, hi = (38, 50, 28), (68, 76, 70)
    for (_, l, h), shape in ((fill1, (5, 7, 40)), (surface, (24, 24, 24)), (fill2, (9, 5, 33)), ((None,) + box[:2], (3, 3, 3))):
        assert tuple(b - a for a, b in zip(l, h)) == shape and all(lo[a] <= l[a] and h[a] <= hi[a] for a in range(3))
    keep = []

    def given(tris):
        if not device:
            return tris
        keep.append(torch.from_numpy(np.ascontiguousarray(tris).view(np.uint8).reshape(-1).copy()).cuda())
        torch.cuda.synchronize()                      # the tensor is written on torch's stream, read on the context's
        return keep[-1]
    hg, s = E.HostGrid(mat0, rgb0), fresh("sunlit", mat0, rgb0)
    try:
        def step(label, got, rc_want):
            rc, want = rc_want
            assert rc == 0 and want["voxels"] > 0 and V.same_result(got, want), f"{path} path, {label}: result {got} != {want}"
            assert_grid(s, hg.mat, hg.rgb, f"{path} path, {label}")
        step("fill into 5 x 7 x 40", s.fill_triangles(given(fill1[0]), *fill1[1:], FL.PAY), FL.emul_call(hg, *fill1, FL.PAY))
        step("surface pass into 24^3", s.voxelize_triangles(given(surface[0]), *surface[1:]), V.emul_call(hg, *surface, once=device))
        step("fill into 9 x 5 x 33", s.fill_triangles(given(fill2[0]), *fill2[1:], FL.PAY), FL.emul_call(hg, *fill2, FL.PAY))
        s.update_voxels(*box)
        assert hg.apply(*box) == 0
        assert_grid(s, hg.mat, hg.rgb, f"{path} path, update of a 3^3 box")
        rc, d2, near = D.emul_call(hg.mat, lo, hi, 400)
        assert rc == 0 and (d2 == 0).any() and (d2 > 0).any()
        if device:
            out = tuple(torch.full(d2.shape, 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in range(2))
            torch.cuda.synchronize()
            s.distance_field(lo, hi, 400, nearest=True, out=out)
            s.sync()
            got = tuple(t.cpu().numpy() for t in out)
        else:
            got = s.distance_field(lo, hi, 400, nearest=True)
        D.check(*got, (d2, near), f"{path} path, distance field over the union")
        assert_grid(s, hg.mat, hg.rgb, f"{path} path, after the distance field")
    finally:
        s.close()


def test_error_codes_empty_calls_and_a_null_result():
    lib = _lib.load()
    mat, rgb, params = R.scene("sunlit")
    one = FL.mesh(128, np.array([(60.25, 70.25, 60.25), (60.75, 70.3, 60.3), (60.3, 70.75, 60.25), (60.5, 70.5, 60.75)]), FL.TET)   # around the centre of cell (60, 70, 60)
    poison = np.full(1, -1, np.int64).repeat(5).view(np.uint8)[:40].copy()

    def call(s, lo, hi, tris=one, n=None, on_device=0, result="fresh"):
        res = poison.copy() if isinstance(result, str) else result
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        rc = lib.vrt_fill_triangles(C.c_void_p(s._ctx), len(tris) if n is None else n, p(tris), None if lo is None else (C.c_int32 * 3)(*lo),
                                    None if hi is None else (C.c_int32 * 3)(*hi), FL.PAY, p(res), on_device)
        return rc, res
    s = NativeSession(lib, "vrt_", config("sunlit"))
    try:
        assert call(s, (1, 1, 1), (2, 2, 2))[0] == _abi.VRT_E_STATE                   # before vrt_prepare
        orc.setup(s, mat, rgb, params)
        s.upload_voxels(mat, rgb)
        assert call(s, (1, 1, 1), (2, 2, 2))[0] == _abi.VRT_E_STATE                   # after an upload that no prepare has followed
        with pytest.raises(NativeError):
            s.fill_triangles(one, (1, 1, 1), (2, 2, 2), FL.PAY)
        with pytest.raises(NativeError):              # an empty array meets the same checks of box and state
            s.fill_triangles(one[:0], (1, 1, 1), (2, 2, 2), FL.PAY)
        s.prepare()
        import torch
        with pytest.raises(ValueError):               # a tensor in host memory never reaches the device path
            s.fill_triangles(torch.from_numpy(one.view(np.uint8).reshape(-1).copy()), (56, 66, 56), (64, 74, 64), FL.PAY)
        with pytest.raises(NativeError):
            s.fill_triangles(one[:0], (2, 1, 1), (1, 2, 2), FL.PAY)
        assert not s.fill_triangles(one[:0], (0, 0, 0), (128, 128, 128), FL.PAY).tobytes().strip(b"\0")
        assert not s.fill_triangles(torch.zeros(0, dtype=torch.uint8, device="cuda"), (0, 0, 0), (128, 128, 128), FL.PAY).tobytes().strip(b"\0")
        for lo, hi in (((2, 1, 1), (1, 2, 2)), ((-1, 0, 0), (0, 1, 1)), ((127, 127, 127), (128, 128, 129)), ((0, 200, 0), (1, 201, 1))):
            assert call(s, lo, hi)[0] == _abi.VRT_E_INVALID, (lo, hi)
        assert call(s, None, (1, 1, 1))[0] == call(s, (0, 0, 0), None)[0] == call(s, (0, 0, 0), (1, 1, 1), tris=None, n=1)[0] == _abi.VRT_E_INVALID
        assert call(s, (0, 0, 0), (1, 1, 1), n=-1)[0] == call(s, (0, 0, 0), (1, 1, 1), n=2 ** 32 - 1)[0] == _abi.VRT_E_INVALID
        assert call(s, (0, 0, 0), (1, 1, 1), on_device=2)[0] == call(s, (0, 0, 0), (1, 1, 1), on_device=-1)[0] == _abi.VRT_E_INVALID
        for field in ("reserved0", "reserved1"):
            bad = one.copy()
            bad[field][2] = 7
            assert call(s, (0, 0, 0), (128, 128, 128), tris=bad)[0] == _abi.VRT_E_INVALID
        for lo, hi, n in (((5, 5, 5), (5, 9, 9), None), ((128, 128, 128), (128, 128, 128), None), ((0, 0, 0), (128, 128, 128), 0)):
            rc, res = call(s, lo, hi, n=n)
            assert rc == _abi.VRT_OK and not res.any(), (lo, hi, n)                   # nothing done, the result zeroed
        assert_grid(s, mat, rgb, "after the refused and the empty calls")
        rc, _ = call(s, (56, 66, 56), (64, 74, 64), result=None)                      # a NULL result
        assert rc == _abi.VRT_OK
        m, c = whole_grid(s)
        assert m[60, 70, 60] == 11 and (m != mat).sum() == 1 and c[60, 70, 60].tolist() == [90, 160, 230]
        rc, res = call(s, (56, 66, 56), (64, 74, 64))
        r = res.view(_abi.VOXELIZE_RESULT)[0]
        assert rc == _abi.VRT_OK and r["lo"].tolist() == [60, 70, 60] and r["hi"].tolist() == [61, 71, 61] and r["voxels"] == 1 and r["invalid"] == 0
        # on the device path a reserved word makes the triangle invalid: the tetrahedron is open, and counted
        bad = one.copy()
        bad["reserved0"][3] = 1
        t = torch.from_numpy(bad.view(np.uint8).reshape(-1).copy()).cuda()
        torch.cuda.synchronize()
        want = FL.brute(m, c, bad, (56, 66, 56), (64, 74, 64), FL.PAY)
        got = s.fill_triangles(t, (56, 66, 56), (64, 74, 64), FL.PAY)
        assert got["invalid"] == 1 and FL.same_result(got, want[2])
        assert_grid(s, want[0], want[1], "reserved word on the device path")
    finally:
        s.close()


def test_renderer_fill_triangles_equals_authoring_the_grid():
    from voxel_rt2_amd.renderer import Renderer

    def renderer():
        r = Renderer(dx=1 / 64, image_res=(W, H), up=(0, 1, 0), voxel_edges=0.06, exposure=1.5, max_depth=DEPTH, seed=SEED, sky_res=0)
        r.set_directional_light((0.6, 1.0, 0.4), 0.1, (1.0, 0.95, 0.85))
        r.background_color[None] = (0.35, 0.5, 0.75)
        r.floor_height[None] = -0.3
        return r
    first = [((x, -3, z), 11, (0.8, 0.3, 0.2)) for x in range(-6, 7) for z in range(-6, 7)]
    v, faces = V.icosphere((0.05, 0.12, -0.03), 0.11, 1)                                  # world units: 80 triangles
    bv, bf = V.icosphere((0.11, 0.15, -0.02), 0.05, 0)

    def records(vv, ff):
        t = np.zeros(len(ff), V.TRI)
        t["v0"], t["v1"], t["v2"] = (np.asarray(vv, np.float32)[ff][:, k] for k in range(3))
        return t
    e, f = renderer(), renderer()
    try:
        with pytest.raises(NativeError):
            e.fill_triangles(v, faces)
        for vox in first:
            e.set_voxel(*vox)
        e.prepare_data()
        e.set_voxel((9, -3, 9), 2, (1.0, 1.0, 1.0))                                       # not yet sent: goes first
        base_m, base_c = e.voxel_material.copy(), e.voxel_color.copy()
        assert base_m[9 + 64, -3 + 64, 9 + 64] == 2
        box = e.mesh_box(v)
        r1 = e.fill_triangles(v, faces, color=(200, 120, 40), mat=54)                      # lo, hi: mesh_box
        assert e.current_spp == 0
        bm, bc, b1 = FL.brute(base_m, base_c, records(v, faces), *box, V.payload((200, 120, 40), 54))
        assert FL.same_result(r1, b1) and r1["voxels"] > 1000 and r1["invalid"] == 0
        assert e.voxel_material.tobytes() == bm.tobytes() and e.voxel_color.tobytes() == bc.tobytes()
        r2 = e.fill_triangles(bv, bf, color=(1, 2, 3), mat=0, reset=False)                 # a bite carved out
        bm, bc, b2 = FL.brute(bm, bc, records(bv, bf), *e.mesh_box(bv), V.payload((1, 2, 3), 0))
        assert FL.same_result(r2, b2) and r2["voxels"] > 50
        # solid plus conservative skin: brute-force fill, then brute-force surface, and the record of their union
        sv, sf = V.icosphere((-0.2, 0.1, 0.1), 0.07, 1)
        r3 = e.fill_triangles(sv, sf, color=(30, 220, 90), mat=2, shell=True)
        srec = records(sv, sf)
        srec["voxel"] = V.payload((30, 220, 90), 2)
        sbox = e.mesh_box(sv)
        before = bm.copy()
        bm, bc, b3 = FL.brute(bm, bc, srec, *sbox, V.payload((30, 220, 90), 2))
        bm, bc, b4 = V.brute(bm, bc, srec, *sbox)
        union = np.argwhere((bm == 2) & (before != 2))
        assert b3["voxels"] < len(union) and b4["voxels"] < len(union) < b3["voxels"] + b4["voxels"]
        assert r3["voxels"] == len(union) and r3["lo"].tolist() == union.min(axis=0).tolist() and r3["hi"].tolist() == (union.max(axis=0) + 1).tolist() and r3["invalid"] == 0
        m, c = e.session.fetch_voxels((0, 0, 0), (128, 128, 128))
        assert m.tobytes() == bm.tobytes() and c.tobytes() == bc.tobytes()
        assert e.voxel_material.tobytes() == m.tobytes() and e.voxel_color.tobytes() == c.tobytes()     # the host mirror is in step
        import torch
        with pytest.raises(ValueError):
            e.fill_triangles(torch.zeros(48, dtype=torch.uint8, device="cuda"), shell=True)
        f.set_voxel_arrays(m, c)
        f.prepare_data()
        for r in (e, f):
            r.accumulate(4)
        assert e.fetch_hdr().tobytes() == f.fetch_hdr().tobytes() and e.fetch_hdr().std() > 0
    finally:
        e.session.close()
        f.session.close()


def test_fill_mesh_example_runs(tmp_path, monkeypatch):
    import sys
    for k, v in (("VRT_RES", "64x40"), ("VRT_FRAMES", "2"), ("VRT_SKY_RES", "32"), ("VRT_MAX_DEPTH", "2"), ("VRT_OUT", str(tmp_path / "fill.png"))):
        monkeypatch.setenv(k, v)
    monkeypatch.syspath_prepend(ROOT)
    sys.modules.pop("scene", None)
    mod = runpy.run_path(os.path.join(ROOT, "examples", "fill_mesh.py"), run_name="fill_mesh")
    r, results = mod["main"]()
    try:
        assert (tmp_path / "fill.png").exists()
        assert all(res["voxels"] > 0 and res["invalid"] == 0 for res in results.values())
        m, c = r.session.fetch_voxels((0, 0, 0), (r.voxel_grid_res,) * 3)
        assert r.voxel_material.tobytes() == m.tobytes() and r.voxel_color.tobytes() == c.tobytes()
        lo, hi = results["sphere"]["lo"], results["sphere"]["hi"]
        centre = tuple(int(x) for x in (lo + hi) // 2)
        assert m[centre] == 2                                                             # solid: the middle of the ball is filled
        assert results["carve"]["voxels"] > 0 and (m == 54).sum() > 0
    finally:
        r.session.close()
