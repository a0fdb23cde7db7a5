"""vrt_cast_rays and vrt_fetch_voxels ON THE DEVICE, bit for bit (tests/cast.py holds scenes, ray families, the oracle's records and the
comparison; every float is compared by its bits, any NaN equal to any NaN):
  - every ray family on every scene == the oracle's next_hit: the first function-level check of the device's next_hit, floor quirk,
    tie rule and edge darkening included;
  - the host path and the device path (torch tensors) give identical bytes, and so do the two instantiations of the kernel, each
    forced by a batch on its side of the switch-over;
  - batches that are no multiple of the workgroup or of the staging chunk, and one larger than a grid's stride;
  - a query queued before / after an edit sees the old / new grid;
  - frames rendered with queries interleaved == frames rendered without: HDR and both histories;
  - error codes; pick == cast_rays(pick_ray); pick_ray == the oracle's cast direction; fetch_voxels after host and device edits;
    sync_voxels_from_device."""
import ctypes as C

import numpy as np
import pytest

import cast as K
import edit as E
import orc
import rays as R
from voxel_rt2_amd import _abi, _lib, host
from voxel_rt2_amd._session import NativeError, NativeSession

pytestmark = pytest.mark.gpu


def session(name, reference_indexing=False, **kw):
    s = NativeSession(_lib.load(), "vrt_", K.config(name, **kw))
    mat, rgb, params = K.scene(name)
    orc.setup(s, mat, rgb, params)
    if reference_indexing:
        s.set_reference_indexing(True)
    return s


@pytest.fixture(scope="module")
def live():
    """live(scene): one prepared context per scene, shared by the tests that only ask it questions."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = session(name)
        return made[name]
    yield get
    for s in made.values():
        s.close()


def device_cast(s, rays):
    """The device path: tensors on the device, the work queued on the context's stream, read back after a sync."""
    import torch
    t_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1)).cuda()
    t_hits = torch.full((len(rays) * _abi.HIT.itemsize,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                          # the tensors are written on torch's stream, read on the context's
    s.cast_rays(t_rays, t_hits)
    s.sync()
    return t_hits.cpu().numpy().view(_abi.HIT)


def tiled(rays, want, n):
    k = -(-n // len(rays))
    return np.tile(rays, k)[:n], np.tile(want, k)[:n]


@pytest.mark.parametrize("scene,fam", K.cases())
def test_device_equals_oracle(live, scene, fam):
    rays, want, _ = K.family(scene, fam)
    K.check(live(scene).cast_rays(rays), rays, want, f"{scene}/{fam}")


@pytest.mark.parametrize("scene", ["sunlit", "s1_256"])
def test_paths_and_instantiations_give_identical_bytes(live, scene):
    """n on either side of the switch-over forces either instantiation; host arrays and device tensors go through the same kernel."""
    n0 = K.switch_over()
    rays = np.concatenate([K.family(scene, f)[0] for f in ("random", "edges", "floor", "invalid")])
    want = np.concatenate([K.family(scene, f)[1] for f in ("random", "edges", "floor", "invalid")])
    s = live(scene)
    for n in sorted({1, 63, min(n0 - 1, len(rays)), n0, n0 + 257}):
        if n < 1:
            continue
        r, w = tiled(rays, want, n)
        a, b = s.cast_rays(r), device_cast(s, r)
        K.check(a, r, w, f"{scene} host path n={n}")
        assert a.tobytes() == b.tobytes(), f"{scene} n={n}: host and device path differ in {K.mismatches(a, b).size} records"
    # the same rays through both instantiations: as one batch above the switch-over, and in pieces below it
    r, w = tiled(rays, want, max(n0 + 257, len(rays)))
    whole = s.cast_rays(r)
    step = max(1, n0 - 1)
    pieces = np.concatenate([s.cast_rays(r[i:i + step]) for i in range(0, min(len(r), 8 * step), step)])
    assert whole[:len(pieces)].tobytes() == pieces.tobytes()
    K.check(whole, r, w, f"{scene} staged")


def test_odd_batches_chunks_and_more_than_a_grid(live):
    s = live("sunlit")
    rays = np.concatenate([K.family("sunlit", f)[0] for f in ("random", "edges", "inside")])
    want = np.concatenate([K.family("sunlit", f)[1] for f in ("random", "edges", "inside")])
    chunk = K.lib().cast_emul_chunk()
    for n in (255, 257, chunk + 777):                 # the host path stages chunk + 777 rays in two pieces
        r, w = tiled(rays, want, n)
        K.check(s.cast_rays(r), r, w, f"host path n={n}")
    n = 2048 * 256 + 131                              # more workgroups' worth than any residency (256 CUs x 8): lanes take several turns
    r, w = tiled(rays, want, n)
    K.check(device_cast(s, r), r, w, f"device path n={n}")


def test_a_query_sees_the_grid_as_queued():
    import torch
    s = session("one_voxel")
    try:
        ray = np.zeros(1, _abi.RAY)
        ray["origin"], ray["dir"], ray["t_max"] = (127.5 / 64 - 1, 0.9, 0.5 / 64 - 1), (0.0, -1.0, 0.0), np.inf
        t_ray = torch.from_numpy(ray.view(np.uint8).reshape(-1)).cuda()
        before, after = (torch.zeros(48, dtype=torch.uint8, device="cuda") for _ in range(2))
        gone = (torch.zeros(1, dtype=torch.int8, device="cuda"), torch.zeros(3, dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        s.cast_rays(t_ray, before)                    # queued, not waited for
        s.update_voxels((127, 64, 0), (128, 65, 1), gone[0].data_ptr(), gone[1].data_ptr(), on_device=True)
        s.cast_rays(t_ray, after)
        s.sync()
        b, a = before.cpu().numpy().view(_abi.HIT)[0], after.cpu().numpy().view(_abi.HIT)[0]
        assert b["kind"] == _abi.HIT_VOXEL and b["cell"].tolist() == [127, 64, 0] and b["mat_id"] == 11
        assert a["kind"] == _abi.HIT_FLOOR and a["cell"].tolist() == [-1, -1, -1]
        assert s.cast_rays(ray)[0].tobytes() == a.tobytes()
    finally:
        s.close()


def test_frames_do_not_notice_queries():
    """accumulate(4) x 3 with queries in between, on the host path and on the device path: HDR and both histories as without them."""
    import torch
    rays = np.concatenate([K.family("sunlit", "random")[0], K.family("sunlit", "edges")[0]])
    t_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
    t_hits = torch.zeros(len(rays) * 48, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def run(query):
        s = session("sunlit", width=64, height=40)
        try:
            for k in range(3):
                s.accumulate(4)
                if query == "host":
                    s.cast_rays(rays[:1 + 997 * k])
                elif query == "device":
                    s.cast_rays(t_rays, t_hits)
            return [s.fetch_hdr()] + [s.fetch_buffer(w) for w in (_abi.BUF_HISTORY_DIFFUSE, _abi.BUF_HISTORY_SPECULAR)], s.stats()
        finally:
            s.close()
    plain, stats = run(None)
    assert plain[0].std() > 0
    for query in ("host", "device"):
        got, st = run(query)
        for a, b, what in zip(got, plain, ("hdr", "diffuse history", "specular history")):
            assert a.tobytes() == b.tobytes(), f"{query} queries changed the {what}: {(a != b).sum()} of {a.size} values"
        for key in ("path_samples", "render_launches", "temporal_launches", "rays"):
            assert st[key] == stats[key], (query, key)


def test_error_codes():
    lib = _lib.load()
    mat, rgb, params = K.scene("sunlit")
    r, h = np.zeros(4, _abi.RAY), np.zeros(4, _abi.HIT)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    cast = lambda s, n=4, rr=r, hh=h, dev=0: lib.vrt_cast_rays(C.c_void_p(s._ctx), n, p(rr), p(hh), dev)
    box = lambda v: (C.c_int32 * 3)(*v)
    m, c = np.zeros((1, 1, 1), np.int8), np.zeros((1, 1, 1, 3), np.uint8)
    fetch = lambda s, lo=(1, 1, 1), hi=(2, 2, 2), mm=m, cc=c, dev=0: lib.vrt_fetch_voxels(C.c_void_p(s._ctx), None if lo is None else box(lo),
                                                                                     None if hi is None else box(hi), p(mm), p(cc), dev)
    s = NativeSession(lib, "vrt_", K.config("sunlit"))
    try:
        assert cast(s) == fetch(s) == _abi.VRT_E_STATE                                 # before vrt_prepare
        orc.setup(s, mat, rgb, params)
        s.upload_voxels(mat, rgb)
        assert cast(s) == fetch(s) == _abi.VRT_E_STATE                                 # after an upload that no prepare has followed
        with pytest.raises(NativeError):
            s.cast_rays(r)
        s.prepare()
        assert cast(s) == fetch(s) == _abi.VRT_OK
        assert cast(s, rr=None) == cast(s, hh=None) == cast(s, n=-1) == cast(s, dev=2) == cast(s, dev=-1) == _abi.VRT_E_INVALID
        assert cast(s, n=0) == _abi.VRT_OK
        assert fetch(s, lo=None) == fetch(s, hi=None) == fetch(s, mm=None) == fetch(s, cc=None) == fetch(s, dev=2) == _abi.VRT_E_INVALID
        for lo, hi in (((2, 1, 1), (1, 2, 2)), ((-1, 0, 0), (0, 1, 1)), ((127, 127, 127), (128, 128, 129))):
            assert fetch(s, lo, hi) == _abi.VRT_E_INVALID, (lo, hi)
        assert fetch(s, (5, 5, 5), (5, 9, 9)) == fetch(s, (128, 128, 128), (128, 128, 128)) == _abi.VRT_OK   # empty boxes
        assert len(s.cast_rays(np.zeros(0, _abi.RAY))) == 0 and s.fetch_voxels((3, 3, 3), (3, 4, 4))[0].shape == (0, 1, 1)
    finally:
        s.close()


def renderer(w=32, h=16):
    from voxel_rt2_amd.renderer import Renderer
    r = Renderer(dx=1 / 64, image_res=(w, h), up=(0, 1, 0), voxel_edges=0.06, exposure=1.5, max_depth=2, seed=7, sky_res=0)
    r.floor_height[None] = -0.3
    for x in range(-20, 21):
        for z in range(-20, 21):
            r.set_voxel((x, -3 + (x * z) % 3, z), 11, (0.8, 0.3, 0.2))
    return r


def test_pick_is_cast_rays_of_pick_ray():
    r = renderer()
    try:
        with pytest.raises(NativeError):
            r.pick(3, 3)                                                              # nothing prepared yet
        r.prepare_data()
        kinds = set()
        for u, v in ((0, 0), (16, 7), (31, 15), (15, 4), (20, 2), (16, 15)):
            o, d = r.pick_ray(u, v)
            a, b = r.pick(u, v), r.cast_rays(o, d)[0]
            assert a.tobytes() == b.tobytes()
            kinds.add(int(a["kind"]))
        assert kinds == {_abi.HIT_MISS, _abi.HIT_FLOOR, _abi.HIT_VOXEL}, kinds
        hit = r.pick(16, 7)
        assert hit["kind"] == _abi.HIT_VOXEL and r.voxel_material[tuple(hit["cell"])] == 11
        shadow = r.cast_rays(*r.pick_ray(16, 7), any_hit=True)[0]
        assert shadow["t"] == hit["t"] and shadow["mat_id"] == 0 and r.cast_rays(*r.pick_ray(16, 7), t_max=hit["t"])[0]["kind"] == _abi.HIT_MISS
    finally:
        r.session.close()


def test_pick_ray_equals_the_oracles_cast_direction():
    """Every pixel of a 32 x 16 camera against orc_unit_cast_dir with camera_is_moving = 1 (no jitter): bit equality -- pick_ray follows
    get_cast_dir's float32 statements in their order."""
    r = renderer()
    r.set_camera_pos(0.7, 0.9, 1.6)
    from voxel_rt2_amd import camera as cam_mod
    view, proj = cam_mod.default_matrices(32, 16, pos=(0.7, 0.9, 1.6), look=(0.1, -0.2, 0.0), fov=float(np.deg2rad(38.0)))
    r.set_view_mat(cam_mod.to_glm_memory(view))
    r.set_proj_mat(cam_mod.to_glm_memory(proj))
    o = orc.Oracle(host.make_config(32, 16, max_depth=2, seed=7), threads=1)
    try:
        o.set_camera(host.make_camera(view, proj, (0.7, 0.9, 1.6), jitter_index=1, moving=True))
        worst = 0.0
        for v in range(16):
            for u in range(32):
                origin, d = r.pick_ray(u, v)
                want = o.cast_dir(u, v)
                worst = max(worst, float(np.abs(d - want).max()))
                assert d.tobytes() == want.tobytes(), f"pixel ({u}, {v}): {d} != {want}; largest component difference so far {worst}"
                assert origin.tolist() == np.array((0.7, 0.9, 1.6), np.float32).tolist()
    finally:
        o.close()
        r.session.close()


def test_fetch_voxels_after_host_and_device_edits():
    import torch
    name = "unaligned"
    base, edits = E.sequence(name)
    states = E.grids(name)
    s = session("sunlit")
    try:
        G = 128
        m, c = s.fetch_voxels((0, 0, 0), (G, G, G))
        assert m.tobytes() == states[0][0].tobytes() and c.tobytes() == states[0][1].tobytes()
        s.update_voxels(*edits[0])                                                     # from host arrays
        lo, hi, bm, bc = edits[1]
        keep = (torch.from_numpy(np.ascontiguousarray(bm)).cuda(), torch.from_numpy(np.ascontiguousarray(bc)).cuda())
        torch.cuda.synchronize()
        s.update_voxels(lo, hi, keep[0].data_ptr(), keep[1].data_ptr(), on_device=True)   # from device memory: the host never saw it
        mat, rgb = states[2]
        for lo, hi in (((0, 0, 0), (G, G, G)), E.UNALIGNED, ((2, 4, 60), (9, 71, 69)), ((127, 127, 127), (128, 128, 128)), ((0, 0, 0), (1, 128, 1))):
            sl = tuple(slice(l, h) for l, h in zip(lo, hi))
            m, c = s.fetch_voxels(lo, hi)
            assert m.tobytes() == mat[sl].tobytes() and c.tobytes() == rgb[sl].tobytes(), (lo, hi)
        lo, hi = (2, 4, 60), (9, 71, 69)                                              # and into device memory
        shape = tuple(h - l for l, h in zip(lo, hi))
        tm, tc = torch.zeros(shape, dtype=torch.int8, device="cuda"), torch.zeros(shape + (3,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        s.fetch_voxels(lo, hi, tm.data_ptr(), tc.data_ptr(), on_device=True)
        s.sync()
        sl = tuple(slice(l, h) for l, h in zip(lo, hi))
        assert tm.cpu().numpy().tobytes() == mat[sl].tobytes() and tc.cpu().numpy().tobytes() == rgb[sl].tobytes()
    finally:
        s.close()


def test_sync_voxels_from_device_then_get_voxel():
    import torch
    r = renderer()
    try:
        r.prepare_data()
        hit = r.pick(16, 7)
        cell = hit["cell"] + (hit["normal"] > 0.5).astype(np.int32) - (hit["normal"] < -0.5).astype(np.int32)   # the cell in front of the hit face
        new = (torch.full((1, 1, 1), 54, dtype=torch.int8, device="cuda"), torch.tensor([[[[10, 200, 30]]]], dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        r.session.update_voxels(cell, cell + 1, new[0].data_ptr(), new[1].data_ptr(), on_device=True)
        idx = tuple(int(v) - 64 for v in cell)
        assert r.get_voxel(idx)[0] == 0                                                 # the host does not know yet
        r.sync_voxels_from_device(cell - 1, cell + 2)
        m, col = r.get_voxel(idx)
        assert m == 54 and np.allclose(col, (10 / 255, 200 / 255, 30 / 255), atol=1e-6)
        assert r.dirty_box()[0] == r.dirty_box()[1]                                     # nothing to send back
        again = r.pick(16, 7)
        assert again["cell"].tolist() == cell.tolist() and again["mat_id"] == 54 and again["t"] < hit["t"]
        r.sync_voxels_from_device()
        assert r.voxel_material[tuple(cell)] == 54 and (r.voxel_material > 0).sum() == 41 * 41 + 1
    finally:
        r.session.close()
