"""vrt_trace_radiance ON THE DEVICE, bit for bit (tests/radiance.py holds the cases, the oracle's values and the comparison; every float
is compared by its bits, any NaN equal to any NaN):
  - every case == the oracle's render body: pose by pose on the host path (small launches: the pyramid in global memory) and all poses
    in one batch on the device path, tiled until the launch walks on the staged pyramid;
  - 2 048 rays x 600 samples take more than one chunk: 64 of the rays against the oracle, all of them against the same rays reversed;
  - 1, 63, 64, 65 and 257 rays x 3 samples == the host build: a wave's reservation, its short last one, a second workgroup;
  - one ray x 4 096 samples == the ordered sum of 4 096 one-sample calls;
  - a query queued before / after an edit sees the old / new grid; frames rendered with queries interleaved == frames rendered without,
    a pending deferred accumulation included; vrt_get_stats does not notice queries;
  - error codes; Renderer.trace_radiance with arrays and with tensors; render_panorama."""
import ctypes as C

import numpy as np
import pytest

import radiance as X
from voxel_rt2_amd import _abi, _lib
from voxel_rt2_amd._session import NativeError, NativeSession

pytestmark = pytest.mark.gpu


def session(case, **kw):
    return X.start(NativeSession(_lib.load(), "vrt_", X.config(case, **kw)), case)


def device_trace(s, rays, samples, first_frame=X.FIRST_FRAME, sync=True):
    """The device path: tensors on the device, the work queued on the context's stream, read back after a sync."""
    import torch
    t_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1)).cuda()
    t_out = torch.full((len(rays) * _abi.RADIANCE.itemsize,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                          # the tensors are written on torch's stream, read on the context's
    s.trace_radiance(t_rays, samples, first_frame, t_out)
    if not sync:
        return t_rays, t_out
    s.sync()
    return t_out.cpu().numpy().view(_abi.RADIANCE)


@pytest.mark.parametrize("case", [c for c in X.CASES if c != "one_voxel_d2"])
def test_device_equals_oracle(case):
    want = X.expected(case)
    s = session(case)
    try:
        for pose, (rays, recs) in want.items():
            for n, rec in recs.items():
                assert not X.lib().radiance_emul_staged(len(rays) * n, -1)
                X.check(s.trace_radiance(rays, n, X.FIRST_FRAME), rays, rec, f"{case} pose {pose} samples {n} host path")
        n = max(X.SAMPLES[case])
        rays = np.concatenate([want[p][0] for p in want])
        rec = np.concatenate([want[p][1][n] for p in want])
        k = 1
        while not X.lib().radiance_emul_staged(k * len(rays) * n, -1):
            k += 1
        rays, rec = np.tile(rays, k), np.tile(rec, k)
        assert len(X.chunks(len(rays), n)) == 1
        X.check(device_trace(s, rays, n), rays, rec, f"{case} all poses x {k}, samples {n}, device path, staged")
        X.check(s.trace_radiance(rays[:len(rays) // k + 37], n, X.FIRST_FRAME), rays, rec[:len(rays) // k + 37], f"{case} host path, odd batch")
    finally:
        s.close()


def test_more_than_one_chunk():
    case, Wd, Hd, spp = "one_voxel_d2", 64, 32, 600
    assert len(X.chunks(Wd * Hd, spp)) > 1                                             # at the committed budget (plan_query_chunk)
    o = X.start(X.ShimOracle(X.config(case, Wd, Hd)), case)
    o.set_camera(X.camera("default", 0, Wd, Hd))
    uv = np.array([(u, v) for v in range(Hd) for u in range(Wd)], np.int32)
    rays = X.camera_rays(o, "default", uv, Wd)
    pick = np.arange(64) * 32 + (np.arange(64) * 7) % 32                               # a fixed subset: two pixels of every row
    rgb = o.radiance(uv[pick], spp, X.FIRST_FRAME)
    o.close()
    s = session(case)
    try:
        got = device_trace(s, rays, spp)
        back = device_trace(s, rays[::-1], spp)[::-1]
        assert got.tobytes() == back.tobytes(), f"{X.mismatches(got, back).size} records depend on the order of the rays"
        assert got["rgb"][pick].tobytes() == rgb.tobytes(), f"{(got['rgb'][pick] != rgb).any(axis=1).sum()} of 64 rays differ from the oracle"
        assert s.trace_radiance(rays[pick], spp, X.FIRST_FRAME).tobytes() == got[pick].tobytes()   # one chunk on the host path
        assert (got["rgb"] > 0).any() and np.isinf(got["t"]).any() and np.isfinite(got["t"]).any()
    finally:
        s.close()


@pytest.fixture(scope="module")
def one_voxel_rays():
    """The 64 x 32 camera rays of the one_voxel case's default pose, and the case's scene for the host build."""
    case, Wd, Hd = "one_voxel_d2", 64, 32
    o = X.start(X.ShimOracle(X.config(case, Wd, Hd)), case)
    o.set_camera(X.camera("default", 0, Wd, Hd))
    rays = X.camera_rays(o, "default", np.array([(u, v) for v in range(Hd) for u in range(Wd)], np.int32), Wd)
    o.close()
    return rays, X.HostScene(case)


@pytest.mark.parametrize("n_rays", [1, 63, 64, 65, 257])
def test_batch_sizes_around_a_waves_reservation(one_voxel_rays, n_rays):
    """A wave's take of 64 items, its short last take and a second workgroup (WaveItems, vrt_query_kernels.hip): 3 samples of n_rays rays on
    the device path against the host build of the same functions, byte for byte."""
    rays, host_scene = one_voxel_rays
    rays = rays[(np.arange(n_rays) * 5) % len(rays)]
    want = host_scene.trace(rays, 3)
    s = session("one_voxel_d2")
    try:
        got = device_trace(s, rays, 3)
        assert got.tobytes() == want.tobytes(), f"{X.mismatches(got, want).size} of {n_rays} records differ from the host build's"
    finally:
        s.close()


def test_one_ray_many_samples_is_the_ordered_sum_of_its_samples():
    import torch
    case, spp = "sunlit_d5", 4096
    ray = X.expected(case)["street"][0][[70]]
    s = session(case)
    try:
        whole = s.trace_radiance(ray, spp, 11)[0]
        t_ray = torch.from_numpy(ray.view(np.uint8).reshape(-1)).cuda()
        t_out = torch.zeros((spp, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for k in range(spp):                                                           # 4 096 one-sample calls, queued
            s.trace_radiance(t_ray, 1, 11 + k, t_out[k])
        s.sync()
        one = t_out.cpu().numpy()
        acc = np.zeros(3, np.float32)
        for k in range(spp):
            acc = acc + one[k, :3]
        assert (acc / np.float32(spp)).astype(np.float32).tobytes() == whole["rgb"].tobytes()
        assert (one[:, 3] == whole["t"]).all() and len(np.unique(one[:, :3], axis=0)) > spp // 4 and whole["rgb"].min() > 0
        assert device_trace(s, ray, spp, 11)[0].tobytes() == whole.tobytes()
    finally:
        s.close()


def test_a_query_sees_the_grid_as_queued():
    import torch
    s = session("one_voxel_d2")
    try:
        ray = np.zeros(1, _abi.PATH_RAY)
        ray["origin"], ray["dir"], ray["stream"] = (127.5 / 64 - 1, 0.9, 0.5 / 64 - 1), (0.0, -1.0, 0.0), 9
        t_ray = torch.from_numpy(ray.view(np.uint8).reshape(-1)).cuda()
        before, after = (torch.zeros(4, dtype=torch.float32, device="cuda") for _ in range(2))
        gone = (torch.zeros(1, dtype=torch.int8, device="cuda"), torch.zeros(3, dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        s.trace_radiance(t_ray, 8, 0, before)         # queued, not waited for
        s.update_voxels((127, 64, 0), (128, 65, 1), gone[0].data_ptr(), gone[1].data_ptr(), on_device=True)
        s.trace_radiance(t_ray, 8, 0, after)
        s.sync()
        b, a = before.cpu().numpy(), after.cpu().numpy()
        hit = np.zeros(1, _abi.RAY)
        hit["origin"], hit["dir"], hit["t_max"] = ray["origin"], ray["dir"], np.inf
        assert b[3] == np.float32(0.9) - np.float32(65 / 64 - 1) and a[3] == s.cast_rays(hit)[0]["t"] and a[3] > b[3]
        assert b[:3].tobytes() != a[:3].tobytes() and s.trace_radiance(ray, 8, 0)[0].tobytes() == a.tobytes()
    finally:
        s.close()


def test_frames_and_stats_do_not_notice_queries():
    """accumulate(4) x 3 with queries in between, on the host path and on the device path: HDR, both histories and the stats as without
    them.  Every query of the sequence finds a deferred accumulation pending: the contexts run the overlapped pipeline (pipeline_flags
    bit 0) and the library's own plan (plan_pipeline_shape, compiled for the host) accumulates more than three launches of this size in
    one pass, so no pass is queued before the first fetch -- asserted below, since looking (vrt_get_stats) would force it."""
    import os
    import plan
    case = "sunlit_d5"
    defer_k = plan.shape(64 * 40 * 4, int(os.environ.get("GPU_MAX_HW_QUEUES", 4)))[1]
    assert defer_k > 3, f"launches of 64 x 40 x 4 items are accumulated {defer_k} at a time: no accumulation stays pending across the queries"
    rays = np.concatenate([r for r, _ in X.expected(case).values()])
    keep = []

    def run(query):
        s = session(case, width=64, height=40)
        try:
            for k in range(3):
                s.accumulate(4)
                if query == "host":
                    s.trace_radiance(rays[:1 + 397 * k], 2, k)
                elif query == "device":
                    keep.append(device_trace(s, rays, 3, k, sync=False))
            return [s.fetch_hdr()] + [s.fetch_buffer(w) for w in (_abi.BUF_HISTORY_DIFFUSE, _abi.BUF_HISTORY_SPECULAR)], s.stats()
        finally:
            s.close()
    plain, stats = run(None)
    assert plain[0].std() > 0
    assert stats["pipeline_flags"] & 1 and stats["render_launches"] == stats["temporal_launches"] == 3, stats
    for query in ("host", "device"):
        got, st = run(query)
        for a, b, what in zip(got, plain, ("hdr", "diffuse history", "specular history")):
            assert a.tobytes() == b.tobytes(), f"{query} queries changed the {what}: {(a != b).sum()} of {a.size} values"
        for key in ("path_samples", "render_launches", "temporal_launches", "gris_launches", "rays", "dda_iters", "occupancy_queries", "closest_hits",
                    "sky_lookups", "pipeline_flags"):
            assert st[key] == stats[key], (query, key)


def test_error_codes():
    lib = _lib.load()
    case = "sunlit_d2"
    mat, rgb, params = X.scene(case)
    r, o = np.zeros(4, _abi.PATH_RAY), np.zeros(4, _abi.RADIANCE)
    r["dir"] = (0.0, -1.0, 0.0)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    call = lambda s, n=4, rr=r, spp=1, oo=o, dev=0: lib.vrt_trace_radiance(C.c_void_p(s._ctx), n, p(rr), spp, 0, p(oo), dev)
    s = NativeSession(lib, "vrt_", X.config(case))
    try:
        assert call(s) == _abi.VRT_E_STATE                                             # before vrt_prepare
        X.start(s, case)
        s.upload_voxels(mat, rgb)
        assert call(s) == _abi.VRT_E_STATE                                             # after an upload that no prepare has followed
        with pytest.raises(NativeError):
            s.trace_radiance(r)
        s.prepare()
        assert call(s) == _abi.VRT_OK
        assert call(s, rr=None) == call(s, oo=None) == call(s, n=-1) == call(s, dev=2) == call(s, dev=-1) == _abi.VRT_E_INVALID
        assert call(s, spp=0) == call(s, spp=-3) == call(s, spp=_abi.RADIANCE_MAX_SAMPLES + 1) == _abi.VRT_E_INVALID
        bad = r.copy()
        bad["reserved"][2] = 1
        assert call(s, rr=bad) == _abi.VRT_E_INVALID and b"reserved" in lib.vrt_last_error()
        assert call(s, n=0) == _abi.VRT_OK and len(s.trace_radiance(np.zeros(0, _abi.PATH_RAY))) == 0
    finally:
        s.close()


def renderer(w=32, h=16):
    from voxel_rt2_amd.renderer import Renderer
    r = Renderer(dx=1 / 64, image_res=(w, h), up=(0, 1, 0), voxel_edges=0.06, exposure=1.5, max_depth=3, seed=7, sky_res=0)
    r.floor_height[None] = -0.3
    r.set_directional_light((0.3, 1.0, 0.2), 0.1, (1.0, 0.9, 0.8))
    r.background_color[None] = (0.2, 0.3, 0.5)
    for x in range(-20, 21):
        for z in range(-20, 21):
            r.set_voxel((x, -3 + (x * z) % 3, z), 11, (0.8, 0.3, 0.2))
    return r


def test_facade_arrays_tensors_and_panorama():
    import torch
    r = renderer()
    try:
        with pytest.raises(NativeError):
            r.trace_radiance((0.0, 0.5, 0.0), (0.0, -1.0, 0.0))                           # nothing prepared yet
        r.prepare_data()
        rng = np.random.default_rng(7)
        o = rng.uniform(-0.5, 0.5, (300, 3)) + (0.0, 0.6, 0.0)
        d = rng.standard_normal((300, 3)) * 3.0
        a = r.trace_radiance(o, d, samples=3, first_frame=2)
        b = r.trace_radiance(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), samples=3, first_frame=2)
        assert a.dtype == _abi.RADIANCE and a.tobytes() == b.tobytes() and (a["rgb"] > 0).any(axis=1).mean() > 0.5
        unit = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        assert r.trace_radiance(o, unit, samples=3, first_frame=2, normalize=False).tobytes() == a.tobytes()
        st = np.arange(300)[::-1].copy()
        c = r.trace_radiance(o[::-1], d[::-1], samples=3, first_frame=2, streams=st)
        assert c[::-1].tobytes() == a.tobytes()                                           # a ray's stream, not its place, keys its samples
        Wp, Hp, origin = 32, 16, (0.1, 0.2, -0.05)
        pano = r.render_panorama(origin, Wp, Hp, 2)
        dirs = r.panorama_dirs(Wp, Hp)
        assert pano.shape == (Hp, Wp, 3) and pano.dtype == np.float32
        assert np.allclose(np.linalg.norm(dirs, axis=-1), 1.0) and dirs[0, :, 1].min() > 0.9 and dirs[-1, :, 1].max() < -0.9
        assert np.allclose(dirs[Hp // 2, Wp // 2], (0.0, 0.0, -1.0), atol=0.15)
        want = r.trace_radiance(np.tile(np.float32(origin), (Wp * Hp, 1)), dirs.reshape(-1, 3), samples=2)
        assert pano.tobytes() == np.ascontiguousarray(want["rgb"]).tobytes()
        assert pano[:3].mean() > 0 and np.isinf(want["t"].reshape(Hp, Wp)[0]).all() and np.isfinite(want["t"].reshape(Hp, Wp)[-1]).all()
    finally:
        r.session.close()
