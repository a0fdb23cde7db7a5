"""vrt_gather_irradiance ON THE DEVICE, bit for bit (tests/sensor.py holds the cases, the sensors, the expectation and the comparison;
every float is compared by its bits, any NaN equal to any NaN).  The expectation is tests/sensor.py's: the oracle's own sampling, shadow
ray, escape test and sky-only value, and -- for hemisphere rays that hit something -- vrt_trace_radiance on the device, which
tests/test_gpu_radiance.py pins to the oracle's render body.
  - every case == expectation, on the host path and on the device path, on the pyramid in global memory and on the staged one;
  - batches of 1, 63, 64, 65 and 257 sensors (a wave's reservation and its refill) x samples 1 and 3;
  - a call of more than one block and more than one chunk == the same sensors gathered in small calls;
  - one sensor x 4 096 samples == the ordered sums of 4 096 one-sample calls;
  - a gather queued before / after an edit sees the old / new grid; frames, histories and vrt_get_stats do not notice gathers, a
    pending deferred accumulation included;
  - error codes; Renderer.gather_irradiance with arrays and with tensors, default streams, bake_faces."""
import ctypes as C

import numpy as np
import pytest

import radiance as X
import sensor as S
from voxel_rt2_amd import _abi, _lib
from voxel_rt2_amd._session import NativeError, NativeSession

pytestmark = pytest.mark.gpu


def session(case, **kw):
    return S.start(NativeSession(_lib.load(), "vrt_", S.config(case, **kw)), case)


def device_gather(s, sensors, samples, first_frame=S.FIRST_FRAME, sync=True):
    """The device path: tensors on the device, the work queued on the context's stream, read back after a sync."""
    import torch
    t_in = torch.from_numpy(np.ascontiguousarray(sensors).view(np.uint8).reshape(-1)).cuda()
    t_out = torch.full((len(sensors) * _abi.IRRADIANCE.itemsize,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                          # the tensors are written on torch's stream, read on the context's
    s.gather_irradiance(t_in, samples, first_frame, t_out)
    if not sync:
        return t_in, t_out
    s.sync()
    return t_out.cpu().numpy().view(_abi.IRRADIANCE)


def device_query(s):
    return lambda rays, frame: s.trace_radiance(rays, 1, frame)["rgb"]


@pytest.mark.parametrize("case", list(S.CASES))
def test_device_equals_expectation(case):
    sensors = S.sensors_of(case)
    s = session(case)
    try:
        for n in S.SAMPLES:
            want = S.expected(case, n, device_query(s))
            host_ok = sensors["reserved"] == 0                                     # (the host path refuses a call with a reserved field set)
            S.check(s.gather_irradiance(sensors[host_ok], n, S.FIRST_FRAME), sensors[host_ok], want[host_ok], f"{case} samples {n} host path")
            S.check(device_gather(s, sensors, n), sensors, want, f"{case} samples {n} device path")
        n = max(S.SAMPLES)
        k = 1
        while not X.lib().radiance_emul_staged(k * len(sensors) * n, -1):          # plan_cast_staged's rule on the items of a launch
            k += 1
        many, want = np.tile(sensors, k), np.tile(S.expected(case, n, device_query(s)), k)
        assert len(S.chunks(len(many), n)) == 1
        S.check(device_gather(s, many, n), many, want, f"{case} x {k}, samples {n}, device path, staged")
    finally:
        s.close()


@pytest.mark.parametrize("n_sensors", [1, 63, 64, 65, 257])
def test_batch_sizes_around_a_waves_reservation(n_sensors):
    case = "sunlit_d5"
    sensors = S.sensors_of(case)
    pick = (np.arange(n_sensors) * 5) % len(sensors)
    s = session(case)
    try:
        for n in S.SAMPLES:
            want = S.expected(case, n, device_query(s))[pick]
            S.check(device_gather(s, sensors[pick], n), sensors[pick], want, f"{n_sensors} sensors, samples {n}")
    finally:
        s.close()


def test_a_normal_too_long_for_a_ray_is_a_zero_sample():
    """tests/test_sensor_host.py's argument, on the device: normals whose hemisphere direction comes out all zeros (or whose origin
    overflows) are valid sensors with all-zero records, on both paths, and the sensors around them are not disturbed."""
    case = "sunlit_d5"
    fmax = np.finfo(np.float32).max
    long_ = np.concatenate([S.make((0, 0, 0), (1e20, 3e38, 0.0)), S.make((0.1, -0.2, 0.3), (0.0, -2e19, 0.0)), S.make((fmax, 0.0, 0.0), (fmax, 0.0, 0.0))])
    good = S.families(case)["floor"][:70]
    mixed = np.concatenate([good[:1], long_, good[1:]])
    mixed["stream"] = np.arange(len(mixed)) * 3 + 1
    s = session(case)
    try:
        got = device_gather(s, mixed, 3)
        assert not S.as_floats(got[1:4]).view(np.uint32).any()
        assert got.tobytes() == s.gather_irradiance(mixed, 3, S.FIRST_FRAME).tobytes()
        rest = np.r_[0, 4:len(mixed)]
        assert got[rest].tobytes() == device_gather(s, mixed[rest], 3).tobytes() and (got["sky"][rest] > 0).any()
    finally:
        s.close()


def test_more_than_one_block_and_more_than_one_chunk():
    """The smallest call the plan cuts both ways: one sensor more than a block holds (2^18 + 1), two samples -- a block's two samples
    do not fit the plane together -- at depth 2, against the same sensors gathered in calls of one block's chunk or less."""
    case, spp = "sunlit_d2", 2
    n = S.lib().sensor_emul_rays(1 << 40) + 1
    assert len(S.blocks(n)) == 2 and len(S.chunks(S.blocks(n)[0][1], spp)) == 2
    assert len(S.blocks(n - 1)) == 1 and len(S.chunks(n, 1)) == 1                    # no smaller call does
    base = S.sensors_of(case)
    base = base[S.valid(base)]
    sensors = np.tile(base, n // len(base) + 1)[:n].copy()
    sensors["stream"] = np.arange(n, dtype=np.uint32)
    s = session(case)
    try:
        got = device_gather(s, sensors, spp)
        small = 1 << 16
        assert len(S.blocks(small)) == 1 and len(S.chunks(small, spp)) == 1
        parts = [device_gather(s, sensors[at:at + small], spp) for at in range(0, n, small)]
        assert got.tobytes() == np.concatenate(parts).tobytes()
        assert (got["sky"] > 0).any() and (got["sun"] > 0).any() and (got["sky_rgb"] > 0).any()
    finally:
        s.close()


def test_one_sensor_many_samples_is_the_ordered_sum_of_its_samples():
    import torch
    case, spp = "sunlit_d5", 4096
    sensor = S.families(case)["floor"][[3]].copy()
    s = session(case)
    try:
        whole = s.gather_irradiance(sensor, spp, 11)
        t_in = torch.from_numpy(sensor.view(np.uint8).reshape(-1)).cuda()
        t_out = torch.zeros((spp, 8), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for k in range(spp):                                                           # 4 096 one-sample calls, queued
            s.gather_irradiance(t_in, 1, 11 + k, t_out[k])
        s.sync()
        one = t_out.cpu().numpy()
        acc = np.zeros(8, np.float32)
        for k in range(spp):
            acc = acc + one[k]
        assert (acc / np.float32(spp)).astype(np.float32).tobytes() == whole.tobytes()
        assert len(np.unique(one[:, :3], axis=0)) > spp // 4 and 0 < whole["sky"][0] < 1 and set(np.unique(one[:, 3])) == {0.0, 1.0}
        assert device_gather(s, sensor, spp, 11).tobytes() == whole.tobytes()
    finally:
        s.close()


def test_a_gather_sees_the_grid_as_queued():
    """A roof over a sensor is opened between two queued gathers: `sky` is 0 before and not after."""
    import torch
    case = "sunlit_d2"
    s = session(case)
    try:
        lo, hi = (80, 70, 80), (125, 71, 125)                                          # above the fixtures' roof: a second, much wider slab
        n = (hi[0] - lo[0]) * (hi[2] - lo[2])
        solid = (torch.full((n,), 1, dtype=torch.int8, device="cuda"), torch.full((n * 3,), 128, dtype=torch.uint8, device="cuda"))
        gone = (torch.zeros(n, dtype=torch.int8, device="cuda"), torch.zeros(n * 3, dtype=torch.uint8, device="cuda"))
        sensor = S.make(S.world(128, (102.5, 69.875, 102.5)), (0.0, 1.0, 0.0))         # an eighth of a voxel under that slab's middle, facing up
        sensor["stream"] = 5
        t_in = torch.from_numpy(sensor.view(np.uint8).reshape(-1)).cuda()
        closed, opened = (torch.zeros(8, dtype=torch.float32, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        s.update_voxels(lo, hi, solid[0].data_ptr(), solid[1].data_ptr(), on_device=True)
        s.gather_irradiance(t_in, 16, 0, closed)           # queued, not waited for
        s.update_voxels(lo, hi, gone[0].data_ptr(), gone[1].data_ptr(), on_device=True)
        s.gather_irradiance(t_in, 16, 0, opened)
        s.sync()
        c, o = closed.cpu().numpy(), opened.cpu().numpy()
        assert c[3] == 0 and c[7] == 0 and o[3] > 0 and o[7] > 0, (c, o)
        assert s.gather_irradiance(sensor, 16, 0).view(np.float32).tobytes() == o.tobytes()
    finally:
        s.close()


def test_frames_and_stats_do_not_notice_gathers():
    """accumulate(4) x 3 with gathers in between, on the host path and on the device path: HDR, both histories and the stats as without
    them, with a deferred accumulation pending at every gather (tests/test_gpu_radiance.py's argument: the plan accumulates more than
    three launches of this size in one pass)."""
    import os
    import plan
    case = "sunlit_d5"
    defer_k = plan.shape(64 * 40 * 4, int(os.environ.get("GPU_MAX_HW_QUEUES", 4)))[1]
    assert defer_k > 3, f"launches of 64 x 40 x 4 items are accumulated {defer_k} at a time: no accumulation stays pending across the gathers"
    sensors = S.sensors_of(case)
    sensors = sensors[sensors["reserved"] == 0]
    keep = []

    def run(query):
        s = session(case, width=64, height=40)
        try:
            for k in range(3):
                s.accumulate(4)
                if query == "host":
                    s.gather_irradiance(sensors[:1 + 97 * k], 2, k)
                elif query == "device":
                    keep.append(device_gather(s, sensors, 3, k, sync=False))
            return ([s.fetch_hdr()] + [s.fetch_buffer(w) for w in (_abi.BUF_HISTORY_DIFFUSE, _abi.BUF_HISTORY_SPECULAR, _abi.BUF_GBUF_DEPTH, _abi.BUF_GBUF_NORMAL,
                                                                     _abi.BUF_GBUF_POSITION, _abi.BUF_GBUF_MAT)], s.stats())
        finally:
            s.close()
    plain, stats = run(None)
    assert plain[0].std() > 0
    assert stats["pipeline_flags"] & 1 and stats["render_launches"] == stats["temporal_launches"] == 3, stats
    for query in ("host", "device"):
        got, st = run(query)
        for a, b, what in zip(got, plain, ("hdr", "diffuse history", "specular history", "depth", "normal", "position", "material")):
            assert a.tobytes() == b.tobytes(), f"{query} gathers changed the {what}: {(a != b).sum()} of {a.size} values"
        for key in ("path_samples", "render_launches", "temporal_launches", "gris_launches", "rays", "dda_iters", "occupancy_queries", "closest_hits",
                    "sky_lookups", "pipeline_flags"):
            assert st[key] == stats[key], (query, key)


def test_error_codes():
    lib = _lib.load()
    case = "sunlit_d2"
    mat, rgb, params = S.scene(case)
    r, o = np.zeros(4, _abi.SENSOR), np.zeros(4, _abi.IRRADIANCE)
    r["normal"] = (0.0, 1.0, 0.0)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    call = lambda s, n=4, rr=r, spp=1, oo=o, dev=0: lib.vrt_gather_irradiance(C.c_void_p(s._ctx), n, p(rr), spp, 0, p(oo), dev)
    s = NativeSession(lib, "vrt_", S.config(case))
    try:
        assert call(s) == _abi.VRT_E_STATE                                             # before vrt_prepare
        S.start(s, case)
        s.upload_voxels(mat, rgb)
        assert call(s) == _abi.VRT_E_STATE                                             # after an upload that no prepare has followed
        with pytest.raises(NativeError):
            s.gather_irradiance(r)
        s.prepare()
        assert call(s) == _abi.VRT_OK
        assert call(s, rr=None) == call(s, oo=None) == call(s, n=-1) == call(s, dev=2) == call(s, dev=-1) == _abi.VRT_E_INVALID
        assert call(s, spp=0) == call(s, spp=-3) == call(s, spp=_abi.RADIANCE_MAX_SAMPLES + 1) == _abi.VRT_E_INVALID
        bad = r.copy()
        bad["reserved"][2] = 1
        before = o.copy()
        assert call(s, rr=bad) == _abi.VRT_E_INVALID and b"reserved" in lib.vrt_last_error() and o.tobytes() == before.tobytes()
        assert call(s, n=0) == _abi.VRT_OK and len(s.gather_irradiance(np.zeros(0, _abi.SENSOR))) == 0
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


def test_facade_arrays_tensors_default_streams_and_bake_faces():
    import torch
    r = renderer()
    try:
        with pytest.raises(NativeError):
            r.gather_irradiance((0.0, 0.5, 0.0), (0.0, 1.0, 0.0))                         # nothing prepared yet
        r.prepare_data()
        cell, face, centre, normal = r.surface_faces((40, 58, 40), (90, 66, 90))
        assert len(cell) > 1000 and set(np.unique(face)) == set(range(6))
        a = r.gather_irradiance(centre, normal, samples=3, first_frame=2)
        b = r.gather_irradiance(torch.from_numpy(centre).cuda(), torch.from_numpy(normal).cuda(), samples=3, first_frame=2)
        assert a.dtype == _abi.IRRADIANCE and a.tobytes() == b.tobytes()
        assert (a["sky"][face == 3] > 0).mean() > 0.5 and (a["sun"][face == 2] == 0).all() and (a["sun"][face == 3] > 0).any()
        st = np.arange(len(cell))[::-1].copy()
        c = r.gather_irradiance(centre[::-1], normal[::-1], samples=3, first_frame=2, streams=st)
        assert c[::-1].tobytes() == a.tobytes()                                           # a sensor's stream, not its place, keys its samples; the default is arange(n)
        assert r.gather_irradiance(centre[:1], normal[:1], samples=3, first_frame=2, streams=[0]).tobytes() == a[:1].tobytes()
        bc, bf, baked = r.bake_faces((40, 58, 40), (90, 66, 90), samples=3)
        assert (bc == cell).all() and (bf == face).all()
        assert baked.tobytes() == r.gather_irradiance(centre, normal, samples=3).tobytes()
        assert r.gather_irradiance(centre, normal).tobytes() == r.gather_irradiance(centre, normal, samples=64, first_frame=0).tobytes()
    finally:
        r.session.close()
