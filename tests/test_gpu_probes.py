"""vrt_gather_probes ON THE DEVICE, bit for bit (tests/probe.py holds the cases, the probes, the expectation and the comparison; every
float is compared by its bits, any NaN equal to any NaN).  The expectation is tests/probe.py's: the oracle's own sampling, shadow ray,
escape test and sky-only value, and -- for rays that hit something -- vrt_trace_radiance on the device, which tests/test_gpu_radiance.py
pins to the oracle's render body; the basis, the products and the ordered sums in numpy float32.
  - every case == expectation, on the host path and on the device path, on the pyramid in global memory and on the staged one;
  - batches of 1, 63, 64, 65 and 257 probes (a wave's reservation and its refill) x samples 1 and 3;
  - a call of more than one block and more than one chunk == the same probes gathered in small calls;
  - one probe x 4 096 samples == the ordered float32 sums of 4 096 one-sample calls;
  - a gather queued before / after an edit sees the old / new grid; frames, histories and vrt_get_stats do not notice gathers, a
    pending deferred accumulation included;
  - error codes; Renderer.gather_probes with arrays and with tensors, default streams, probe_lattice into gather_probes."""
import ctypes as C

import numpy as np
import pytest

import probe as P
import radiance as X
from voxel_rt2_amd import _abi, _lib
from voxel_rt2_amd._session import NativeError, NativeSession

pytestmark = pytest.mark.gpu


def session(case, **kw):
    return P.start(NativeSession(_lib.load(), "vrt_", P.config(case, **kw)), case)


def device_gather(s, probes, samples, first_frame=P.FIRST_FRAME, sync=True):
    """The device path: tensors on the device, the work queued on the context's stream, read back after a sync."""
    import torch
    t_in = torch.from_numpy(np.array(probes).view(np.uint8).reshape(-1)).cuda()
    t_out = torch.full((len(probes) * _abi.SH_PROBE.itemsize,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                          # the tensors are written on torch's stream, read on the context's
    s.gather_probes(t_in, samples, first_frame, t_out)
    if not sync:
        return t_in, t_out
    s.sync()
    return t_out.cpu().numpy().view(_abi.SH_PROBE)


def device_query(s):
    return lambda rays, frame: s.trace_radiance(rays, 1, frame)["rgb"]


@pytest.mark.parametrize("case", list(P.CASES))
def test_device_equals_expectation(case):
    probes = P.probes_of(case)
    s = session(case)
    try:
        for n in P.SAMPLES:
            want = P.expected(case, n, device_query(s))
            P.check(s.gather_probes(probes, n, P.FIRST_FRAME), probes, want, f"{case} samples {n} host path")
            P.check(device_gather(s, probes, n), probes, want, f"{case} samples {n} device path")
        n = max(P.SAMPLES)
        k = 1
        while not X.lib().radiance_emul_staged(k * len(probes) * n, -1):            # plan_cast_staged's rule on the items of a launch
            k += 1
        many, want = np.tile(probes, k), np.tile(P.expected(case, n, device_query(s)), k)
        assert len(P.chunks(len(many), n)) == 1
        P.check(device_gather(s, many, n), many, want, f"{case} x {k}, samples {n}, device path, staged")
    finally:
        s.close()


@pytest.mark.parametrize("n_probes", [1, 63, 64, 65, 257])
def test_batch_sizes_around_a_waves_reservation(n_probes):
    case = "sunlit_d5"
    probes = P.probes_of(case)
    pick = (np.arange(n_probes) * 5) % len(probes)
    s = session(case)
    try:
        for n in P.SAMPLES:
            want = P.expected(case, n, device_query(s))[pick]
            P.check(device_gather(s, probes[pick], n), probes[pick], want, f"{n_probes} probes, samples {n}")
    finally:
        s.close()


def test_more_than_one_block_and_more_than_one_chunk():
    """The smallest call the plan cuts both ways: one probe more than a block holds (2^18 + 1), two samples -- a block's two samples
    do not fit the plane together -- at depth 2, against the same probes gathered in calls of 2^16."""
    case, spp = "sunlit_d2", 2
    n = (1 << 18) + 1
    assert n == P.lib().probe_emul_rays(1 << 40) + 1
    assert len(P.blocks(n)) == 2 and len(P.chunks(P.blocks(n)[0][1], spp)) == 2
    assert len(P.blocks(n - 1)) == 1 and len(P.chunks(n, 1)) == 1                    # no smaller call is cut both ways
    base = P.probes_of(case)
    base = base[P.valid(base)]
    probes = np.tile(base, n // len(base) + 1)[:n].copy()
    probes["stream"] = np.arange(n, dtype=np.uint32)
    s = session(case)
    try:
        got = device_gather(s, probes, spp)
        small = 1 << 16
        assert len(P.blocks(small)) == 1 and len(P.chunks(small, spp)) == 1
        parts = [device_gather(s, probes[at:at + small], spp) for at in range(0, n, small)]
        assert got.tobytes() == np.concatenate(parts).tobytes()
        assert (got["sky"] > 0).any() and (got["sun"] > 0).any() and (got["sh"][:, 0] > 0).any() and (got["sh"][:, 1:] != 0).any()
    finally:
        s.close()


def test_one_probe_many_samples_is_the_ordered_sum_of_its_samples():
    import torch
    case, spp = "sunlit_d5", 4096
    probe = P.families(case)["open_air"][[3]].copy()
    s = session(case)
    try:
        whole = s.gather_probes(probe, spp, 11)
        t_in = torch.from_numpy(probe.view(np.uint8).reshape(-1)).cuda()
        t_out = torch.zeros((spp, 32), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for k in range(spp):                                                           # 4 096 one-sample calls, queued
            s.gather_probes(t_in, 1, 11 + k, t_out[k])
        s.sync()
        one = t_out.cpu().numpy()
        acc = np.zeros(32, np.float32)
        for k in range(spp):
            acc = acc + one[k]
        assert (acc / np.float32(spp)).astype(np.float32).tobytes() == whole.tobytes()
        assert len(np.unique(one[:, :6], axis=0)) > spp // 4 and 0 < whole["sky"][0] < 1 and set(np.unique(one[:, 27])) == {0.0, 1.0}
        assert device_gather(s, probe, spp, 11).tobytes() == whole.tobytes()
    finally:
        s.close()


def test_a_gather_sees_the_grid_as_queued():
    """A closed shell around a probe is opened between two queued gathers: `sky` and `sun` are 0 before and not after."""
    import torch
    case = "sunlit_d2"
    s = session(case)
    try:
        lo, hi = (60, 100, 60), (67, 107, 67)                                          # open air, above everything the scene holds there
        shape = tuple(b - a for a, b in zip(lo, hi))
        shell = np.ones(shape, np.int8)
        shell[1:-1, 1:-1, 1:-1] = 0
        n = shell.size
        solid = (torch.from_numpy(shell.reshape(-1).copy()).cuda(), torch.full((n * 3,), 128, dtype=torch.uint8, device="cuda"))
        gone = (torch.zeros(n, dtype=torch.int8, device="cuda"), torch.zeros(n * 3, dtype=torch.uint8, device="cuda"))
        probe = P.make(P.world(128, (63.5, 103.5, 63.5)), 5)                           # the shell's middle
        t_in = torch.from_numpy(probe.view(np.uint8).reshape(-1)).cuda()
        closed, opened = (torch.zeros(32, dtype=torch.float32, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        s.update_voxels(lo, hi, solid[0].data_ptr(), solid[1].data_ptr(), on_device=True)
        s.gather_probes(t_in, 16, 0, closed)               # queued, not waited for
        s.update_voxels(lo, hi, gone[0].data_ptr(), gone[1].data_ptr(), on_device=True)
        s.gather_probes(t_in, 16, 0, opened)
        s.sync()
        c, o = closed.cpu().numpy(), opened.cpu().numpy()
        assert c[27] == 0 and c[31] == 0 and o[27] > 0 and o[31] > 0, (c, o)
        assert s.gather_probes(probe, 16, 0).view(np.float32).tobytes() == o.tobytes()
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
    probes = P.probes_of(case)
    keep = []

    def run(query):
        s = session(case, width=64, height=40)
        try:
            for k in range(3):
                s.accumulate(4)
                if query == "host":
                    s.gather_probes(probes[:1 + 97 * k], 2, k)
                elif query == "device":
                    keep.append(device_gather(s, probes, 3, k, sync=False))
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
    mat, rgb, params = P.scene(case)
    r, o = np.zeros(4, _abi.PROBE), np.zeros(4, _abi.SH_PROBE)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    call = lambda s, n=4, rr=r, spp=1, oo=o, dev=0: lib.vrt_gather_probes(C.c_void_p(s._ctx), n, p(rr), spp, 0, p(oo), dev)
    s = NativeSession(lib, "vrt_", P.config(case))
    try:
        assert call(s) == _abi.VRT_E_STATE                                             # before vrt_prepare
        P.start(s, case)
        s.upload_voxels(mat, rgb)
        assert call(s) == _abi.VRT_E_STATE                                             # after an upload that no prepare has followed
        with pytest.raises(NativeError):
            s.gather_probes(r)
        s.prepare()
        assert call(s) == _abi.VRT_OK
        assert call(s, rr=None) == call(s, oo=None) == call(s, n=-1) == call(s, dev=2) == call(s, dev=-1) == _abi.VRT_E_INVALID
        assert call(s, spp=0) == call(s, spp=-3) == call(s, spp=_abi.RADIANCE_MAX_SAMPLES + 1) == _abi.VRT_E_INVALID
        assert call(s, n=0) == _abi.VRT_OK and len(s.gather_probes(np.zeros(0, _abi.PROBE))) == 0
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


def test_facade_arrays_tensors_default_streams_and_probe_lattice():
    import torch
    r = renderer()
    try:
        with pytest.raises(NativeError):
            r.gather_probes((0.0, 0.5, 0.0))                                              # nothing prepared yet
        r.prepare_data()
        centre, cell = r.probe_lattice((40, 58, 40), (90, 74, 90), 4)
        assert len(centre) > 100 and (r.voxel_material[cell[:, 0], cell[:, 1], cell[:, 2]] <= 0).all()
        a = r.gather_probes(centre, samples=3, first_frame=2)
        b = r.gather_probes(torch.from_numpy(centre).cuda(), samples=3, first_frame=2)
        assert a.dtype == _abi.SH_PROBE and a.tobytes() == b.tobytes()
        high = cell[:, 1] >= 66                                                           # above the field of voxels (its top is y index 63)
        assert high.sum() > 50 and (a["sky"][high] > 0).mean() > 0.5 and (a["sun"][high] > 0).mean() > 0.9 and (a["sh"][high, 0] > 0).all()
        st = np.arange(len(cell))[::-1].copy()
        c = r.gather_probes(centre[::-1], samples=3, first_frame=2, streams=st)
        assert c[::-1].tobytes() == a.tobytes()                                           # a probe's stream, not its place, keys its samples; the default is arange(n)
        assert r.gather_probes(centre[:1], samples=3, first_frame=2, streams=[0]).tobytes() == a[:1].tobytes()
        assert r.gather_probes(centre).tobytes() == r.gather_probes(centre, samples=64, first_frame=0).tobytes()
        up = np.tile(np.float64((0, 1, 0)), (len(a), 1))
        e = r.sh_irradiance(r.gather_probes(centre), up)
        assert e.shape == (len(a), 3) and np.isfinite(e).all() and (e[high] > 0).mean() > 0.9
    finally:
        r.session.close()
