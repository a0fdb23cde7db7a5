"""vrt_denoise ON THE DEVICE, bit for bit (tests/denoise.py holds the expectation -- include/vrt_api.h's text in numpy float32 -- and the
comparison: every float by its bits, any NaN equal to any NaN).
  - six contexts -- s1, sunlit, sunlit behind a moving camera, sunlit with ReSTIR, dense, and the smallest frame vrt_create accepts --
    after 1 and after 3 vrt_accumulate calls: the five buffers and the HDR frame are fetched, and numpy's expectation on them equals
    vrt_denoise on the host path and on the device path, for the default parameters and two other sets;
  - purity: HDR, both histories, the g-buffers and vrt_get_stats after accumulate, denoise, accumulate equal those after accumulate,
    fetch_hdr, accumulate -- with a deferred accumulation pending at the call, and on a context that defers nothing;
  - ordering: a denoise queued on the device path, then more vrt_accumulate calls at once and one sync at the end: the result is the
    expectation on the buffers fetched BEFORE the call -- after three calls, and after more calls than the pipeline has copies;
  - every error code; NativeSession.denoise with `out`; Renderer.fetch_denoised in both forms."""
import ctypes as C
import os

import numpy as np
import pytest

import cast as K
import denoise as D
import orc
import plan
import states as T
from voxel_rt2_amd import _abi, _lib, host
from voxel_rt2_amd._session import NativeError, NativeSession

pytestmark = pytest.mark.gpu

# name: (scene, width, height, max_depth, config keywords, samples a call, moving)
CASES = {
    "s1": ("s1", 64, 40, 4, {}, 2, False),
    "sunlit": ("sunlit", 80, 48, 5, {}, 2, False),
    "sunlit_moving": ("sunlit", 72, 44, 4, {}, 1, True),
    "sunlit_restir": ("sunlit", 64, 40, 4, dict(use_restir=True), 2, False),
    "dense": ("dense", 48, 40, 4, {}, 2, False),
    "smallest": ("sunlit", 1, 1, 4, {}, 2, False),       # no multiple of any tile: the smallest frame vrt_create accepts
}
# the other contexts the tests below open
CONTEXTS = dict(CASES)
CONTEXTS.update({
    "sunlit_pending": ("sunlit", 64, 40, 5, {}, 4, False),           # 64 x 40 x 4 items a launch: accumulated more than one at a time
    "errors": ("sunlit", 64, 48, 2, {}, 1, False),
    "errors_tile": ("sunlit", 64, 48, 2, dict(rows=(8, 24)), 1, False),
})
PARAMS = (None, (6, 0.5, 0.0, 0.0), (2, 0.25, 0.5, 8.0))
MOVES = ("street", "courtyard", "under_eaves", "default", "street")
BUFFERS = dict(pos=_abi.BUF_GBUF_POSITION, normal=_abi.BUF_GBUF_NORMAL, mat=_abi.BUF_GBUF_MAT, hist_d=_abi.BUF_HISTORY_DIFFUSE, hist_s=_abi.BUF_HISTORY_SPECULAR)
STAT_KEYS = ("path_samples", "render_launches", "temporal_launches", "gris_launches", "rays", "dda_iters", "occupancy_queries", "closest_hits", "sky_lookups",
             "pipeline_flags")


def session(case):
    name, w, h, depth, kw, _, _ = CONTEXTS[case]
    mat, rgb, params = K.scene(name)
    cfg = host.make_config(w, h, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=depth, seed=23, grid_res=mat.shape[0], **kw)
    s = NativeSession(_lib.load(), "vrt_", cfg)
    orc.setup(s, mat, rgb, params, cam=T.camera("default", w, h, 0))
    return s


def step(s, case, k):
    """The case's k-th vrt_accumulate call; a moving camera goes to another pose first and ends its frame behind it."""
    _, w, h, _, _, spp, moving = CONTEXTS[case]
    if moving:
        s.set_camera(T.camera(MOVES[k % len(MOVES)], w, h, k + 1, moving=True, max_accum_frames=50.0))
    s.accumulate(spp)
    if moving:
        s.end_frame()


def fetch_planes(s):
    planes = {k: s.fetch_buffer(which) for k, which in BUFFERS.items()}
    planes["hdr"] = s.fetch_hdr()
    return planes


def abi_params(params):
    return None if params is None else _abi.VrtDenoiseParams(*params)


def device_denoise(s, params, sync=True):
    """The device path: a tensor on the device, the work queued on the context's stream, read back after a sync."""
    import torch
    t = torch.full((s.H, s.W, 3), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()                          # the tensor is written on torch's stream, and again on the context's
    s.denoise(abi_params(params), t)
    if not sync:
        return t
    s.sync()
    return t.cpu().numpy()


def check_now(s, moving, label):
    planes = fetch_planes(s)
    for params in PARAMS:
        want = D.expected(planes, params or D.DEFAULTS, moving, s.cfg.dx)
        D.check(s.denoise(abi_params(params)), want, f"{label} {params} host path")
        D.check(device_denoise(s, params), want, f"{label} {params} device path")
    return planes, want


@pytest.mark.parametrize("case", list(CASES))
def test_device_equals_expectation(case):
    moving = CASES[case][6]
    s = session(case)
    try:
        k = 0
        if moving:                                    # two steps first: the history is a resampled one from then on
            for k in range(2):
                step(s, case, k)
            k = 2
        step(s, case, k)
        planes, want = check_now(s, moving, f"{case} after 1 call")
        if case != "smallest":
            surface = ~(planes["pos"] == 0).all(axis=-1)
            assert surface.sum() > surface.size // 4 and (want[surface] != planes["hdr"][surface]).any(), "nothing was filtered"
        step(s, case, k + 1)
        step(s, case, k + 2)
        check_now(s, moving, f"{case} after 3 calls")
    finally:
        s.close()


def observed(s):
    return [s.fetch_hdr()] + [s.fetch_buffer(w) for w in (_abi.BUF_HISTORY_DIFFUSE, _abi.BUF_HISTORY_SPECULAR, _abi.BUF_GBUF_DEPTH, _abi.BUF_GBUF_NORMAL,
                                                           _abi.BUF_GBUF_POSITION, _abi.BUF_GBUF_MAT)], s.stats()


@pytest.mark.parametrize("case", ["sunlit_pending", "sunlit_restir"])
def test_frames_and_stats_do_not_notice_a_denoise(case):
    """accumulate, denoise, accumulate == accumulate, fetch_hdr, accumulate.  `sunlit_pending`: 64 x 40 x 4 items a launch, which the plan
    accumulates more than one at a time -- the first call's accumulation is pending when the denoise (or the fetch) forces it."""
    keep = []
    if case == "sunlit_pending":
        assert plan.shape(64 * 40 * 4, int(os.environ.get("GPU_MAX_HW_QUEUES", 4)))[1] > 1, "launches of 64 x 40 x 4 items are not deferred: nothing is pending"

    def run(between):
        s = session(case)
        try:
            step(s, case, 0)
            if between == "host":
                s.denoise()
            elif between == "device":
                keep.append(device_denoise(s, None, sync=False))
            else:
                s.fetch_hdr()
            step(s, case, 1)
            return observed(s)
        finally:
            s.close()
    plain, stats = run(None)
    assert plain[0].std() > 0
    for between in ("host", "device"):
        got, st = run(between)
        for a, b, what in zip(got, plain, ("hdr", "diffuse history", "specular history", "depth", "normal", "position", "material")):
            assert a.tobytes() == b.tobytes(), f"a denoise on the {between} path changed the {what}: {(a != b).sum()} of {a.size} values"
        for key in STAT_KEYS:
            assert st[key] == stats[key], (between, key)


@pytest.mark.parametrize("calls", [3, 2 * 12 + 2])
def test_launches_queued_behind_a_denoise_do_not_overtake_it(calls):
    """The buffers are fetched, a denoise is queued on the device path, `calls` vrt_accumulate calls follow at once and one sync ends it:
    the result is the expectation on the buffers fetched before the call.  3 calls; and 26, more than twice the copies the pipeline can
    have of what a launch writes (VRT_MAX_SETS = 12, thirteen rotating normal planes): every plane the denoise read has been written
    again by then."""
    case = "sunlit"
    s = session(case)
    try:
        step(s, case, 0)
        planes = fetch_planes(s)
        want = D.expected(planes, D.DEFAULTS, False, s.cfg.dx)
        t = device_denoise(s, None, sync=False)
        for k in range(calls):
            step(s, case, 1 + k)
        s.sync()
        D.check(t.cpu().numpy(), want, f"{calls} calls behind the denoise")
        assert not D.same_f32(s.fetch_hdr(), planes["hdr"]).all()                        # the frame has moved on
    finally:
        s.close()


def test_error_codes():
    lib = _lib.load()
    _abi.declare(lib, "vrt_")
    out = np.zeros((48, 64, 3), np.float32)
    po = out.ctypes.data_as(C.c_void_p)

    def call(s, params=None, o=po, dev=0):
        return lib.vrt_denoise(C.c_void_p(s._ctx) if s is not None else None, None if params is None else C.byref(_abi.VrtDenoiseParams(*params)), o, dev)
    s = session("errors")
    try:
        assert call(None) == _abi.VRT_E_INVALID
        assert call(s) == _abi.VRT_E_STATE                                           # nothing accumulated since vrt_create
        assert call(s, o=None) == call(s, dev=2) == call(s, dev=-1) == _abi.VRT_E_INVALID       # arguments are looked at first
        for bad in ((0, 0.25, 0.5, 64.0), (7, 0.25, 0.5, 64.0), (-1, 0.25, 0.5, 64.0), (5, -0.1, 0.5, 64.0), (5, 0.25, -1.0, 64.0), (5, 0.25, 0.5, -2.0),
                    (5, np.nan, 0.5, 64.0), (5, 0.25, np.inf, 64.0), (5, 0.25, 0.5, np.nan), (5, np.inf, 0.5, 64.0), (5, 0.25, 0.5, -np.inf)):
            assert call(s, bad) == _abi.VRT_E_INVALID, bad
        with pytest.raises(NativeError):
            s.denoise()
        step(s, "errors", 0)
        assert call(s) == _abi.VRT_OK
        for good in ((1, 0.0, 0.0, 0.0), (6, 3.0, 2.0, 1e6)):
            assert call(s, good) == _abi.VRT_OK, good
        for bad in ((0, 0.25, 0.5, 64.0), (5, 0.25, 0.5, np.nan)):
            assert call(s, bad) == _abi.VRT_E_INVALID, bad
        s.reset()
        assert call(s) == _abi.VRT_E_STATE                                           # nothing accumulated since vrt_reset
        step(s, "errors", 1)
        assert call(s) == _abi.VRT_OK
        s.set_camera(T.camera("default", 64, 48, 3, render_scale=0.5))
        assert call(s) == _abi.VRT_OK                                                # what counts is the camera the frame was rendered with
        s.accumulate(1)
        assert call(s) == _abi.VRT_E_STATE                                           # ... a render scale other than 1
        s.set_camera(T.camera("default", 64, 48, 4))
        assert call(s) == _abi.VRT_E_STATE
        s.accumulate(1)
        assert call(s) == _abi.VRT_OK
    finally:
        s.close()
    s = session("errors_tile")                                                       # a row tile
    try:
        s.accumulate(1)
        assert call(s) == _abi.VRT_E_STATE
    finally:
        s.close()
    s = session("errors")                                                            # row stripes
    try:
        s.set_row_stripes(8, 2, 1)
        s.accumulate(1)
        assert call(s) == _abi.VRT_E_STATE
    finally:
        s.close()
    s = session("errors")                                                            # the history exchange, which a whole frame may opt into
    try:
        s.set_history_exchange(True)
        s.accumulate(1)
        assert call(s) == _abi.VRT_E_STATE
    finally:
        s.close()


def test_session_out_argument():
    import torch
    s = session("s1")
    try:
        step(s, "s1", 0)
        mine = np.zeros((s.H, s.W, 3), np.float32)
        assert s.denoise(out=mine) is mine and mine.tobytes() == s.denoise().tobytes()
        with pytest.raises(ValueError):
            s.denoise(out=np.zeros((s.H, s.W, 4), np.float32))
        with pytest.raises(ValueError):
            s.denoise(out=torch.zeros(7, dtype=torch.float32, device="cuda"))
    finally:
        s.close()


def test_facade_fetch_denoised_in_both_forms():
    from test_gpu_probes import renderer
    r = renderer(48, 32)
    try:
        r.prepare_data()
        r.accumulate(2)
        s = r.session
        planes = fetch_planes(s)
        hdr = r.fetch_denoised()
        D.check(hdr, D.expected(planes, D.DEFAULTS, False, s.cfg.dx), "fetch_denoised()")
        other = r.fetch_denoised(iterations=3, plane_tolerance=0.5, sigma_l=0.0, full_at=8.0)
        D.check(other, D.expected(planes, (3, 0.5, 0.0, 8.0), False, s.cfg.dx), "fetch_denoised(3, 0.5, 0, 8)")
        ldr = r.fetch_denoised(ldr=True)
        assert ldr.shape == (32, 48, 4) and ldr.dtype == np.float32 and ldr.tobytes() == r.tone_map(hdr).tobytes()
        assert (ldr[..., :3] >= 0).all() and (ldr[..., :3] <= 1).all() and (ldr[..., 3] == 1).all()
    finally:
        r.session.close()
