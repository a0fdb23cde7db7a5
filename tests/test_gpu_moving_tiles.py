"""The moving camera on contiguous row tiles (include/vrt_api.h: vrt_set_history_exchange, vrt_history_rows_io).

The "ranks" are contexts in one process on device 0; the all-gather of their temporal state goes through torch device tensors
(the collective itself is covered on CPU by tests/test_history_exchange_host.py).  The sequence is the reference's: a still
frame, then moving steps (set_camera_is_moving, render scale 0.5, then 1.0; scene.py:206-262) with a translation and a pitch, so
that the reprojected history taps cross the tile edges, then a still step after reset."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
from voxel_rt2_amd import _abi, _lib, camera, host, parallel, scenes
from voxel_rt2_amd._session import NativeSession

pytestmark = pytest.mark.gpu
W, H = 128, 80
ROW_BYTES = parallel.HISTORY_BYTES_PER_PIXEL * W
TILES3 = [(0, 23), (23, 61), (61, 80)]


@pytest.fixture(autouse=True, params=["pool", "fused"])
def render_schedule(request, monkeypatch):
    monkeypatch.setenv("VRT_RENDER", request.param)
    return request.param


def context(rows=None, restir=False, oracle=False, exchange=False):
    mat, rgb, params = scenes.scene_sunlit(0)
    cfg = host.make_config(W, H, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=4, seed=9,
                           use_restir=restir, rows=rows)
    s = orc.Oracle(cfg) if oracle else NativeSession(_lib.load(), "vrt_", cfg)
    orc.setup(s, mat, rgb, params)
    if exchange:
        parallel.enable_moving_camera(s)
    return s


def rc(s, name, *args):
    """Return code of an entry point (the session wrapper raises instead)."""
    return getattr(s._lib, "vrt_" + name)(C.c_void_p(s._ctx), *args)


def exchange(tiles, bounds, zero=False):
    """The all-gather of parallel.exchange_history between contexts of one process; zero: import zeros instead."""
    full = torch.zeros((len(tiles), max(b - a for a, b in bounds) * ROW_BYTES), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if not zero:
        for r, s in enumerate(tiles):
            s.history_rows_io(*bounds[r], full[r].data_ptr(), False)
            s.sync()
    for r, s in enumerate(tiles):
        for q, (lo, hi) in enumerate(bounds):
            if q != r:
                s.history_rows_io(lo, hi, full[q].data_ptr(), True)
        s.sync()


def moving_camera(k, scale):
    # translation and pitch, up and down in turn: the reprojected taps cross every tile edge with geometry on it, both ways
    pos = (0.4 + 0.06 * (k + 1), 0.5 + (-0.04, 0.03, -0.03, 0.04)[k], 2.0)
    view, proj = camera.default_matrices(W, H, pos=pos, look=(0.0, (0.12, -0.08, 0.10, -0.10)[k], 0.0))
    return host.make_camera(view, proj, pos, jitter_index=k + 1, moving=True, render_scale=scale, max_accum_frames=50.0)


def run_sequence(sessions, after_call=lambda: None, check=lambda step: None):
    """A still frame, four moving steps, a still step after reset; after_call runs behind every accumulate call, check(step)
    after every step."""
    steps = [0]

    def step(n):
        for s in sessions:
            s.accumulate(n)
        after_call()
        for s in sessions:
            s.end_frame()
        check(steps[0])
        steps[0] += 1

    step(2)
    for k in range(4):
        cam = moving_camera(k, 0.5 if k < 2 else 1.0)
        for s in sessions:
            s.set_camera(cam)
            if k == 0:
                s.reset()
        step(1)
    view, proj = camera.default_matrices(W, H, pos=(0.64, 0.34, 2.0), look=(0.0, 0.48, 0.0))
    for s in sessions:
        s.set_camera(host.make_camera(view, proj, (0.64, 0.34, 2.0), jitter_index=5))
        s.reset()
    step(1)


def assemble(tiles, bounds, which=None):
    out = None
    for s, (a, b) in zip(tiles, bounds):
        x = s.fetch_hdr() if which is None else s.fetch_buffer(which)
        out = np.zeros_like(x) if out is None else out
        out[a:b] = x[a:b]
    return out


def differing_rows(a, b):
    return sorted(set(np.argwhere((a.view(np.uint32) != b.view(np.uint32)).reshape(a.shape[0], -1).any(axis=1)).ravel().tolist()))


def check_tiles_equal_whole_and_oracle(bounds, restir):
    whole, ref = context(restir=restir), context(restir=restir, oracle=True)
    tiles = [context(rows=b, restir=restir, exchange=True) for b in bounds]

    def check(step):
        got, want = assemble(tiles, bounds), whole.fetch_hdr()
        assert np.isfinite(want).all() and want.max() > 0
        bad = differing_rows(got, want)
        assert not bad, f"step {step}: tiles differ from the whole frame on rows {bad[:16]}"
        assert np.array_equal(want.view(np.uint32), ref.fetch_hdr().view(np.uint32)), f"step {step}: whole frame differs from the oracle"
        for which in (_abi.BUF_HISTORY_DIFFUSE, _abi.BUF_HISTORY_SPECULAR):
            bad = differing_rows(assemble(tiles, bounds, which), whole.fetch_buffer(which))
            assert not bad, f"step {step}: buffer {which} differs on rows {bad[:16]}"

    run_sequence([whole, ref] + tiles, after_call=lambda: exchange(tiles, bounds), check=check)


def test_moving_tiles_equal_whole_frame_and_oracle():
    check_tiles_equal_whole_and_oracle(TILES3, restir=False)


def test_moving_restir_tiles_equal_whole_frame_and_oracle():
    check_tiles_equal_whole_and_oracle([(0, 37), (37, 80)], restir=True)


def test_moving_tiles_read_across_tiles():
    """The same sequence with zeros imported instead of the other tiles' rows: the frame differs in more than one tile, so the
    equality above depends on the rows that were exchanged."""
    whole = context()
    tiles = [context(rows=b, exchange=True) for b in TILES3]
    touched = set()

    def check(step):
        if 1 <= step <= 4:   # the moving steps (the still step after reset reads no history)
            bad = differing_rows(assemble(tiles, TILES3), whole.fetch_hdr())
            touched.update(t for t, (a, b) in enumerate(TILES3) if any(a <= r < b for r in bad))

    run_sequence([whole] + tiles, after_call=lambda: exchange(tiles, TILES3, zero=True), check=check)
    assert len(touched) >= 2, f"only tiles {sorted(touched)} differ"


def test_static_tiles_with_exchange_equal_tiles_without():
    off = [context(rows=b) for b in TILES3]
    on = [context(rows=b, exchange=True) for b in TILES3]
    targets = [torch.zeros((b - a, W, 3), dtype=torch.float32, device="cuda") for a, b in TILES3]
    torch.cuda.synchronize()
    for s, t in zip(on, targets):
        s.set_hdr_targets([t.data_ptr()])
    for n in (3, 1, 2):
        for s in off + on:
            s.accumulate(n)
            s.end_frame()
        exchange(on, TILES3)
    a, b = assemble(off, TILES3), assemble(on, TILES3)
    assert a.max() > 0 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for s, t, (lo, hi) in zip(on, targets, TILES3):
        s.sync()
        assert s.hdr_targets_written() == 3
        assert np.array_equal(t.cpu().numpy().view(np.uint32), a[lo:hi].view(np.uint32))


def test_guards():
    E_INVALID, E_STATE = _abi.VRT_E_INVALID, _abi.VRT_E_STATE
    lib = _lib.load()
    buf = torch.zeros(H * ROW_BYTES, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ptr = C.c_void_p(buf.data_ptr())
    moving = moving_camera(0, 0.5)

    # moving camera on a tile without the opt-in; the context goes on with the still camera
    t = context(rows=(23, 61))
    assert rc(t, "set_camera", C.byref(moving)) == E_INVALID
    t.accumulate(1)
    # opt-in after the first accumulate
    assert rc(t, "set_history_exchange", 1) == E_STATE
    t.accumulate(1)
    assert np.isfinite(t.fetch_hdr()).all()

    t = context(rows=(23, 61), exchange=True)
    t.accumulate(1)
    t.set_camera(moving)
    # a moving accumulate with other rows not imported since the last call, then with all of them
    assert rc(t, "history_rows_io", 0, 23, ptr, 1) == 0 and rc(t, "history_rows_io", 61, 79, ptr, 1) == 0
    assert rc(t, "accumulate", 1) == E_STATE and "79" in lib.vrt_last_error().decode()
    # more than one sample per moving call
    assert rc(t, "history_rows_io", 79, 80, ptr, 1) == 0
    assert rc(t, "accumulate", 2) == E_INVALID
    # ranges: export outside the own rows, import inside them, rows outside the image
    for args in ((0, 23, 0), (22, 30, 0), (23, 62, 0), (23, 61, 1), (10, 24, 1), (60, 70, 1), (-1, 5, 1), (61, 81, 1), (30, 30, 0), (5, 3, 1)):
        assert rc(t, "history_rows_io", args[0], args[1], ptr, args[2]) == E_INVALID, args
    t.accumulate(1)   # every other row was imported above
    assert np.isfinite(t.fetch_hdr()).all()

    # row stripes, either order
    w = context()
    w.set_row_stripes(16, 2, 0)
    assert rc(w, "set_history_exchange", 1) == E_INVALID
    w = context(exchange=True)
    assert rc(w, "set_row_stripes", 16, 2, 0) == E_INVALID

    # opt-in on a whole-frame context: accepted, output unchanged
    plain, opted = context(), context(exchange=True)

    def check(step):
        assert np.array_equal(plain.fetch_hdr().view(np.uint32), opted.fetch_hdr().view(np.uint32)), step

    run_sequence([plain, opted], check=check)
