"""Deferred accumulation on the GPU: with a static camera the library queues ONE accumulation pass (k_temporal_group) for several
overlapped render launches, and everything that looks at the result forces the pending ones first.  Frames, histories and
g-buffer planes are compared bit for bit (as uint32) with the CPU oracle, which accumulates after every launch."""
import ctypes as C

import numpy as np
import pytest

import orc
from voxel_rt2_amd import _abi, _lib, camera, host, scenes
from voxel_rt2_amd._session import NativeSession

pytestmark = pytest.mark.gpu
W, H, DEPTH = 320, 180, 5
PLANES = (_abi.BUF_GBUF_DEPTH, _abi.BUF_GBUF_NORMAL, _abi.BUF_GBUF_MAT, _abi.BUF_HISTORY_DIFFUSE, _abi.BUF_HISTORY_SPECULAR)


def _scene():
    return scenes.scene_sunlit(0)


def _cfg(seed=3, rows=None, w=W, h=H):
    _, _, params = _scene()
    return host.make_config(w, h, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=DEPTH, seed=seed, rows=rows)


def _gpu(cfg, dev=False):
    mat, rgb, params = _scene()
    s = NativeSession(_lib.load_dev() if dev else _lib.load(), "vrt_", cfg)
    orc.setup(s, mat, rgb, params)
    return s


def _oracle(cfg):
    mat, rgb, params = _scene()
    o = orc.Oracle(cfg, threads=16)
    orc.setup(o, mat, rgb, params)
    return o


def _same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{what}: {(a.view(np.uint32) != b.view(np.uint32)).sum()} of {a.size} values differ"


def test_every_number_of_pending_launches_is_flushed_by_the_fetch():
    """1 ... 9 calls of four samples, a fresh context each: the fetch finds every residue of the group size pending."""
    cfg = _cfg()
    o = _oracle(cfg)
    for n in range(1, 10):
        o.accumulate(4)
        g = _gpu(cfg)
        for _ in range(n):
            g.accumulate(4)
        _same(g.fetch_hdr(), o.fetch_hdr(), f"{n} calls")
        st = g.stats()
        assert st["render_launches"] == n and st["temporal_launches"] == n and st["pipeline_flags"] & 1, st
        g.close()
    o.close()


def test_mixed_sample_counts_per_call():
    cfg = _cfg(seed=4)
    g, o = _gpu(cfg), _oracle(cfg)
    for n in (1, 4, 4, 2, 1, 1, 3, 4, 2, 2, 1):
        g.accumulate(n)
        o.accumulate(n)
    _same(g.fetch_hdr(), o.fetch_hdr(), "HDR")
    for which in PLANES:
        _same(g.fetch_buffer(which), o.fetch_buffer(which), f"buffer {which}")
    st = g.stats()
    assert st["temporal_launches"] == st["render_launches"] == 11, st
    g.close(); o.close()


def test_one_sample_calls_with_a_new_jitter_each():
    """Twenty one-sample calls, a new jitter (other matrices) before each and vrt_end_frame behind: the slices carry their own
    parameters, nothing is flushed between the calls."""
    cfg = _cfg(seed=11)
    g, o = _gpu(cfg), _oracle(cfg)
    for k in range(20):
        cam = host.default_camera(W, H, jitter_index=k + 1)
        for s in (g, o):
            s.set_camera(cam)
            s.accumulate(1)
            s.end_frame()
    _same(g.fetch_hdr(), o.fetch_hdr(), "HDR")
    for which in PLANES + (_abi.BUF_GBUF_REFL_DEPTH,):
        _same(g.fetch_buffer(which), o.fetch_buffer(which), f"buffer {which}")
    st = g.stats()
    assert st["temporal_launches"] == st["render_launches"] == 20, st
    g.close(); o.close()


def test_scene_and_accumulation_limit_changed_between_calls():
    """vrt_set_scene (another light) and another max_accum_frames (vrt_set_camera) between the calls of one group."""
    mat, rgb, params = _scene()
    cfg = _cfg(seed=6)
    g, o = _gpu(cfg), _oracle(cfg)
    view, proj = camera.default_matrices(W, H)
    for k, (limit, weight) in enumerate(((1e9, 1.0), (3.0, 1.0), (3.0, 0.5), (6.0, 0.5), (2.0, 2.0), (1e9, 1.0), (4.0, 1.0))):
        p = dict(params)
        p["light_weight"] = params.get("light_weight", 3.0) * weight
        for s in (g, o):
            s.set_scene(host.make_scene_params(**p))
            s.set_camera(host.make_camera(view, proj, camera.DEFAULT_POS, jitter_index=k, max_accum_frames=limit))
            s.accumulate(3 if k % 2 else 4)
    _same(g.fetch_hdr(), o.fetch_hdr(), "HDR")
    _same(g.fetch_buffer(_abi.BUF_HISTORY_DIFFUSE), o.fetch_buffer(_abi.BUF_HISTORY_DIFFUSE), "diffuse history")
    _same(g.fetch_buffer(_abi.BUF_HISTORY_SPECULAR), o.fetch_buffer(_abi.BUF_HISTORY_SPECULAR), "specular history")
    g.close(); o.close()


def test_static_then_moving_then_static_camera():
    """A moving-camera launch is not deferred: the pending static ones are accumulated before its pass resamples their histories."""
    cfg = _cfg(seed=7)
    g, o = _gpu(cfg), _oracle(cfg)
    pos = (0.46, 0.5, 2.0)
    view, proj = camera.default_matrices(W, H, pos=pos)
    for s in (g, o):
        for n in (4, 4, 2):      # three launches pending
            s.accumulate(n)
        s.end_frame()
        s.set_camera(host.make_camera(view, proj, pos, jitter_index=2, moving=True, render_scale=0.5, max_accum_frames=50.0))
        s.accumulate(1)
        s.end_frame()
        s.set_camera(host.make_camera(view, proj, pos, jitter_index=3, moving=True, max_accum_frames=50.0))
        s.accumulate(1)
        s.end_frame()
        s.set_camera(host.make_camera(view, proj, pos, jitter_index=4))
        for n in (4, 1, 4, 4, 4):
            s.accumulate(n)
    _same(g.fetch_hdr(), o.fetch_hdr(), "HDR")
    for which in PLANES:
        _same(g.fetch_buffer(which), o.fetch_buffer(which), f"buffer {which}")
    g.close(); o.close()


def test_reset_in_the_middle_of_a_group():
    cfg = _cfg(seed=8)
    g, o = _gpu(cfg), _oracle(cfg)
    for s in (g, o):
        for _ in range(6):       # a whole group and two pending launches
            s.accumulate(4)
        s.reset()
        for _ in range(3):
            s.accumulate(4)
    _same(g.fetch_hdr(), o.fetch_hdr(), "HDR")
    _same(g.fetch_buffer(_abi.BUF_HISTORY_DIFFUSE), o.fetch_buffer(_abi.BUF_HISTORY_DIFFUSE), "diffuse history")
    g.close(); o.close()


@pytest.mark.parametrize("every", [1, 3])
def test_frames_presented_asynchronously(every):
    """vrt_fetch_hdr_async every frame / every third frame while further frames are queued: each presented frame is the oracle's."""
    cfg = _cfg(seed=9)
    g, o = _gpu(cfg), _oracle(cfg)
    bufs = [g.host_alloc((H, W, 3)) for _ in range(2)]
    shown, want, slot_of = [], [], []
    for k in range(10):
        g.accumulate(4)
        o.accumulate(4)
        if k % every == every - 1:
            if len(slot_of) >= 2:     # the slot's fetch before last is collected first
                j = slot_of[-2]
                g.fetch_wait(j)
                shown.append(bufs[j].copy())
            j = len(slot_of) % 2
            g.fetch_hdr_async(bufs[j], slot=j)
            slot_of.append(j)
            want.append(o.fetch_hdr())
    for j in slot_of[-2:] if len(slot_of) >= 2 else slot_of:
        g.fetch_wait(j)
        shown.append(bufs[j].copy())
    assert len(shown) == len(want) >= 3
    for k, (a, b) in enumerate(zip(shown, want)):
        _same(a, b, f"presented frame {k}")
    _same(g.fetch_hdr(), o.fetch_hdr(), "the last frame")
    g.close(); o.close()


def test_row_shard():
    """A row tile defers like a whole frame: its own rows equal the oracle's."""
    rows = (64, 120)
    g, o = _gpu(_cfg(seed=10, rows=rows)), _oracle(_cfg(seed=10))
    for n in (4, 4, 3, 4, 4, 1, 4):
        g.accumulate(n)
        o.accumulate(n)
    _same(g.fetch_hdr()[rows[0]:rows[1]], o.fetch_hdr()[rows[0]:rows[1]], "own rows")
    for which in (_abi.BUF_HISTORY_DIFFUSE, _abi.BUF_HISTORY_SPECULAR, _abi.BUF_GBUF_REFL_DEPTH):
        _same(g.fetch_buffer(which)[rows[0]:rows[1]], o.fetch_buffer(which)[rows[0]:rows[1]], f"buffer {which}")
    g.close(); o.close()


def test_group_sizes_of_the_development_build(monkeypatch):
    """VRT_DEFER = 1 (a pass per launch), 2, 4 and 8: the same frames, the oracle's."""
    cfg = _cfg(seed=12)
    calls = (4, 4, 4, 1, 4, 2, 4, 4, 4, 4, 3)
    o = _oracle(cfg)
    for n in calls:
        o.accumulate(n)
    want, want_h = o.fetch_hdr(), o.fetch_buffer(_abi.BUF_HISTORY_SPECULAR)
    o.close()
    for k in ("1", "2", "4", "8"):
        monkeypatch.setenv("VRT_DEFER", k)     # (read when the context is created)
        g = _gpu(cfg, dev=True)
        for n in calls:
            g.accumulate(n)
        _same(g.fetch_hdr(), want, f"VRT_DEFER={k}")
        _same(g.fetch_buffer(_abi.BUF_HISTORY_SPECULAR), want_h, f"VRT_DEFER={k}: specular history")
        st = g.stats()
        assert st["temporal_launches"] == st["render_launches"] == len(calls), (k, st)
        g.close()


@pytest.mark.parametrize("fail_at", [1, 2, 5, 7])
def test_failed_launch_inside_a_group(monkeypatch, fail_at):
    """A launch that fails to queue (VRT_TEST_FAIL_LAUNCH) with launches pending: those are accumulated all the same, the failed
    one leaves nothing behind -- the result of a context that never saw the failure."""
    lib = _lib.load_dev()
    cfg = _cfg(seed=13)
    monkeypatch.setenv("VRT_DEFER", "4")
    good = _gpu(cfg, dev=True)
    for _ in range(9):
        good.accumulate(4)
    want = good.fetch_hdr()
    good.close()
    monkeypatch.setenv("VRT_TEST_FAIL_LAUNCH", str(fail_at))
    s = _gpu(cfg, dev=True)
    monkeypatch.delenv("VRT_TEST_FAIL_LAUNCH")
    done = 0
    for _ in range(fail_at):
        s.accumulate(4)
        done += 1
    assert lib.vrt_accumulate(C.c_void_p(s._ctx), 4) == -2 and b"injected" in lib.vrt_last_error()
    while done < 9:
        s.accumulate(4)
        done += 1
    st = s.stats()
    assert st["temporal_launches"] == 9, st
    _same(s.fetch_hdr(), want, "after the failure")
    s.close()
