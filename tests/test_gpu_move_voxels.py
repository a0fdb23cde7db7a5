"""vrt_move_voxels ON THE DEVICE, byte for byte against the brute force of tests/move.py over every voxel of the grid, plus the record:
  - every case of tests/move.py at 128^3 on one shared context (the base grid uploaded afresh for each), with the selection staged from
    the host and read in place on the device;
  - a moved context == a fresh context on the brute force's final grid: the stored voxels, the ray walks over the pyramid and texels
    (vrt_trace_probe, every walk, culling off and on), vrt_cast_rays records and an accumulated frame, bit for bit; one frame also
    against the CPU oracle; one case at 256^3;
  - VRT_MOVE_DRY_RUN, and VRT_MOVE_IF_FREE with a blocked cell, leave every fetched byte, every walk and the next frame as they were;
  - ordering: a vrt_update_voxels queued before and one after the move on the context's stream, a vrt_cast_rays between each pair;
  - a context with frames in flight, with ReSTIR, on a row tile (tests/states.py) moves as a fresh one;
  - the error codes and empty cases of include/vrt_api.h, one by one;
  - Renderer.move_voxels / copy_voxels keep voxel_material / voxel_color equal to sync_voxels_from_device; examples/topple.py."""
import ctypes as C
import os
import runpy

import numpy as np
import pytest

import edit as E
import move as M
import orc
import radiance as X
import rays as R
import states as ST
import voxelize as V
from voxel_rt2_amd import _abi, _lib, host
from voxel_rt2_amd._session import NativeError, NativeSession

pytestmark = pytest.mark.gpu
ROOT = M.ROOT
W, H, DEPTH, SEED = 48, 32, 3, 7
MODES = [R.WALKS["record"], R.WALKS["branchy"] | R.BOX, R.WALKS["flat"] | R.BOX]   # (each walk once, the culling box off and on)


def config(gridname, G):
    p = M.params(gridname)
    return host.make_config(W, H, voxel_edges=p["voxel_edges"], exposure=p["exposure"], max_depth=DEPTH, seed=SEED, grid_res=G, sky_res=0)


def fresh(gridname, mat, rgb, cls=None):
    cfg = config(gridname, mat.shape[0])
    s = cls(cfg) if cls else NativeSession(_lib.load(), "vrt_", cfg)
    orc.setup(s, mat, rgb, M.params(gridname))
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


def rays_around(mat, boxes, seed):
    """tests/rays.py's families aimed at the boxes, from cell boundaries of a sample of the grid's solids, and axis-parallel ones"""
    G = mat.shape[0]
    aim = np.zeros_like(mat)
    for lo, hi in boxes:
        aim[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
    rng = np.random.default_rng([20261021, 5, seed])
    thin = np.zeros_like(mat)
    solid = np.argwhere(mat > 0)
    if len(solid):
        pick = solid[rng.integers(0, len(solid), 2000)]
        thin[pick[:, 0], pick[:, 1], pick[:, 2]] = 1
    return np.ascontiguousarray(np.concatenate([R.box_aimed(rng, G, aim, n=500), R.boundary_origins(rng, G, thin, n=200), R.axis_parallel(rng, G, n=100)]))


def cast_of(G, probe_rays):
    rays = np.zeros(len(probe_rays), _abi.RAY)
    rays["origin"], rays["dir"], rays["t_max"] = V.world(G, probe_rays[:, :3]), probe_rays[:, 3:], np.inf
    return rays


def whole_grid(s):
    g = int(s.cfg.grid_res)
    return s.fetch_voxels((0, 0, 0), (g, g, g))


def move(s, c, select=None, flags=None):
    return s.move_voxels(c["src"][0], c["src"][1], c["dst"][0], c["dst"][1], c["m"], c["t"], c["flags"] if flags is None else flags, select, c["value"])


def on_device(select, keep):
    import torch
    t = torch.from_numpy(np.array(select, np.int32)).cuda()
    torch.cuda.synchronize()                          # the tensor is written on torch's stream, read on the context's
    keep.append(t)
    return t


@pytest.fixture(scope="module")
def live():
    s = fresh("clutter", *M.grid("clutter"))
    yield s
    s.close()


@pytest.mark.parametrize("name", M.NAMES_128)
def test_device_equals_brute_force(live, name):
    c, (sel, _), want = M.case(name), M.select_of(name), M.expected(name)
    mat, rgb = M.grid(c["grid"])
    keep = []
    for path in ("host", "device") if sel is not None else ("host",):
        live.upload_voxels(mat, rgb)
        live.prepare()
        got = move(live, c, sel if path == "host" else on_device(sel, keep))
        M.check(*whole_grid(live), got, want, f"{name}, selection on the {path}")


def same_scene(e, f, rays, label):
    """context e == context f: stored voxels, every walk, cast records, a frame"""
    (m, c), (fm, fc) = whole_grid(e), whole_grid(f)
    assert m.tobytes() == fm.tobytes() and c.tobytes() == fc.tobytes(), label
    for mode in MODES:
        got, want = probe(e, mode, rays), probe(f, mode, rays)
        bad = np.flatnonzero((got.view(np.uint8).reshape(len(rays), -1) != want.view(np.uint8).reshape(len(rays), -1)).any(axis=1))
        assert got.tobytes() == want.tobytes(), f"{label}, mode {mode}: {bad.size} of {len(rays)} records differ: {R.describe(rays, got, want, bad)}"
    cast = cast_of(m.shape[0], rays)
    assert e.cast_rays(cast).tobytes() == f.cast_rays(cast).tobytes(), f"{label}: vrt_cast_rays records differ"
    e.reset()
    f.reset()
    a, b = frame(e), frame(f)
    assert a.tobytes() == b.tobytes(), f"{label}: {(a != b).sum()} of {a.size} frame values differ"
    return a


def check_deep(name, oracle=False):
    c, (sel, _), want = M.case(name), M.select_of(name), M.expected(name)
    mat, rgb = M.grid(c["grid"])
    e, f = fresh(c["grid"], mat, rgb), fresh(c["grid"], want[0], want[1])
    try:
        frame(e)                                      # frames before the move: the histories are the caller's to reset
        frame(f)                                      # (the frame counter goes on through a reset: as many launches on both)
        got = move(e, c, sel)
        M.check(*whole_grid(e), got, want, name)
        a = same_scene(e, f, rays_around(want[0], (c["src"], c["dst"]), len(name)), name)
        assert a.std() > 0
        if oracle:
            o = fresh(c["grid"], want[0], want[1], cls=lambda cfg: orc.Oracle(cfg, threads=4))
            try:
                frame(o)
                o.reset()
                b = frame(o)
                assert a.tobytes() == b.tobytes(), f"{name}: {(a != b).sum()} of {a.size} values differ from the oracle's"
            finally:
                o.close()
    finally:
        e.close()
        f.close()


@pytest.mark.parametrize("name", M.DEEP)
def test_moved_context_equals_fresh_context(name):
    check_deep(name, oracle=name == "turn30_y")


def test_moved_context_equals_fresh_context_256():
    assert M.expected(M.CASE_256)[2]["written"] > 10000 and M.expected(M.CASE_256)[2]["blocked"] > 0
    check_deep(M.CASE_256)


@pytest.mark.parametrize("name", ["flags05_blocked", "flags04_free", "flags09_blocked", "flags11_blocked"])
def test_dry_runs_and_blocked_moves_change_nothing(name):
    c, (sel, _), want = M.case(name), M.select_of(name), M.expected(name)
    mat, rgb = M.grid(c["grid"])
    assert want[0].tobytes() == mat.tobytes() and (c["flags"] & M.DRY or want[2]["blocked"] > 0)
    e, u = fresh(c["grid"], mat, rgb), fresh(c["grid"], mat, rgb)
    try:
        for s in (e, u):
            s.accumulate(4)
        keep = []
        assert move(e, c, sel) == want[2] and move(e, c, None if sel is None else on_device(sel, keep)) == want[2]
        a, b = frame(e), frame(u)                     # no reset: the accumulation goes on as if nothing had been asked
        assert a.tobytes() == b.tobytes(), f"{name}: {(a != b).sum()} of {a.size} frame values differ"
        same_scene(e, u, rays_around(mat, (c["src"], c["dst"]), 3), name)
    finally:
        e.close()
        u.close()


def test_edits_and_queries_queued_around_the_move_are_ordered():
    import torch
    c, (sel, _) = M.case("select_root_shift"), M.select_of("select_root_shift")
    mat0, rgb0 = M.grid("clutter")
    first, last = E._pattern((58, 10, 0), (66, 18, 6), seed=4, m=21), E._pattern((62, 12, 2), (72, 20, 9), seed=5, m=33)
    mat1, rgb1 = E.apply_numpy(mat0, rgb0, first)
    mat2, rgb2, rec = M.brute(mat1, rgb1, c, sel)
    mat3, rgb3 = E.apply_numpy(mat2, rgb2, last)
    assert rec["written"] > 20 and mat2.tobytes() != mat1.tobytes() and M.brute(mat0, rgb0, c, sel)[2] != rec
    rays = cast_of(128, rays_around(mat2, (c["src"], c["dst"]), 11))
    e = fresh("clutter", mat0, rgb0)
    fs = [fresh("clutter", m, col) for m, col in ((mat1, rgb1), (mat2, rgb2), (mat3, rgb3))]
    try:
        want = [f.cast_rays(rays) for f in fs]
        assert want[0].tobytes() != want[1].tobytes() != want[2].tobytes()
        keep = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (first[2], first[3], last[2], last[3])]
        t_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).cuda()
        outs = [torch.zeros(len(rays) * _abi.HIT.itemsize, dtype=torch.uint8, device="cuda") for _ in range(3)]
        t_sel = on_device(sel, keep)
        e.accumulate(4)
        fs[2].accumulate(4)                           # (as many launches on both: same_scene compares frames)
        e.update_voxels(first[0], first[1], keep[0].data_ptr(), keep[1].data_ptr(), on_device=True)      # queued, not waited for
        e.cast_rays(t_rays, outs[0])
        got = move(e, c, t_sel)
        e.cast_rays(t_rays, outs[1])
        e.update_voxels(last[0], last[1], keep[2].data_ptr(), keep[3].data_ptr(), on_device=True)
        e.cast_rays(t_rays, outs[2])
        e.sync()
        assert got == rec
        for k, what in enumerate(("before the move", "after the move", "after the last edit")):
            assert outs[k].cpu().numpy().tobytes() == want[k].tobytes(), what
        m, col = whole_grid(e)
        assert m.tobytes() == mat3.tobytes() and col.tobytes() == rgb3.tobytes()
        same_scene(e, fs[2], rays_around(mat3, (c["src"], c["dst"]), 12), "after edit, move, edit")
    finally:
        for s in [e] + fs:
            s.close()


BUSY = dict(grid="sunlit_d5", src=((20, 44, 44), (56, 68, 70)), dst=((10, 40, 40), (70, 90, 80)), flags=M.ERASE | M.KEEP, select=None, value=0)
BUSY["m"], BUSY["t"] = M.inverse_rounded(M.rot("y", 30.0), (38.0, 56.0, 57.0), (3, 4, -2))


@pytest.mark.parametrize("state", ["big_frame", "restir", "tile"])
def test_a_busy_context_moves_as_a_fresh_one(state):
    mat, rgb = X.scene("sunlit_d5")[:2]
    want = M.brute(mat, rgb, BUSY)
    assert want[2]["written"] > 100 and want[2]["erased"] > 100
    s = ST.open_session(X, "sunlit_d5", state)
    try:
        got = move(s, BUSY)
        if state in ST.AFTER:
            ST.AFTER[state](s)
        M.check(*whole_grid(s), got, want, state)
        assert move(s, BUSY, flags=BUSY["flags"] | M.DRY) == M.brute(want[0], want[1], BUSY, flags=BUSY["flags"] | M.DRY)[2]
    finally:
        s.close()


def test_error_codes_and_empty_cases():
    lib = _lib.load()
    mat, rgb = M.grid("clutter")
    ok = M.case("shift_near")
    res = np.full(1, 77, _abi.MOVE_RESULT)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(s, rec=True, select=None, dev=0, r=res, **kw):
        record = M.record_of(ok)
        for k, v in kw.items():
            record[0][k] = v
        return lib.vrt_move_voxels(C.c_void_p(s._ctx) if s is not None else None, p(record) if rec else None, p(select), dev, p(r))
    s = NativeSession(lib, "vrt_", config("clutter", 128))
    try:
        assert call(s) == _abi.VRT_E_STATE                                                 # before vrt_prepare
        orc.setup(s, mat, rgb, M.params("clutter"))
        s.upload_voxels(mat, rgb)
        assert call(s) == _abi.VRT_E_STATE                                                 # after an upload that no prepare has followed
        assert call(s, flags=16) == _abi.VRT_E_INVALID                                     # (arguments are checked before the state)
        with pytest.raises(NativeError):
            move(s, ok)
        s.prepare()
        assert call(None) == _abi.VRT_E_INVALID and call(s, rec=False) == _abi.VRT_E_INVALID
        for k in ("src", "dst"):
            for lo, hi in (((2, 1, 1), (1, 2, 2)), ((-1, 0, 0), (0, 1, 1)), ((127, 127, 127), (128, 128, 129))):
                assert call(s, **{k + "_lo": lo, k + "_hi": hi}) == _abi.VRT_E_INVALID, (k, lo, hi)
        B, T = _abi.MOVE_M_MAX, _abi.MOVE_T_MAX
        assert call(s, m=[B + 1] + [0] * 8) == _abi.VRT_E_INVALID and call(s, m=[0] * 8 + [-B - 1]) == _abi.VRT_E_INVALID
        assert call(s, t=[0, T + 1, 0]) == _abi.VRT_E_INVALID and call(s, t=[-T - 1, 0, 0]) == _abi.VRT_E_INVALID
        for flags in (16, 0x100, 0x80000000):
            assert call(s, flags=flags) == _abi.VRT_E_INVALID
        assert call(s, reserved=1) == _abi.VRT_E_INVALID
        assert call(s, dev=2) == _abi.VRT_E_INVALID and call(s, dev=-1) == _abi.VRT_E_INVALID
        m, c = whole_grid(s)
        assert m.tobytes() == mat.tobytes() and c.tobytes() == rgb.tobytes() and res[0]["written"] == 77        # refused calls touched nothing
        assert call(s, flags=M.DRY | M.ERASE, m=[B] * 9, t=[T, -T, T]) == _abi.VRT_OK and res[0]["written"] == 0 and res[0]["erased"] > 0   # the bounds themselves are valid
        assert call(s, flags=M.DRY, r=None) == _abi.VRT_OK                                  # result may be NULL
        res[:] = 77                                                                        # an empty source box: OK, nothing done, the record zeroed
        assert call(s, src_lo=(5, 5, 5), src_hi=(5, 9, 9)) == _abi.VRT_OK and res.tobytes() == bytes(48)
        m, c = whole_grid(s)
        assert m.tobytes() == mat.tobytes() and c.tobytes() == rgb.tobytes()
        want = M.expected("dst_empty")                                                     # an empty destination box still vacates
        assert move(s, M.case("dst_empty")) == want[2] and want[2]["erased"] > 0 and want[2]["written"] == 0
        M.check(*whole_grid(s), None, want, "empty destination box")
        with pytest.raises(ValueError):
            move(s, ok, select=np.zeros((2, 1, 1), np.int32))
        with pytest.raises(ValueError):
            s.move_voxels((0, 0, 0), (1, 1, 1), (0, 0, 0), (1, 1, 1), [0] * 8, [0] * 3)
    finally:
        s.close()


# ---- the facade -----------------------------------------------------------------------------------------------------------------------
def renderer():
    from voxel_rt2_amd.renderer import Renderer
    r = Renderer(dx=1 / 64, image_res=(64, 36), up=(0, 1, 0), voxel_edges=0.06, exposure=1.5, max_depth=2, seed=7, sky_res=0)
    r.set_directional_light((0.6, 1.0, 0.4), 0.1, (1.0, 0.95, 0.85))
    r.background_color[None] = (0.35, 0.5, 0.75)
    r.floor_height[None] = -0.3
    return r


def facade_case(r, src_lo, src_hi, kw):
    """the tests/move.py case of a Renderer.move_voxels call, through the facade's own move_transform and moved_box"""
    rot, pivot, shift = kw.get("rotation"), kw.get("pivot"), kw.get("shift", (0, 0, 0))
    m, t = r.move_transform(rot, pivot, shift)
    box = r.moved_box(src_lo, src_hi, rot, pivot, shift)
    flags = (0 if kw.get("copy") else M.ERASE) | (M.KEEP if kw.get("keep_solid") else 0) | (M.IF_FREE if kw.get("if_free") else 0) | (M.DRY if kw.get("dry_run") else 0)
    return dict(src=(tuple(src_lo), tuple(src_hi)), dst=(tuple(kw.get("dst_lo", box[0])), tuple(kw.get("dst_hi", box[1]))), m=m.reshape(-1).tolist(), t=t.tolist(),
                flags=flags, value=kw.get("select_value", 0))


def test_renderer_move_voxels_keeps_the_host_mirror_in_step():
    e = renderer()
    try:
        with pytest.raises(NativeError):
            e.move_voxels((0, 0, 0), (4, 4, 4))
        for x in range(-8, 9):
            for z in range(-8, 9):
                e.set_voxel((x, -3, z), 11, (0.8, 0.3, 0.2))
        for x in range(-3, 2):
            for y in range(-2, 6):
                for z in range(-2, 1):
                    e.set_voxel((x, y, z), 54 if y < 2 else 2, (0.2, 0.7, 0.9) if (x + y) % 2 else (0.9, 0.8, 0.1))
        e.prepare_data()
        e.set_voxel((1, 6, 0), 2, (1.0, 1.0, 1.0))                                          # not yet sent: goes first
        src = ((61, 62, 62), (66, 71, 65))
        calls = [dict(rotation=e.rotation_matrix("z", -90), pivot=(66, 62, 0)),             # the block tipped about its lower edge, onto the slab's level
                 dict(shift=(0, -1, 0), if_free=True),                                      # down into the slab: blocked, nothing happens
                 dict(shift=(0, -1, 0), keep_solid=True, copy=True),
                 dict(rotation=e.rotation_matrix("y", 30.0), pivot=(64.0, 0.0, 64.0), shift=(10, 20, 5), copy=True),
                 dict(shift=(3, 3, 3), dry_run=True)]
        boxes = [src, ((66, 62, 62), (75, 67, 65)), ((66, 62, 62), (75, 67, 65)), ((50, 60, 50), (80, 70, 80)), ((50, 60, 50), (80, 70, 80))]
        for (lo, hi), kw in zip(boxes, calls):
            e.accumulate(1)
            mat, rgb = e.voxel_material.copy(), e.voxel_color.copy()
            want = M.brute(mat, rgb, facade_case(e, lo, hi, kw))
            got = e.copy_voxels(lo, hi, **{k: v for k, v in kw.items() if k != "copy"}) if kw.get("copy") else e.move_voxels(lo, hi, **kw)
            assert got == want[2], (kw, got, want[2])
            changed = want[0].tobytes() != mat.tobytes()
            assert e.current_spp == (0 if changed else 1) or not changed
            M.check(*e.session.fetch_voxels((0, 0, 0), (128, 128, 128)), None, want, f"device after {kw}")
            M.check(e.voxel_material, e.voxel_color, None, want, f"host mirror after {kw}")
        assert got["written"] > 0 and e.voxel_material[66, 62, 62] > 0                       # the tipped block lies where the dry run looked
    finally:
        e.session.close()


def test_topple_example_runs(tmp_path, monkeypatch):
    import sys
    for k, v in (("VRT_RES", "160x90"), ("VRT_FRAMES", "1"), ("VRT_SPP", "1"), ("VRT_SKY_RES", "32"), ("VRT_MAX_DEPTH", "2"), ("VRT_OUT", str(tmp_path / "topple.png"))):
        monkeypatch.setenv(k, v)
    monkeypatch.syspath_prepend(ROOT)
    sys.modules.pop("scene", None)
    mod = runpy.run_path(os.path.join(ROOT, "examples", "topple.py"), run_name="topple")
    r, res = mod["main"]()
    try:
        assert (tmp_path / "topple_before.png").exists() and (tmp_path / "topple_after.png").exists()
        g = r.voxel_grid_res
        mat, rgb = res["cut_grid"]
        piece = int((res["labels"] == res["root"]).sum())
        assert piece > 500 and len(res["steps"]) == 3 and res["tipped"]
        for k, step in enumerate(res["steps"]):                                              # the numpy prediction: the same calls through the brute force
            c = facade_case(r, step["src_lo"], step["src_hi"], step["kw"])
            mat, rgb, rec = M.brute(mat, rgb, c, step["kw"].get("select"))
            assert step["res"] == rec and rec["written"] == rec["erased"] == piece and rec["blocked"] == 0, (k, step["res"], rec)
        m, c = r.session.fetch_voxels((0, 0, 0), (g, g, g))
        M.check(m, c, None, (mat, rgb, None), "the final grid")
        assert r.voxel_material.tobytes() == m.tobytes() and r.voxel_color.tobytes() == c.tobytes()
        lo, hi = res["lo"], res["hi"]
        assert hi[0] - lo[0] > hi[1] - lo[1] and int((m[tuple(slice(a, b) for a, b in zip(lo, hi))] > 0).sum()) == piece    # it lies on its side
        assert (m[lo[0]:hi[0], lo[1] - 1, lo[2]:hi[2]] > 0).any()                            # on something
    finally:
        r.session.close()
