"""vrt_distance_field ON THE DEVICE, byte for byte against the numpy brute forces of tests/distance.py, over every cell of every box:
  - every case family at 128^3 on the host path and on the device path (torch tensors), with and without `nearest`; three at 256^3;
  - the whole grid with max_d2 = 16 on a sparse and on a half-full scene; the whole grid unbounded on the sparse one;
  - field, edit, field queued on the device path without a wait in between: the first sees the old grid, the second the new one;
  - frames accumulated with calls interleaved == frames without, vrt_get_stats unchanged; a context with frames in flight, with ReSTIR,
    on a row tile answers as a fresh one (tests/states.py);
  - the error codes and empty cases of include/vrt_api.h, one by one;
  - the facade: signed, grow_voxels and shrink_voxels against numpy-predicted grids on a fresh context, grow then shrink, the example."""
import ctypes as C
import functools
import os
import runpy

import numpy as np
import pytest

import distance as D
import orc
import radiance as X
import states as ST
from voxel_rt2_amd import _abi, _lib, host
from voxel_rt2_amd._session import NativeError, NativeSession

pytestmark = pytest.mark.gpu
ROOT = D.ROOT


def session(name, width=16, height=8, **kw):
    """a prepared context on a named grid of tests/distance.py"""
    mat, params = D.grid(name), D.params(name)
    cfg = host.make_config(width, height, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=2, grid_res=mat.shape[0], **kw)
    s = NativeSession(_lib.load(), "vrt_", cfg)
    orc.setup(s, mat, D.colours(name), params)
    return s


@pytest.fixture(scope="module")
def live():
    """live(grid): one prepared context per grid, shared by the tests that only ask it questions."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = session(name)
        return made[name]
    yield get
    for s in made.values():
        s.close()


def device_field(s, lo, hi, max_d2, to_empty=False, nearest=True, sync=True):
    """The device path: tensors on the device, the work queued on the context's stream, read back after a sync."""
    import torch
    shape = tuple(h - l for l, h in zip(lo, hi))
    out = tuple(torch.full(shape, 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in range(2 if nearest else 1))
    torch.cuda.synchronize()                          # the tensors are written on torch's stream, then on the context's
    s.distance_field(lo, hi, max_d2, to_empty=to_empty, nearest=nearest, out=out if nearest else out[0])
    if not sync:
        return out
    s.sync()
    return tuple(t.cpu().numpy() for t in out)


def both_paths(s, name):
    c = D.CASES[name]
    want = D.expected(name)
    args = (c["lo"], c["hi"], c["max_d2"])
    d2, near = s.distance_field(*args, to_empty=c["to_empty"], nearest=True)
    D.check(d2, near, want, name + " host path")
    D.check(*device_field(s, *args, c["to_empty"]), want, name + " device path")
    only = s.distance_field(*args, to_empty=c["to_empty"])
    assert only.tobytes() == want[0].tobytes(), name + ": d2 without nearest, host path"
    assert device_field(s, *args, c["to_empty"], nearest=False)[0].tobytes() == want[0].tobytes(), name + ": d2 without nearest, device path"


@pytest.mark.parametrize("name", D.NAMES_128)
def test_device_equals_brute_force(live, name):
    both_paths(live(D.CASES[name]["grid"]), name)


@pytest.mark.parametrize("name", D.GPU_256)
def test_device_equals_brute_force_256(live, name):
    both_paths(live(D.CASES[name]["grid"]), name)


@pytest.mark.parametrize("name,to_empty", [("s1", False), ("dense", False), ("dense", True)])
def test_whole_grid_bounded(live, name, to_empty):
    """every cell of the 128^3 grid, max_d2 = 16, against brute_offsets"""
    lo, hi = (0, 0, 0), (128, 128, 128)
    want = D.brute_offsets(D.grid(name), lo, hi, 16, to_empty)
    D.check(*device_field(live(name), lo, hi, 16, to_empty), want, f"{name} whole grid to_empty={to_empty}")


def test_whole_grid_unbounded_on_a_sub_lattice(live):
    """One unbounded call over the whole sparse grid: the grown box is the grid and lines are as long and targets as far as they get.
    The device computes every cell; the brute force over 3337 targets is affordable for every fifth cell per axis only, so THIS test --
    and no other -- compares on the sub-lattice [::5, ::5, ::5] (17576 cells, faces and far corners included)."""
    lo, hi = (0, 0, 0), (128, 128, 128)
    d2, near = device_field(live("s1"), lo, hi, _abi.DIST_MAX_D2)
    want = D.brute_targets(D.grid("s1"), lo, hi, _abi.DIST_MAX_D2, stride=5)
    assert (d2 != D.FAR).all() and (near >= 0).all()
    D.check(np.ascontiguousarray(d2[::5, ::5, ::5]), np.ascontiguousarray(near[::5, ::5, ::5]), want, "s1 whole grid unbounded")
    assert d2.max() > 64 * 64                                                              # (far targets: the cells across the grid)


def test_a_field_sees_the_grid_as_queued():
    import torch
    c = D.CASES["s1_edit"]
    lo, hi, bm, bc = D.S1_EDIT
    s = session("s1")
    try:
        keep = (torch.from_numpy(np.ascontiguousarray(bm)).cuda(), torch.from_numpy(np.ascontiguousarray(bc)).cuda())
        torch.cuda.synchronize()
        before = device_field(s, c["lo"], c["hi"], c["max_d2"], sync=False)                  # queued, not waited for
        s.update_voxels(lo, hi, keep[0].data_ptr(), keep[1].data_ptr(), on_device=True)
        after = device_field(s, c["lo"], c["hi"], c["max_d2"], sync=False)
        s.sync()
        old = D.reference(D.grid("s1"), c["lo"], c["hi"], c["max_d2"])
        D.check(before[0].cpu().numpy(), before[1].cpu().numpy(), old, "before the edit")
        D.check(after[0].cpu().numpy(), after[1].cpu().numpy(), D.expected("s1_edit"), "after the edit")
        assert old[0].tobytes() != D.expected("s1_edit")[0].tobytes()
    finally:
        s.close()


def test_frames_do_not_notice_fields():
    """accumulate(4) x 3 with fields in between, on the host path and on the device path: HDR, both histories and the statistics as
    without them; and vrt_get_stats is the same before and after a call."""
    import torch
    lo, hi = (30, 50, 40), (70, 70, 80)
    shape = tuple(h - l for l, h in zip(lo, hi))
    t_out = tuple(torch.zeros(shape, dtype=torch.int32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()

    def run(query):
        s = session("sunlit", width=64, height=40)
        try:
            for k in range(3):
                s.accumulate(4)
                if query == "host":
                    s.distance_field(lo, hi, 100 * (k + 1), nearest=k != 1, to_empty=k == 2)
                elif query == "device":
                    s.distance_field(lo, hi, 100 * (k + 1), nearest=True, to_empty=k == 2, out=t_out)
            frames = [s.fetch_hdr()] + [s.fetch_buffer(w) for w in (_abi.BUF_HISTORY_DIFFUSE, _abi.BUF_HISTORY_SPECULAR)]
            st = s.stats()
            s.distance_field(lo, hi, 50, nearest=True)
            assert s.stats() == st
            return frames, st
        finally:
            s.close()
    plain, stats = run(None)
    assert plain[0].std() > 0
    for query in ("host", "device"):
        got, st = run(query)
        for a, b, what in zip(got, plain, ("hdr", "diffuse history", "specular history")):
            assert a.tobytes() == b.tobytes(), f"{query} fields changed the {what}: {(a != b).sum()} of {a.size} values"
        for key in ("path_samples", "render_launches", "temporal_launches", "rays"):
            assert st[key] == stats[key], (query, key)


BUSY = ((20, 44, 44), (56, 68, 70), 144)


@functools.lru_cache(maxsize=None)
def busy_reference():
    return D.reference(X.scene("sunlit_d5")[0], *BUSY)


@pytest.mark.parametrize("state", ["big_frame", "restir", "tile"])
def test_a_busy_context_answers_as_a_fresh_one(state):
    """frames in flight with their pass pending / ReSTIR on / a row tile (tests/states.py): the same bytes as the brute force, which is
    what a fresh context gives (test_device_equals_brute_force)"""
    case, (lo, hi, max_d2) = "sunlit_d5", BUSY
    want = busy_reference()
    assert (want[0] != D.FAR).any() and (want[0] == D.FAR).any()
    s = ST.open_session(X, case, state)
    try:
        d2, near = s.distance_field(lo, hi, max_d2, nearest=True)                              # the host path does not force the pending pass
        if state in ST.AFTER:
            ST.AFTER[state](s)
        D.check(d2, near, want, f"{state} host path")
        D.check(*device_field(s, lo, hi, max_d2), want, f"{state} device path")
    finally:
        s.close()


def test_error_codes_and_empty_cases():
    lib = _lib.load()
    out, near = np.full((1, 1, 1), 77, np.int32), np.full((1, 1, 1), 77, np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    box = lambda v: None if v is None else (C.c_int32 * 3)(*v)
    field = lambda s, lo=(1, 1, 1), hi=(2, 2, 2), max_d2=4, flags=0, o=out, n=near, dev=0: lib.vrt_distance_field(
        C.c_void_p(s._ctx) if s is not None else None, box(lo), box(hi), max_d2, flags, p(o), p(n), dev)
    mat, rgb, params = D.grid("s1"), D.colours("s1"), D.params("s1")
    s = NativeSession(lib, "vrt_", host.make_config(16, 8, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=2, grid_res=128))
    try:
        assert field(s) == _abi.VRT_E_STATE                                                # before vrt_prepare
        orc.setup(s, mat, rgb, params)
        s.upload_voxels(mat, rgb)
        assert field(s) == _abi.VRT_E_STATE                                                # after an upload that no prepare has followed
        with pytest.raises(NativeError):
            s.distance_field((1, 1, 1), (2, 2, 2), 4)
        assert field(s, max_d2=-1) == _abi.VRT_E_INVALID                                   # (arguments are checked before the state)
        s.prepare()
        assert field(s) == _abi.VRT_OK and out[0, 0, 0] == D.FAR and near[0, 0, 0] == -1
        assert field(s, n=None) == _abi.VRT_OK                                             # nearest may be NULL
        assert field(None) == _abi.VRT_E_INVALID
        assert field(s, lo=None) == _abi.VRT_E_INVALID
        assert field(s, hi=None) == _abi.VRT_E_INVALID
        assert field(s, o=None) == _abi.VRT_E_INVALID
        for lo, hi in (((2, 1, 1), (1, 2, 2)), ((-1, 0, 0), (0, 1, 1)), ((127, 127, 127), (128, 128, 129))):
            assert field(s, lo, hi) == _abi.VRT_E_INVALID, (lo, hi)
        assert field(s, max_d2=-1) == _abi.VRT_E_INVALID
        assert field(s, max_d2=_abi.DIST_MAX_D2 + 1) == _abi.VRT_E_INVALID
        assert field(s, max_d2=_abi.DIST_MAX_D2) == field(s, max_d2=0) == _abi.VRT_OK
        assert field(s, flags=2) == _abi.VRT_E_INVALID
        assert field(s, flags=0x80000000) == _abi.VRT_E_INVALID
        assert field(s, flags=_abi.DIST_TO_EMPTY) == _abi.VRT_OK and out[0, 0, 0] == 0
        assert field(s, dev=2) == _abi.VRT_E_INVALID
        assert field(s, dev=-1) == _abi.VRT_E_INVALID
        out[:] = 77                                                                        # empty boxes: OK, nothing written
        assert field(s, (5, 5, 5), (5, 9, 9)) == field(s, (128, 128, 128), (128, 128, 128)) == _abi.VRT_OK and out[0, 0, 0] == 77
        assert s.distance_field((3, 3, 3), (3, 4, 4)).shape == (0, 1, 1)
        d2, n = s.distance_field((3, 3, 3), (4, 4, 3), nearest=True)
        assert d2.shape == n.shape == (1, 1, 0)
        with pytest.raises(ValueError):
            s.distance_field((1, 1, 1), (2, 2, 2), out=np.zeros((2, 1, 1), np.int32))
    finally:
        s.close()


# ---- the facade -----------------------------------------------------------------------------------------------------------------------
W, H = 64, 36


def renderer():
    from voxel_rt2_amd.renderer import Renderer
    r = Renderer(dx=1 / 64, image_res=(W, H), up=(0, 1, 0), voxel_edges=0.06, exposure=1.5, max_depth=2, seed=7, sky_res=0)
    r.set_directional_light((0.6, 1.0, 0.4), 0.1, (1.0, 0.95, 0.85))
    r.background_color[None] = (0.35, 0.5, 0.75)
    r.floor_height[None] = -0.3
    return r


def blob(r):
    """a slab, an L-shaped block in two colours and materials on it, a lone voxel, and a block pressed into the grid's corner"""
    for x in range(-8, 9):
        for z in range(-8, 9):
            r.set_voxel((x, -3, z), 11, (0.8, 0.3, 0.2))
    for x in range(-3, 4):
        for y in range(-2, 5):
            for z in range(-2, 3):
                if x < 1 or y < 1:
                    r.set_voxel((x, y, z), 54 if x < 0 else 2, (0.2, 0.7, 0.9) if y < 2 else (0.9, 0.8, 0.1))
    r.set_voxel((7, 5, 7), 21, (0.1, 0.9, 0.1))
    for x in range(60, 64):
        for y in range(60, 64):
            for z in range(60, 64):
                r.set_voxel((x, y, z), 1, (0.5, 0.5, 0.5))


def predicted_grow(mat, rgb, lo, hi, md, color, m):
    sl = tuple(slice(l, h) for l, h in zip(lo, hi))
    d2, near = D.brute_targets(mat, lo, hi, md)
    grow = (mat[sl] <= 0) & (d2 <= md)
    src = np.where(grow, near, 0)
    new_m = np.full(grow.shape, m, np.int8) if m is not None else mat.reshape(-1)[src]
    new_c = np.broadcast_to(np.array(color, np.uint8), grow.shape + (3,)) if color is not None else rgb.reshape(-1, 3)[src]
    mat, rgb = mat.copy(), rgb.copy()
    mat[sl] = np.where(grow, new_m, mat[sl])
    rgb[sl] = np.where(grow[..., None], new_c, rgb[sl])
    return mat, rgb, int(grow.sum())


def predicted_shrink(mat, rgb, lo, hi, md):
    sl = tuple(slice(l, h) for l, h in zip(lo, hi))
    d2, _ = D.brute_offsets(mat, lo, hi, md, to_empty=True)
    gone = (mat[sl] > 0) & (d2 <= md)
    mat, rgb = mat.copy(), rgb.copy()
    mat[sl] = np.where(gone, 0, mat[sl])
    rgb[sl] = np.where(gone[..., None], 0, rgb[sl])
    return mat, rgb, int(gone.sum())


def assert_equals_fresh(e, mat, rgb, label):
    g = e.voxel_grid_res
    m, c = e.session.fetch_voxels((0, 0, 0), (g, g, g))
    assert m.tobytes() == mat.tobytes() and c.tobytes() == rgb.tobytes(), f"{label}: {(m != mat).sum()} materials, {(c != rgb).sum()} colour bytes differ"
    assert e.voxel_material.tobytes() == m.tobytes() and e.voxel_color.tobytes() == c.tobytes(), label + ": the host mirror is out of step"
    f = renderer()
    try:
        f.set_voxel_arrays(mat, rgb)
        f.prepare_data()
        e.reset_framebuffer()
        for r in (e, f):
            r.accumulate(4)
        a, b = e.fetch_hdr(), f.fetch_hdr()
        assert a.tobytes() == b.tobytes() and a.std() > 0, f"{label}: the frame differs from a fresh context's in {(a != b).sum()} values"
    finally:
        f.session.close()


def test_renderer_signed_field_is_the_two_calls():
    e = renderer()
    try:
        with pytest.raises(NativeError):
            e.distance_field((0, 0, 0), (4, 4, 4))
        blob(e)
        e.prepare_data()
        lo, hi = (50, 55, 52), (80, 76, 78)
        sl = tuple(slice(l, h) for l, h in zip(lo, hi))
        out, inn = (e.distance_field(lo, hi, radius=6.5, to_empty=t, nearest=True) for t in (False, True))
        for got, t in ((out, False), (inn, True)):
            D.check(*got, D.reference(e.voxel_material, lo, hi, 42, t), f"facade to_empty={t}")          # floor(6.5^2) = 42
        sd, sn = e.distance_field(lo, hi, radius=6.5, nearest=True, signed=True)
        solid = e.voxel_material[sl] > 0
        assert solid.any() and not solid.all()
        assert sd.tobytes() == np.where(solid, -inn[0], out[0]).astype(np.int32).tobytes()
        assert sn.tobytes() == np.where(solid, inn[1], out[1]).astype(np.int32).tobytes()
        assert (sd == D.FAR).any() and (sd[solid] < 0).all() and (sd[~solid] > 0).all()
        assert e.distance_field(lo, hi, radius=6.5, signed=True).tobytes() == sd.tobytes()
        assert e.distance_field(lo, hi).tobytes() == D.reference(e.voxel_material, lo, hi, _abi.DIST_MAX_D2)[0].tobytes()
    finally:
        e.session.close()


@pytest.mark.parametrize("inherit", [False, True])
def test_renderer_grow_equals_a_fresh_context(inherit):
    """(one frame comparison a renderer: vrt_reset does not rewind the frame counter, so only a context's first frames equal a fresh one's)"""
    e = renderer()
    try:
        with pytest.raises(NativeError):
            e.grow_voxels((0, 0, 0), (4, 4, 4), 1)
        blob(e)
        e.prepare_data()
        e.set_voxel((-5, 2, 5), 2, (1.0, 1.0, 1.0))                                         # not yet sent: goes first
        mat, rgb = e.voxel_material.copy(), e.voxel_color.copy()
        lo, hi = (52, 58, 54), (80, 75, 73)                                                 # cuts the slab and the block: solids outside count
        color, m = (None, None) if inherit else ((10, 200, 30), 21)
        n = e.grow_voxels(lo, hi, 2.5, color=color, mat=m)
        mat, rgb, want = predicted_grow(mat, rgb, lo, hi, 6, color, m)
        assert n == want > 500 and e.current_spp == 0
        if inherit:
            sl = tuple(slice(l, h) for l, h in zip(lo, hi))
            assert len(np.unique(mat[sl][mat[sl] > 0])) >= 3 and len(np.unique(rgb[sl].reshape(-1, 3), axis=0)) >= 4   # several payloads were inherited
        assert e.grow_voxels((5, 5, 5), (5, 9, 9), 3) == 0                                  # an empty box
        assert_equals_fresh(e, mat, rgb, f"grow inherit={inherit}")
    finally:
        e.session.close()


def test_renderer_shrink_equals_a_fresh_context():
    e = renderer()
    try:
        with pytest.raises(NativeError):
            e.shrink_voxels((0, 0, 0), (4, 4, 4), 1)
        blob(e)
        e.prepare_data()
        mat, rgb = e.voxel_material.copy(), e.voxel_color.copy()
        lo, hi = (50, 56, 50), (84, 80, 80)
        n = e.shrink_voxels(lo, hi, 1.5, reset=False)
        mat, rgb, want = predicted_shrink(mat, rgb, lo, hi, 2)
        assert n == want > 300 and (mat[60:70, 60:70, 60:70] > 0).any()
        lo, hi = (100, 110, 100), (128, 128, 128)                                           # the block in the grid's corner: its walls do not erode
        n = e.shrink_voxels(lo, hi, 1)
        mat, rgb, want = predicted_shrink(mat, rgb, lo, hi, 1)
        assert n == want == 64 - 27 and (mat[125:, 125:, 125:] > 0).all() and not (mat[124, 124:, 124:] > 0).any()
        assert e.current_spp == 0
        assert_equals_fresh(e, mat, rgb, "shrink")
    finally:
        e.session.close()


def test_grow_then_shrink_contains_the_original():
    e = renderer()
    try:
        blob(e)
        e.prepare_data()
        g = e.voxel_grid_res
        before = e.voxel_material > 0
        lo, hi = (40, 50, 40), (90, 90, 90)
        sl = tuple(slice(l, h) for l, h in zip(lo, hi))
        grown = e.grow_voxels(lo, hi, 3, color=(1, 2, 3), mat=1, reset=False)
        mid = e.voxel_material > 0
        gone = e.shrink_voxels(lo, hi, 3)
        after = e.voxel_material > 0
        assert grown > gone > 0 and (mid >= before).all() and (mid >= after).all()
        assert (after[sl] >= before[sl]).all(), "closing lost a voxel of the original solid"
        assert (after == before)[~np.pad(np.ones([h - l for l, h in zip(lo, hi)], bool), [(l, g - h) for l, h in zip(lo, hi)])].all()
    finally:
        e.session.close()


def test_grow_shrink_example_runs(tmp_path, monkeypatch):
    import sys
    for k, v in (("VRT_RES", "160x90"), ("VRT_FRAMES", "2"), ("VRT_SKY_RES", "32"), ("VRT_MAX_DEPTH", "2"), ("VRT_OUT", str(tmp_path / "grow.png"))):
        monkeypatch.setenv(k, v)
    monkeypatch.syspath_prepend(ROOT)
    sys.modules.pop("scene", None)
    mod = runpy.run_path(os.path.join(ROOT, "examples", "grow_shrink.py"), run_name="grow_shrink")
    r, results = mod["main"]()
    try:
        assert (tmp_path / "grow.png").exists()
        g, s = results["grown"], results["shrunk"]
        assert g["after"] == g["before"] + g["changed"] and g["changed"] > g["before"] // 2
        assert s["after"] == s["before"] - s["changed"] and 0 < s["changed"] < s["before"]
        m, c = r.session.fetch_voxels((0, 0, 0), (r.voxel_grid_res,) * 3)
        assert r.voxel_material.tobytes() == m.tobytes() and r.voxel_color.tobytes() == c.tobytes()
        sl = tuple(slice(int(a), int(b)) for a, b in zip(g["lo"], g["hi"]))
        colours = {tuple(v) for v in c[sl][m[sl] == 54].tolist()}
        assert colours == {(230, 150, 60), (70, 150, 230)}                                  # grown voxels inherited one of the two
    finally:
        r.session.close()
