"""vrt_label_components ON THE DEVICE, byte for byte against the brute forces of tests/label.py, over every cell of every box, plus the
result record:
  - every case family (6-, 18-, 26-connectivity; solid and empty members) in a 128^3 context at an unaligned offset, on the host path
    and on the device path (torch tensors poisoned with 0x5A5A5A5A); three cases at 256^3, whose labels exceed 2^23;
  - the half-full `dense`: 64^3 boxes at two offsets under every connectivity and member kind, and the whole 128^3 grid, solid,
    6-connected (19 255 components of 1 049 143 cells); `s1`, the whole grid, empty, 6-connected: one component of 2 093 815 cells --
    the contention case;
  - label, edit, label queued on the device path without a wait in between: the first sees the old grid, the second the new one;
  - frames accumulated with calls interleaved == frames without, vrt_get_stats unchanged; a context with frames in flight, with ReSTIR,
    on a row tile answers as a fresh one (tests/states.py);
  - the error codes and empty cases of include/vrt_api.h, one by one;
  - the facade on a fresh context, each against numpy-predicted grids: components, floating_voxels, remove_floating, sealed_cavities on
    a hollow box with and without a one-voxel hole; examples/detach.py."""
import ctypes as C
import functools
import os
import runpy

import numpy as np
import pytest

import distance as D
import label as L
import orc
import radiance as X
import states as ST
from voxel_rt2_amd import _abi, _lib, host
from voxel_rt2_amd._session import NativeError, NativeSession

pytestmark = pytest.mark.gpu
ROOT = L.ROOT
POISON = 0x5A5A5A5A


def session(name, width=16, height=8, **kw):
    """a prepared context on a named grid of tests/label.py"""
    mat, params = L.grid(name), L.params(name)
    cfg = host.make_config(width, height, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=2, grid_res=mat.shape[0], **kw)
    s = NativeSession(_lib.load(), "vrt_", cfg)
    orc.setup(s, mat, L.colours(name), params)
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


def device_labels(s, lo, hi, conn=6, empty=False, result=True, sync=True):
    """The device path: poisoned tensors on the device, the work queued on the context's stream, read back after a sync."""
    import torch
    shape = tuple(h - l for l, h in zip(lo, hi))
    labels = torch.full(shape, POISON, dtype=torch.int32, device="cuda")
    record = torch.full((4,), POISON, dtype=torch.int32, device="cuda") if result else None
    torch.cuda.synchronize()                          # the tensors are written on torch's stream, then on the context's
    s.label_components(lo, hi, conn, empty, out=(labels, record) if result else labels)
    if not sync:
        return labels, record
    s.sync()
    return read_back(labels, record)


def read_back(labels, record):
    rec = None
    if record is not None:
        r = record.cpu().numpy().view(_abi.LABEL_RESULT)[0]
        rec = {k: int(r[k]) for k in ("cells", "components", "reserved")}
    return labels.cpu().numpy(), rec


def both_paths(s, name):
    c = L.CASES[name]
    want = L.expected(name)
    args = (c["lo"], c["hi"], c["conn"], c["empty"])
    L.check(*s.label_components(*args), want, name + " host path")
    L.check(*device_labels(s, *args), want, name + " device path")
    assert device_labels(s, *args, result=False)[0].tobytes() == want[0].tobytes(), name + ": device path without a record"


@pytest.mark.parametrize("name", L.FAMILY_NAMES)
def test_device_equals_brute_force(live, name):
    both_paths(live("families"), name)


@pytest.mark.parametrize("name", tuple(L.CASES_256))
def test_device_equals_brute_force_256(live, name):
    assert L.expected(name)[0].max() > 1 << 23 and L.expected(name)[1]["components"] >= 1
    both_paths(live(L.CASES[name]["grid"]), name)


@pytest.mark.parametrize("name", L.DENSE_NAMES)
def test_half_full_boxes(live, name):
    both_paths(live("dense"), name)


@pytest.mark.parametrize("name", tuple(L.WHOLE))
def test_whole_grid(live, name):
    """every cell of the 128^3 grid: the half-full scene's 19 255 solid components, and the sparse scene's one empty component, which
    every tile's seam cells unite into at once"""
    c = L.CASES[name]
    want = L.expected(name)
    assert want[1] == (dict(cells=1049143, components=19255, reserved=0) if name.startswith("dense") else dict(cells=2093815, components=1, reserved=0))
    L.check(*device_labels(live(c["grid"]), c["lo"], c["hi"], c["conn"], c["empty"]), want, name)


def test_labels_see_the_grid_as_queued():
    import torch
    before_c, after_c = L.CASES["s1_before_edit"], L.CASES["s1_edit"]
    lo, hi, bm, bc = D.S1_EDIT
    s = session("s1")
    try:
        keep = (torch.from_numpy(np.ascontiguousarray(bm)).cuda(), torch.from_numpy(np.ascontiguousarray(bc)).cuda())
        torch.cuda.synchronize()
        args = (before_c["lo"], before_c["hi"], before_c["conn"], before_c["empty"])
        before = device_labels(s, *args, sync=False)                                           # queued, not waited for
        s.update_voxels(lo, hi, keep[0].data_ptr(), keep[1].data_ptr(), on_device=True)
        after = device_labels(s, *args, sync=False)
        s.sync()
        L.check(*read_back(*before), L.expected("s1_before_edit"), "before the edit")
        L.check(*read_back(*after), L.expected("s1_edit"), "after the edit")
        assert L.expected("s1_before_edit")[0].tobytes() != L.expected("s1_edit")[0].tobytes()
    finally:
        s.close()


def test_frames_do_not_notice_labels():
    """accumulate(4) x 3 with calls in between, on the host path and on the device path: HDR, both histories and the statistics as
    without them; and vrt_get_stats is the same before and after a call."""
    import torch
    lo, hi = (30, 50, 40), (70, 70, 80)
    shape = tuple(h - l for l, h in zip(lo, hi))
    t_out = (torch.zeros(shape, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()

    def run(query):
        s = session("sunlit", width=64, height=40)
        try:
            for k in range(3):
                s.accumulate(4)
                if query == "host":
                    s.label_components(lo, hi, (6, 18, 26)[k], empty=k == 2)
                elif query == "device":
                    s.label_components(lo, hi, (6, 18, 26)[k], empty=k == 2, out=t_out)
            frames = [s.fetch_hdr()] + [s.fetch_buffer(w) for w in (_abi.BUF_HISTORY_DIFFUSE, _abi.BUF_HISTORY_SPECULAR)]
            st = s.stats()
            s.label_components(lo, hi, 26)
            assert s.stats() == st
            return frames, st
        finally:
            s.close()
    plain, stats = run(None)
    assert plain[0].std() > 0
    for query in ("host", "device"):
        got, st = run(query)
        for a, b, what in zip(got, plain, ("hdr", "diffuse history", "specular history")):
            assert a.tobytes() == b.tobytes(), f"{query} labels changed the {what}: {(a != b).sum()} of {a.size} values"
        for key in ("path_samples", "render_launches", "temporal_launches", "rays"):
            assert st[key] == stats[key], (query, key)


BUSY = ((20, 44, 44), (56, 68, 70), 26)


@functools.lru_cache(maxsize=None)
def busy_reference():
    m = X.scene("sunlit_d5")[0]
    labels = L.reference(m, BUSY[0], BUSY[1], BUSY[2], False)
    return labels, L.record_of(labels, m.shape[0], BUSY[0])


@pytest.mark.parametrize("state", ["big_frame", "restir", "tile"])
def test_a_busy_context_answers_as_a_fresh_one(state):
    """frames in flight with their pass pending / ReSTIR on / a row tile (tests/states.py): the same bytes as the brute force, which is
    what a fresh context gives (test_device_equals_brute_force)"""
    lo, hi, conn = BUSY
    want = busy_reference()
    assert want[1]["components"] > 1 and want[1]["cells"] < want[0].size
    s = ST.open_session(X, "sunlit_d5", state)
    try:
        got = s.label_components(lo, hi, conn)                                                # the host path does not force the pending pass
        if state in ST.AFTER:
            ST.AFTER[state](s)
        L.check(*got, want, f"{state} host path")
        L.check(*device_labels(s, lo, hi, conn), want, f"{state} device path")
    finally:
        s.close()


def test_error_codes_and_empty_cases():
    lib = _lib.load()
    out, rec = np.full((1, 1, 1), 77, np.int32), np.full(1, 77, _abi.LABEL_RESULT)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    box = lambda v: None if v is None else (C.c_int32 * 3)(*v)
    label = lambda s, lo=(1, 1, 1), hi=(2, 2, 2), flags=0, o=out, r=rec, dev=0: lib.vrt_label_components(
        C.c_void_p(s._ctx) if s is not None else None, box(lo), box(hi), flags, p(o), p(r), dev)
    mat, rgb, params = L.grid("s1"), L.colours("s1"), L.params("s1")
    s = NativeSession(lib, "vrt_", host.make_config(16, 8, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=2, grid_res=128))
    try:
        assert label(s) == _abi.VRT_E_STATE                                                # before vrt_prepare
        orc.setup(s, mat, rgb, params)
        s.upload_voxels(mat, rgb)
        assert label(s) == _abi.VRT_E_STATE                                                # after an upload that no prepare has followed
        with pytest.raises(NativeError):
            s.label_components((1, 1, 1), (2, 2, 2))
        assert label(s, flags=6) == _abi.VRT_E_INVALID                                     # (arguments are checked before the state)
        s.prepare()
        assert label(s) == _abi.VRT_OK and out[0, 0, 0] == -1 and rec[0]["cells"] == 0 and rec[0]["components"] == 0 and rec[0]["reserved"] == 0
        assert label(s, flags=_abi.LABEL_EMPTY) == _abi.VRT_OK and out[0, 0, 0] == (128 + 1) * 128 + 1 and rec[0]["cells"] == 1 and rec[0]["components"] == 1
        assert label(s, r=None) == _abi.VRT_OK                                             # result may be NULL
        assert label(None) == _abi.VRT_E_INVALID
        assert label(s, lo=None) == _abi.VRT_E_INVALID
        assert label(s, hi=None) == _abi.VRT_E_INVALID
        assert label(s, o=None) == _abi.VRT_E_INVALID
        for lo, hi in (((2, 1, 1), (1, 2, 2)), ((-1, 0, 0), (0, 1, 1)), ((127, 127, 127), (128, 128, 129))):
            assert label(s, lo, hi) == _abi.VRT_E_INVALID, (lo, hi)
        for flags in (1, 2, 3, 4, 5):
            assert label(s, flags=flags) == _abi.VRT_OK, flags
        for flags in (6, 7, 8, 0x10, 0x80000000):
            assert label(s, flags=flags) == _abi.VRT_E_INVALID, flags
        assert label(s, dev=2) == _abi.VRT_E_INVALID
        assert label(s, dev=-1) == _abi.VRT_E_INVALID
        out[:] = 77                                                                        # empty boxes: OK, no label written, the record zeroed
        rec[0] = (5, 5, 5)
        assert label(s, (5, 5, 5), (5, 9, 9)) == _abi.VRT_OK and out[0, 0, 0] == 77 and rec[0].tolist() == (0, 0, 0)
        rec[0] = (5, 5, 5)
        assert label(s, (128, 128, 128), (128, 128, 128)) == _abi.VRT_OK and out[0, 0, 0] == 77 and rec[0].tolist() == (0, 0, 0)
        labels, record = s.label_components((3, 3, 3), (3, 4, 4))
        assert labels.shape == (0, 1, 1) and record == dict(cells=0, components=0, reserved=0)
        import torch
        t = (torch.zeros((1, 0, 2), dtype=torch.int32, device="cuda"), torch.full((4,), POISON, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        s.label_components((3, 3, 3), (4, 3, 5), out=t)                                    # on the device the record is zeroed on the stream
        s.sync()
        assert t[1].cpu().numpy().tolist() == [0, 0, 0, 0]
        with pytest.raises(ValueError):
            s.label_components((1, 1, 1), (2, 2, 2), out=np.zeros((2, 1, 1), np.int32))
        with pytest.raises(ValueError):
            s.label_components((1, 1, 1), (2, 2, 2), connectivity=8)
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
    """a slab; on it an L-shaped block and a post; over it a lone voxel, a bar that touches the post by an edge only, and a block pressed
    into the grid's corner; under the slab a hanging stub"""
    for x in range(-8, 9):
        for z in range(-8, 9):
            r.set_voxel((x, -3, z), 11, (0.8, 0.3, 0.2))
    for x in range(-3, 4):
        for y in range(-2, 5):
            for z in range(-2, 3):
                if x < 1 or y < 1:
                    r.set_voxel((x, y, z), 54 if x < 0 else 2, (0.2, 0.7, 0.9) if y < 2 else (0.9, 0.8, 0.1))
    for y in range(-2, 4):
        r.set_voxel((6, y, 6), 2, (0.5, 0.9, 0.5))
    for x in range(7, 12):
        r.set_voxel((x, 4, 6), 21, (0.9, 0.2, 0.9))                                         # (7, 4, 6) meets the post's top (6, 3, 6) across an edge
    r.set_voxel((7, 5, -7), 21, (0.1, 0.9, 0.1))
    for x in range(60, 64):
        for y in range(60, 64):
            for z in range(60, 64):
                r.set_voxel((x, y, z), 1, (0.5, 0.5, 0.5))
    for y in range(-6, -3):
        r.set_voxel((-5, y, 5), 11, (0.3, 0.3, 0.3))


BLOB_BOX = ((50, 61, 50), (128, 128, 128))           # from the slab's layer (y = -3 -> 61) up: the stub under the slab is outside


def test_renderer_components_match_the_brute_force_table():
    e = renderer()
    try:
        with pytest.raises(NativeError):
            e.label_components()
        blob(e)
        e.prepare_data()
        e.set_voxel((-6, 9, -6), 2, (1.0, 1.0, 1.0))                                        # not yet sent: goes first
        for lo, hi, conn, empty in ((None, None, 6, False), (BLOB_BOX[0], BLOB_BOX[1], 18, False), ((52, 58, 52), (80, 72, 80), 6, True)):
            g = e.voxel_grid_res
            blo, bhi = (lo or (0, 0, 0)), (hi or (g, g, g))
            want = L.reference(e.voxel_material, blo, bhi, conn, empty)
            labels, record = e.label_components(lo, hi, conn, empty)
            L.check(labels, record, (want, L.record_of(want, g, blo)), f"facade conn {conn} empty {empty}")
            rows = L.table_of(want, g, blo)
            t = {k: v.cpu().numpy() for k, v in e.components(lo, hi, conn, empty).items()}
            assert t["root"].tolist() == [r[0] for r in rows] and t["size"].tolist() == [r[1] for r in rows]
            assert t["lo"].tolist() == [list(r[2]) for r in rows] and t["hi"].tolist() == [list(r[3]) for r in rows]
        whole = L.record_of(L.reference(e.voxel_material, (0, 0, 0), (128, 128, 128), 6, False), 128, (0, 0, 0))
        assert whole["components"] == 5                                                     # the slab with what stands on and hangs from it; the bar; the lone voxel; the corner block; the new voxel
    finally:
        e.session.close()


def predicted_floating(mat, lo, hi, conn):
    labels = L.reference(mat, lo, hi, conn, False)
    ground = labels[:, 0, :]
    return (labels >= 0) & ~np.isin(labels, np.unique(ground[ground >= 0]))


@pytest.mark.parametrize("conn", [6, 18])
def test_renderer_floating_voxels_and_remove_floating(conn):
    e = renderer()
    try:
        with pytest.raises(NativeError):
            e.floating_voxels(*BLOB_BOX)
        blob(e)
        e.prepare_data()
        lo, hi = BLOB_BOX
        sl = tuple(slice(l, h) for l, h in zip(lo, hi))
        want = predicted_floating(e.voxel_material, lo, hi, conn)
        got = e.floating_voxels(lo, hi, conn).cpu().numpy()
        assert got.dtype == np.bool_ and got.tobytes() == want.tobytes()
        bar = want[71 - lo[0]:76 - lo[0], 68 - lo[1], 70 - lo[2]]
        assert bar.all() if conn == 6 else not bar.any()                                     # the bar hangs on the post by an edge
        assert want[124 - lo[0]:, 124 - lo[1]:, 124 - lo[2]:].all() and want[71 - lo[0], 69 - lo[1], 57 - lo[2]] and not want[:, 0, :].any()
        mat, rgb = e.voxel_material.copy(), e.voxel_color.copy()
        n = e.remove_floating(lo, hi, conn)
        assert n == int(want.sum()) == (64 + 1 + 5 if conn == 6 else 64 + 1) and e.current_spp == 0
        mat[sl] = np.where(want, 0, mat[sl])
        rgb[sl] = np.where(want[..., None], 0, rgb[sl])
        m, c = e.session.fetch_voxels((0, 0, 0), (128, 128, 128))
        assert m.tobytes() == mat.tobytes() and c.tobytes() == rgb.tobytes()
        assert e.voxel_material.tobytes() == m.tobytes() and e.voxel_color.tobytes() == c.tobytes(), "the host mirror is out of step"
        assert (m[59, 58:61, 69] > 0).all()                                                 # the stub under the slab, outside the box, stays
        assert e.remove_floating(lo, hi, conn) == 0 and not e.floating_voxels(lo, hi, conn).any().item()
        assert e.remove_floating((5, 5, 5), (5, 9, 9)) == 0                                 # an empty box
    finally:
        e.session.close()


@pytest.mark.parametrize("hole", [False, True])
def test_renderer_sealed_cavities(hole):
    e = renderer()
    try:
        for x in range(-6, 5):                                                              # a hollow box: 11 x 9 x 10 outside, walls one voxel thick
            for y in range(-4, 5):
                for z in range(-5, 5):
                    if x in (-6, 4) or y in (-4, 4) or z in (-5, 4):
                        e.set_voxel((x, y, z), 2, (0.7, 0.7, 0.7))
        e.set_voxel((20, 20, 20), 2, (0.7, 0.7, 0.7))
        if hole:
            e.set_voxel((4, 0, 1), 0, (0.0, 0.0, 0.0))
        e.prepare_data()
        lo, hi = (52, 55, 54), (75, 74, 73)
        labels = L.reference(e.voxel_material, lo, hi, 6, True)
        faces = np.concatenate([f.reshape(-1) for f in (labels[0], labels[-1], labels[:, 0], labels[:, -1], labels[:, :, 0], labels[:, :, -1])])
        want = (labels >= 0) & ~np.isin(labels, np.unique(faces[faces >= 0]))
        got = e.sealed_cavities(lo, hi).cpu().numpy()
        assert got.tobytes() == want.tobytes()
        assert int(got.sum()) == (0 if hole else 9 * 7 * 8)
        if not hole:
            assert got[59 - lo[0]:68 - lo[0], 61 - lo[1]:68 - lo[1], 60 - lo[2]:68 - lo[2]].all()
        tight = e.sealed_cavities((58, 60, 59), (69, 69, 69)).cpu().numpy()                  # the box's walls on the call's faces: the cavity still touches none
        assert int(tight.sum()) == (0 if hole else 9 * 7 * 8)
    finally:
        e.session.close()


def test_detach_example_runs(tmp_path, monkeypatch):
    import sys
    for k, v in (("VRT_RES", "160x90"), ("VRT_FRAMES", "1"), ("VRT_SPP", "1"), ("VRT_SKY_RES", "32"), ("VRT_MAX_DEPTH", "2"), ("VRT_OUT", str(tmp_path / "detach.png"))):
        monkeypatch.setenv(k, v)
    monkeypatch.syspath_prepend(ROOT)
    sys.modules.pop("scene", None)
    mod = runpy.run_path(os.path.join(ROOT, "examples", "detach.py"), run_name="detach")
    r, res = mod["main"]()
    try:
        assert (tmp_path / "detach_before.png").exists() and (tmp_path / "detach_after.png").exists()
        g = r.voxel_grid_res
        m, c = r.session.fetch_voxels((0, 0, 0), (g, g, g))
        assert r.voxel_material.tobytes() == m.tobytes() and r.voxel_color.tobytes() == c.tobytes()
        # the grid as it was when the piece was found: the piece back where it came from
        then = m.copy()
        moved = res["cells"] - np.array([0, res["fall"], 0])
        then[tuple(moved.T)] = 0
        then[tuple(res["cells"].T)] = m[tuple(moved.T)]
        lo, hi = (0, g // 2 - 40, 0), (g, g, g)
        want = predicted_floating(then, lo, hi, 6)
        assert want.sum() == res["size"] == len(res["cells"]) > 500
        assert np.array_equal(np.argwhere(want) + np.array(lo), res["cells"])               # the piece it moved is the brute force's floating component
        assert res["fall"] == mod["CUT"][1] - mod["CUT"][0]                                 # by the height of the cut
        assert not predicted_floating(m, lo, hi, 6).any()                                   # nothing floats any more
        # it rests: taken out once more, its box overlaps nothing where it stands and cannot move down at all
        keep_m, keep_c = m[tuple(moved.T)].copy(), c[tuple(moved.T)].copy()
        for (x, y, z) in moved:
            r.set_voxel((x - g // 2, y - g // 2, z - g // 2), 0, (0.0, 0.0, 0.0))
        r.update_voxels(reset=False)
        blo, bhi = r.box_of_voxels(res["new_lo"], res["new_hi"])
        assert not r.overlap_boxes(blo, bhi)[0][0]
        hit = r.sweep_boxes(blo, bhi, np.array([0.0, -0.5, 0.0], np.float32))[0]
        assert hit["kind"] == _abi.SWEEP_VOXEL and hit["t"] == 0.0
    finally:
        r.session.close()
