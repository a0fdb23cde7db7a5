"""vrt_sweep_boxes ON THE DEVICE, bit for bit (tests/sweep.py holds scenes, box families, the brute force's records and the comparison):
  - every box family on every scene == the numpy brute force over every solid voxel, on the host path and on the device path (torch
    tensors on the context's stream);
  - batches of 1, 63, 64, 65 and plan_sweep_chunk() + 1 boxes;
  - a sweep queued before / after an edit sees the old / new grid: a voxel placed in a box's way, then removed again;
  - frames rendered with sweeps queued before, between and after their launches == frames rendered without: HDR, both histories, stats;
  - the same answer on contexts with ReSTIR on, on a row tile, with frames in flight, after vrt_set_reference_indexing(1);
  - error codes; Renderer.sweep_boxes / overlap_boxes / box_of_voxels; examples/drop_boxes.py at a small resolution."""
import ctypes as C
import os
import runpy

import numpy as np
import pytest

import orc
import sweep as W
from voxel_rt2_amd import _abi, _lib
from voxel_rt2_amd._session import NativeError, NativeSession

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def session(name, reference_indexing=False, **kw):
    import cast as K
    s = NativeSession(_lib.load(), "vrt_", K.config(name, **kw))
    mat, rgb, params = W.scene(name)
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


def device_sweep(s, boxes, sync=True):
    """The device path: tensors on the device, the work queued on the context's stream, read back after a sync."""
    import torch
    t_boxes = torch.from_numpy(np.array(boxes).view(np.uint8).reshape(-1)).cuda()
    t_hits = torch.full((len(boxes) * _abi.SWEEP_HIT.itemsize,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                          # the tensors are written on torch's stream, read on the context's
    s.sweep_boxes(t_boxes, t_hits)
    if not sync:
        return t_boxes, t_hits
    s.sync()
    return t_hits.cpu().numpy().view(_abi.SWEEP_HIT)


def host_path_boxes(boxes):
    """The host path refuses a non-zero `reserved` before anything runs: those boxes go through the device path only."""
    return boxes["reserved"] == 0


@pytest.mark.parametrize("scene,fam", W.cases())
def test_device_equals_brute_force(live, scene, fam):
    boxes, want, _ = W.family(scene, fam)
    s = live(scene)
    W.check(device_sweep(s, boxes), boxes, want, f"{scene}/{fam} device path")
    keep = host_path_boxes(boxes)
    W.check(s.sweep_boxes(boxes[keep]), boxes[keep], want[keep], f"{scene}/{fam} host path")


def test_batch_sizes_on_one_voxel(live):
    s = live("one_voxel")
    boxes = np.concatenate([W.family("one_voxel", f)[0] for f in ("random", "resting", "dyadic", "outside")])
    want = np.concatenate([W.family("one_voxel", f)[1] for f in ("random", "resting", "dyadic", "outside")])
    assert len(set(want["kind"].tolist())) == 4
    chunk = W.lib().sweep_emul_chunk()
    for n in (1, 63, 64, 65, chunk + 1):              # the host path stages chunk + 1 boxes in two pieces; more boxes than any grid has waves
        k = -(-n // len(boxes))
        b, w = np.tile(boxes, k)[:n], np.tile(want, k)[:n]
        W.check(s.sweep_boxes(b), b, w, f"host path n={n}")
        W.check(device_sweep(s, b), b, w, f"device path n={n}")


def test_a_sweep_sees_the_grid_as_queued():
    """one_voxel: a box falls beside the lone voxel and meets the floor; an edit puts a voxel in its way, a second edit removes it.  The
    three sweeps and two edits are queued on the stream back to back and read after one sync."""
    import torch
    s = session("one_voxel")
    try:
        p = lambda k: k / 64 - 1
        box = np.zeros(1, _abi.BOX_SWEEP)
        box["lo"], box["hi"], box["move"], box["t_max"] = (p(40), p(70), p(40)), (p(43), p(73), p(43)), (0.0, -1 / 64, 0.0), np.inf
        t_box = torch.from_numpy(box.view(np.uint8).reshape(-1)).cuda()
        out = [torch.zeros(32, dtype=torch.uint8, device="cuda") for _ in range(3)]
        there = (torch.full((1,), 11, dtype=torch.int8, device="cuda"), torch.full((3,), 200, dtype=torch.uint8, device="cuda"))
        gone = (torch.zeros(1, dtype=torch.int8, device="cuda"), torch.zeros(3, dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        s.sweep_boxes(t_box, out[0])                  # queued, not waited for
        s.update_voxels((41, 60, 42), (42, 61, 43), there[0].data_ptr(), there[1].data_ptr(), on_device=True)
        s.sweep_boxes(t_box, out[1])
        s.update_voxels((41, 60, 42), (42, 61, 43), gone[0].data_ptr(), gone[1].data_ptr(), on_device=True)
        s.sweep_boxes(t_box, out[2])
        s.sync()
        a, b, c = (o.cpu().numpy().view(_abi.SWEEP_HIT)[0] for o in out)
        assert a["kind"] == _abi.SWEEP_FLOOR and a["cell"].tolist() == [-1, -1, -1]
        assert b["kind"] == _abi.SWEEP_VOXEL and b["cell"].tolist() == [41, 60, 42] and b["t"] == 9.0 and b["normal"].tolist() == [0.0, 1.0, 0.0]
        assert c.tobytes() == a.tobytes()
        assert s.sweep_boxes(box)[0].tobytes() == a.tobytes()
    finally:
        s.close()


def test_frames_do_not_notice_sweeps():
    """accumulate(4) x 3 with sweeps queued before, between and after the launches, on the host path and on the device path: HDR, both
    histories and the statistics as without them."""
    import torch
    boxes = np.concatenate([W.family("sunlit", "random")[0], W.family("sunlit", "dyadic")[0]])
    t_boxes = torch.from_numpy(np.array(boxes).view(np.uint8).reshape(-1)).cuda()
    t_hits = torch.zeros(len(boxes) * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def run(query):
        s = session("sunlit", width=64, height=40)

        def ask(k):
            if query == "host":
                s.sweep_boxes(boxes[:1 + 233 * k])
            elif query == "device":
                s.sweep_boxes(t_boxes, t_hits)
        try:
            ask(0)
            for k in range(3):
                s.accumulate(4)
                ask(k + 1)
            return [s.fetch_hdr()] + [s.fetch_buffer(w) for w in (_abi.BUF_HISTORY_DIFFUSE, _abi.BUF_HISTORY_SPECULAR)], s.stats()
        finally:
            s.close()
    plain, stats = run(None)
    assert plain[0].std() > 0
    for query in ("host", "device"):
        got, st = run(query)
        for a, b, what in zip(got, plain, ("hdr", "diffuse history", "specular history")):
            assert a.tobytes() == b.tobytes(), f"{query} sweeps changed the {what}: {(a != b).sum()} of {a.size} values"
        for key in ("path_samples", "render_launches", "temporal_launches", "gris_launches", "rays", "dda_iters", "pipeline_flags"):
            assert st[key] == stats[key], (query, key)


def _restir(s):
    s.accumulate(2)
    s.accumulate(2)


def _in_flight(s):
    for _ in range(3):
        s.accumulate(4)                               # not fetched, not waited for


STATES = {"restir": (16, 8, dict(use_restir=True), _restir, False), "tile": (64, 40, dict(rows=(13, 29)), lambda s: s.accumulate(2), False),
          "in_flight": (64, 40, {}, _in_flight, False), "reference_indexing": (16, 8, {}, lambda s: s.accumulate(1), True)}


@pytest.mark.parametrize("state", list(STATES))
@pytest.mark.parametrize("scene", ["sunlit", "s1_256"])
def test_the_answer_does_not_depend_on_the_frame_state(state, scene):
    w, h, kw, apply, ref = STATES[state]
    s = session(scene, reference_indexing=ref, width=w, height=h, **kw)
    try:
        apply(s)
        for fam in ("random", "resting", "dyadic", "outside", "invalid"):
            boxes, want, _ = W.family(scene, fam)
            W.check(device_sweep(s, boxes), boxes, want, f"{state}: {scene}/{fam} device path")
        boxes, want, _ = W.family(scene, "zeros")
        W.check(s.sweep_boxes(boxes), boxes, want, f"{state}: {scene}/zeros host path")
    finally:
        s.close()


def test_error_codes():
    import cast as K
    lib = _lib.load()
    mat, rgb, params = W.scene("sunlit")
    b, h = np.zeros(4, _abi.BOX_SWEEP), np.zeros(4, _abi.SWEEP_HIT)
    b["hi"], b["t_max"] = 0.1, 1.0
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    sweep = lambda s, n=4, bb=b, hh=h, dev=0: lib.vrt_sweep_boxes(C.c_void_p(s._ctx), n, p(bb), p(hh), dev)
    s = NativeSession(lib, "vrt_", K.config("sunlit"))
    try:
        assert sweep(s) == _abi.VRT_E_STATE                                           # before vrt_prepare
        orc.setup(s, mat, rgb, params)
        s.upload_voxels(mat, rgb)
        assert sweep(s) == _abi.VRT_E_STATE                                           # after an upload that no prepare has followed
        with pytest.raises(NativeError):
            s.sweep_boxes(b)
        s.prepare()
        assert sweep(s) == _abi.VRT_OK
        assert sweep(s, bb=None) == sweep(s, hh=None) == sweep(s, n=-1) == sweep(s, dev=2) == sweep(s, dev=-1) == _abi.VRT_E_INVALID
        assert sweep(s, n=0) == _abi.VRT_OK
        bad = b.copy()
        bad["reserved"][2] = 1
        h[:] = 0
        assert sweep(s, bb=bad) == _abi.VRT_E_INVALID and b"reserved" in lib.vrt_last_error() and not h.view(np.uint8).any()   # nothing ran
        got = device_sweep(s, bad)                                                    # on the device path that box is invalid, the others are answered
        assert got[2].tobytes() == W.miss_record(1)[0].tobytes() and got[0].tobytes() == s.sweep_boxes(b)[0].tobytes()
        assert len(s.sweep_boxes(np.zeros(0, _abi.BOX_SWEEP))) == 0
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


def test_renderer_facade_against_the_records():
    r = renderer()
    try:
        with pytest.raises(NativeError):
            r.sweep_boxes((0, 0, 0), (0.1, 0.1, 0.1), (0, -1, 0))                      # nothing prepared yet
        r.prepare_data()
        S = np.argwhere(r.voxel_material > 0)
        rng = np.random.default_rng(5)
        boxes = W.random_boxes(rng, 128, S, -0.3, 400)
        boxes["flags"] = np.arange(400) % 2
        want, _ = W.brute("empty", boxes, S=S, floor_height=-0.3)                      # ("empty": a 128^3 grid; the solids and the floor are handed over)
        got = r.sweep_boxes(boxes["lo"], boxes["hi"], boxes["move"], boxes["t_max"], floor=boxes["flags"] == 0)
        W.check(got, boxes, want, "Renderer.sweep_boxes")
        assert len(set(want["kind"].tolist())) == 4
        still = boxes.copy()
        still["move"], still["t_max"] = 0.0, 1.0
        want0, _ = W.brute("empty", still, S=S, floor_height=-0.3)
        hit, cell = r.overlap_boxes(boxes["lo"], boxes["hi"], floor=boxes["flags"] == 0)
        assert (hit == (want0["kind"] == _abi.SWEEP_START)).all() and (cell == want0["cell"]).all() and 20 < hit.sum() < 380
        one = r.sweep_boxes((0.0, 0.5, 0.0), (0.1, 0.6, 0.1), (0.0, -1.0, 0.0), t_max=np.inf)   # (3,) arguments, scalars
        assert one.shape == (1,) and one[0]["kind"] == _abi.SWEEP_VOXEL
        # an edit box and a sweep box are the same thing: the box of a solid voxel overlaps exactly that voxel, its neighbour's box nothing
        c = S[len(S) // 2]
        lo, hi = r.box_of_voxels(c, c + 1)
        assert lo.dtype == np.float32 and (lo == c / 64 - 1).all() and (hi == (c + 1) / 64 - 1).all()
        hit, cell = r.overlap_boxes(lo, hi, floor=False)
        assert hit[0] and cell[0].tolist() == c.tolist()
        top = np.array([c[0], S[(S[:, 0] == c[0]) & (S[:, 2] == c[2])][:, 1].max() + 1, c[2]])
        assert not r.overlap_boxes(*r.box_of_voxels(top, top + 1), floor=False)[0][0]
        lo, hi = r.box_of_voxels((0, 0, 0), (128, 128, 128))
        assert lo.tolist() == [-1.0] * 3 and hi.tolist() == [1.0] * 3
    finally:
        r.session.close()


def test_drop_boxes_example_ends_at_rest(tmp_path, monkeypatch):
    """examples/drop_boxes.py at a small resolution: every box ends resting -- with the box taken out of the grid its downward sweep is a
    contact at t = 0 -- and no two boxes overlap: with the box taken out, nothing overlaps the space it occupied."""
    import sys
    for k, v in (("VRT_RES", "64x40"), ("VRT_SPP", "1"), ("VRT_SKY_RES", "32"), ("VRT_MAX_DEPTH", "2"), ("VRT_OUT", str(tmp_path / "drop.png"))):
        monkeypatch.setenv(k, v)
    monkeypatch.syspath_prepend(ROOT)
    sys.modules.pop("scene", None)
    mod = runpy.run_path(os.path.join(ROOT, "examples", "drop_boxes.py"), run_name="drop_boxes")
    r, boxes = mod["main"]()
    try:
        assert (tmp_path / "drop.png").exists() and len(boxes) >= 5 and all(b["resting"] for b in boxes)
        half = r.voxel_grid_res // 2
        down = np.array([0.0, -1 / 64, 0.0], np.float32)
        on_boxes = 0
        for b in boxes:
            lo_idx = np.array(b["lo"]) + half
            hi_idx = lo_idx + np.array(b["size"])
            sl = tuple(slice(l, h) for l, h in zip(lo_idx, hi_idx))
            assert (r.voxel_material[sl] == b["mat"]).all()
            keep = r.voxel_material[sl].copy(), r.voxel_color[sl].copy()
            r.session.update_voxels(lo_idx, hi_idx, np.zeros_like(keep[0]), np.zeros_like(keep[1]))     # the box taken out
            lo, hi = r.box_of_voxels(lo_idx, hi_idx)
            hit = r.sweep_boxes(lo, hi, down)[0]
            assert hit["kind"] == _abi.SWEEP_VOXEL and hit["t"] == 0.0 and hit["normal"].tolist() == [0.0, 1.0, 0.0], (b, hit)
            on_boxes += int(hit["cell"][1] > 27)                                                        # above the terrace and its wall: on another box
            assert not r.overlap_boxes(lo, hi)[0][0], b
            r.session.update_voxels(lo_idx, hi_idx, *keep)                                              # and put back
        assert on_boxes >= 2                                                                            # boxes landed on boxes
    finally:
        r.session.close()
