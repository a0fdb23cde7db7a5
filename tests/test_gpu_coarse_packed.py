"""The packed coarse entry of the pooled kernels' staged 128^3 view ON THE DEVICE (LdsPyramid2<128>, vrt_kernels.hip; coarse_pack,
vrt_trace.h): a 64x48 frame at depth 4, four fused samples in one launch, rendered by the pooled kernel -- flat descent over the staged
{l1 word, packed levels 4-6 | fine base} entries, fine words from LDS alone where the scene has no more than the kernel stages -- must be
the frame the fused kernel renders on the same context settings (VRT_RENDER=fused: branchy descent over the unpacked levels), byte for
byte.  The scenes, each for one thing:
  s1      every fine word is staged: the walk's fine words come from LDS alone
  dense   p = 0.5: 32768 fine words, 1024 staged: the per-lane choice between LDS and global memory
  sunlit  an emitting sun: SHADE's inline shadow rays walk the same entries through raytrace()
  faces   solids in the outermost layers of all six faces, with holes: walks that step out of the grid (cells -1 and 128)
and one context after vrt_update_voxels box edits (tests/edit.py `lds_head`: the fine words go from below what is staged to above and
back): the entries are packed at every launch from the levels as they stand, so they follow an edit with nothing else to refresh."""
import numpy as np
import pytest

import edit as E
import orc
import rays as R
from voxel_rt2_amd import _lib, host, scenes
from voxel_rt2_amd._session import NativeSession

pytestmark = pytest.mark.gpu
W, H, DEPTH, SEED, SAMPLES = 64, 48, 4, 7, 4
STAGED = E.POOL_FINE_WORDS


def faces():
    """(mat, rgb, params): the outermost layer of every face of the grid 30 % solid, a lamp and a block inside."""
    mat, rgb = scenes.empty()
    rng = np.random.default_rng(20250702)
    shell = np.zeros(mat.shape, bool)
    for a in range(3):
        for side in (0, 127):
            idx = [slice(None)] * 3
            idx[a] = side
            shell[tuple(idx)] = True
    on = shell & (rng.random(mat.shape) < 0.3)
    mat[on] = 1
    rgb[on] = rng.integers(40, 256, (int(on.sum()), 3))
    mat[56:72, 100:104, 56:72], rgb[56:72, 100:104, 56:72] = 2, (255, 240, 220)        # material 2 emits
    mat[40:60, 30:50, 70:90], rgb[40:60, 30:50, 70:90] = 11, (200, 90, 60)
    return mat, rgb, dict(R.FLOOR, floor_height=-2.0)


def grid(name):
    return faces() if name == "faces" else R.scene(name)


def fine_words(mat):
    return int((E.rebuild(mat, np.zeros(mat.shape + (3,), np.uint8))["l0"] != 0).sum())


def session(mat, rgb, params):
    cfg = host.make_config(W, H, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=DEPTH, seed=SEED, grid_res=128)
    s = NativeSession(_lib.load(), "vrt_", cfg)
    orc.setup(s, mat, rgb, params)
    return s


def frame(s):
    s.accumulate(SAMPLES)
    return s.fetch_hdr()


def rendered(schedule, monkeypatch, mat, rgb, params, earlier=0):
    """`earlier`: frames rendered and dropped first (a reset clears the accumulation, the frame counter goes on)"""
    monkeypatch.setenv("VRT_RENDER", schedule)          # read when the context is created
    s = session(mat, rgb, params)
    try:
        for _ in range(earlier):
            frame(s)
            s.reset()
        return frame(s)
    finally:
        s.close()


def same(a, b, label):
    assert a.tobytes() == b.tobytes(), f"{label}: {(a != b).sum()} of {a.size} values differ"
    assert np.isfinite(a).all() and a.std() > 0, f"{label}: nothing rendered"


@pytest.mark.parametrize("name", ["s1", "dense", "sunlit", "faces"])
def test_pooled_frame_equals_fused_frame(name, monkeypatch):
    mat, rgb, params = grid(name)
    assert mat.shape == (128, 128, 128)
    if name == "s1":
        assert fine_words(mat) <= STAGED
    if name == "dense":
        assert fine_words(mat) > STAGED
    if name == "sunlit":
        assert max(params["light_color"]) > 0
    if name == "faces":
        assert all((mat[tuple(slice(None) if k != a else side for k in range(3))] > 0).any() for a in range(3) for side in (0, 127))
    same(rendered("pool", monkeypatch, mat, rgb, params), rendered("fused", monkeypatch, mat, rgb, params), name)


def test_pooled_frame_follows_a_box_edit(monkeypatch):
    """A pooled context, prepared on the base grid, rendered, then edited box by box: after each edit its frame is that of a FUSED context
    given the grid as it then stands from the start (and as many frames before this one)."""
    base, edits = E.sequence("lds_head")
    states = E.grids("lds_head")
    params = R.scene(base)[2]
    counts = [fine_words(m) for m, _ in states]
    assert counts[0] <= STAGED < counts[1] and counts[2] == counts[0]
    want = [rendered("fused", monkeypatch, m, c, params, earlier=k) for k, (m, c) in enumerate(states)]
    monkeypatch.setenv("VRT_RENDER", "pool")
    s = session(*states[0], params)
    try:
        same(frame(s), want[0], "base")
        for k, e in enumerate(edits):
            s.update_voxels(*e)
            s.reset()
            same(frame(s), want[k + 1], f"after edit {k}")
        assert want[0].tobytes() != want[1].tobytes()    # (the edit is in view)
    finally:
        s.close()
