"""vrt_update_voxels ON THE DEVICE: a context whose prepared grid was edited box by box (E) against a fresh context given the final
grid through vrt_upload_voxels + vrt_prepare (F), bit for bit -- no tolerance anywhere, every comparison is tobytes() equality:
  (a) the HDR frame after the same accumulate calls, under both schedules of the render stage;
  (b) vrt_trace_probe records of rays from the generators of tests/rays.py, aimed at and around the edited box, in the three walks with
      the culling box off and on -- the step count is the only thing that sees a coarse bit left set, the culled records the only
      thing that sees a culling box that did not follow (on the device or in the host's cull_active);
  (c) for the 128^3 sequences also against the CPU oracle on the final grid, so that E and F are not merely equal to each other.
The sequences (tests/edit.py), each the smallest that can break one thing:
  lone_voxel       a new l0 word and l1 bit ahead of every other (all of l0c shifts), the culling box grows
  last_voxel       the grid becomes empty: bits clear to the top, the culling box becomes lo > hi; then a voxel somewhere else
  unaligned        (3,5,62)..(6,70,67): crosses a brick, a 16-cell and a 64-cell boundary; filled, then half of it cleared
  corners          boxes ending on the grid's faces at (0,0,0) and (G,G,G), then the whole grid (= a plain upload of another scene)
  colour_material  colours only (texels change, the pyramid does not), then material 2 -> 1 on solid voxels
  negative         negative material bytes: texel alpha 0, not occupied
  dense_flip       half of the bricks non-empty under an emitting sun and back: dense_grid selects another kernel geometry
                   (plan_render_variant); no entry point reports it, so what is compared is the frame that kernel renders
  lds_head         the non-empty fine words go from below 1024 (what the pooled kernel keeps in LDS) to above, and back
  *_256            the 256^3 grid: brick-tiled texels, l3, no l0c
  corners_dense    with vrt_set_reference_indexing: reads outside the grid address other cells' bits, near the far faces
Then: the physical sky (the tables survive an edit byte for byte), the device path (a torch tensor), ordering against launches in
flight, a later plain vrt_prepare, the error codes, and the facade (Renderer.set_voxel ... update_voxels)."""
import ctypes as C
import os

import numpy as np
import pytest

import edit as E
import orc
import rays as R
from voxel_rt2_amd import _abi, _lib, host
from voxel_rt2_amd._session import NativeError, NativeSession

pytestmark = pytest.mark.gpu
W, H, DEPTH, SEED = 64, 48, 4, 7
MODES = [w | b for b in (0, R.BOX) for w in R.WALKS.values()]
ORACLE = ("lone_voxel", "last_voxel", "unaligned", "negative", "lds_head")


def config(base, sky_res=0):
    mat, _, params = R.scene(base)
    return host.make_config(W, H, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=DEPTH, seed=SEED, grid_res=mat.shape[0],
                            sky_res=sky_res)


def fresh(base, mat, rgb, reference_indexing=False, cls=None):
    s = NativeSession(_lib.load(), "vrt_", config(base)) if cls is None else cls(config(base))
    orc.setup(s, mat, rgb, R.scene(base)[2])
    if reference_indexing:
        s.set_reference_indexing(True)
    return s


def edited(name, upto, reference_indexing=False, via=None):
    """base grid -> prepare -> the first `upto` edits of the sequence -> reset"""
    base, edits = E.sequence(name)
    s = fresh(base, *E.grids(name)[0], reference_indexing)
    for e in edits[:upto]:
        (via or NativeSession.update_voxels)(s, *e)
    s.reset()
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


def rays_around(name, k):
    """tests/rays.py's families on the grid after edit k: box-aimed rays whose `box` is edit k's own (grown by the culling margin, as
    the generator does), rays from cell boundaries and from inside the final grid's solids, axis-parallel rays."""
    mat = E.grids(name)[k + 1][0]
    lo, hi = E.sequence(name)[1][k][:2]
    G = mat.shape[0]
    aim = np.zeros_like(mat)
    if E.touched(lo, hi, 0) <= 64 ** 3:
        aim[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
    else:                                             # the whole grid: its solids (a thinned-out sample of a dense grid's)
        aim = np.where(np.random.default_rng(1).random(mat.shape) < 20000.0 / max((mat > 0).sum(), 20000), mat > 0, False).astype(np.int8)
    rng = np.random.default_rng([20250611, E.SEQUENCES.index(name), k])
    thin = np.zeros_like(mat)
    solid = np.argwhere(mat > 0)
    if len(solid):
        pick = solid[rng.integers(0, len(solid), 4000)]
        thin[pick[:, 0], pick[:, 1], pick[:, 2]] = 1
    return np.ascontiguousarray(np.concatenate([R.box_aimed(rng, G, aim, n=1200), R.boundary_origins(rng, G, thin, n=600), R.axis_parallel(rng, G, n=300)]))


def cases():
    return [(name, k) for name in E.SEQUENCES for k in range(len(E.sequence(name)[1]))]


@pytest.mark.parametrize("schedule", ["pool", "fused"])
@pytest.mark.parametrize("name,k", cases())
def test_edited_context_equals_fresh_context(name, k, schedule, monkeypatch):
    monkeypatch.setenv("VRT_RENDER", schedule)
    ref = name == "corners_dense"
    base = E.sequence(name)[0]
    e, f = edited(name, k + 1, ref), fresh(base, *E.grids(name)[k + 1], ref)
    try:
        if schedule == "pool":                        # (the probes do not depend on the schedule)
            rays = rays_around(name, k)
            for mode in MODES:
                got, want = probe(e, mode, rays), probe(f, mode, rays)
                bad = np.flatnonzero((got.view(np.uint8).reshape(len(rays), -1) != want.view(np.uint8).reshape(len(rays), -1)).any(axis=1))
                assert got.tobytes() == want.tobytes(), f"{name} edit {k} mode {mode}: {bad.size} of {len(rays)} records differ: {R.describe(rays, got, want, bad)}"
        a, b = frame(e), frame(f)
        assert a.tobytes() == b.tobytes(), f"{name} edit {k} ({schedule}): {(a != b).sum()} of {a.size} values differ"
        assert e.stats()["pipeline_flags"] & 0xFF == f.stats()["pipeline_flags"] & 0xFF
    finally:
        e.close()
        f.close()


@pytest.mark.parametrize("name", ORACLE)
def test_edited_context_equals_oracle_on_the_final_grid(name):
    base, edits = E.sequence(name)
    k = len(edits) - 1
    mat, rgb = E.grids(name)[-1]
    e, o = edited(name, len(edits)), fresh(base, mat, rgb, cls=lambda cfg: orc.Oracle(cfg, threads=4))
    try:
        rays = rays_around(name, k)
        want = np.zeros(len(rays), R.REC)
        orc.lib().orc_unit_raytrace_n(C.c_void_p(o._ctx), len(rays), orc.fptr(rays), orc.fptr(want))
        R.check_probe(lambda mode, r: probe(e, mode, r), rays, want, label=f"{name} against the oracle")
        a, b = frame(e), frame(o)
        assert a.tobytes() == b.tobytes(), f"{name}: {(a != b).sum()} of {a.size} values differ from the oracle's"
    finally:
        e.close()
        o.close()


def test_physical_sky_tables_survive_an_edit():
    """s6 with clouds and atmosphere precomputed at the sky tests' table size: an edit leaves both tables alone, byte for byte, and the
    edited context renders what a fresh one with the same precompute renders."""
    cloud = np.load(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "data", "cloud_texture.npy"))
    mat, rgb, params = R.scene("s6")
    edit = E._pattern((50, 30, 60), (63, 41, 69), seed=8, m=21)           # a block hanging over the ground, aligned to nothing
    final = E.apply_numpy(mat, rgb, edit)

    def session(m, c):
        s = NativeSession(_lib.load(), "vrt_", config("s6", sky_res=64))
        orc.setup(s, m, c, params, cloud=cloud)
        for _ in range(2):
            s.sky_accumulate_clouds(2)
        for sl in range(4):
            s.sky_compute_slice(sl, 4)
        return s
    e, f = session(mat, rgb), session(*final)
    try:
        before = [e.fetch_buffer(w) for w in (_abi.BUF_SKY_SCATTERING, _abi.BUF_SKY_TRANSMITTANCE, _abi.BUF_TRANS_LUT)]
        assert before[0].max() > 0 and before[1].max() > 0
        e.update_voxels(*edit)
        after = [e.fetch_buffer(w) for w in (_abi.BUF_SKY_SCATTERING, _abi.BUF_SKY_TRANSMITTANCE, _abi.BUF_TRANS_LUT)]
        for x, y in zip(before, after):
            assert x.tobytes() == y.tobytes()
        e.reset()
        a, b = frame(e), frame(f)
        assert a.tobytes() == b.tobytes(), f"{(a != b).sum()} of {a.size} values differ"
        e.sky_accumulate_clouds(2)                                        # the cloud passes go on counting where they were
        f.sky_accumulate_clouds(2)
        assert e.fetch_buffer(_abi.BUF_SKY_SCATTERING).tobytes() == f.fetch_buffer(_abi.BUF_SKY_SCATTERING).tobytes()
    finally:
        e.close()
        f.close()


@pytest.mark.parametrize("name", ["lone_voxel", "unaligned"])
def test_device_path_equals_host_path(name):
    import torch
    keep = []

    def from_torch(s, lo, hi, bmat, brgb):
        tm, tc = torch.from_numpy(np.ascontiguousarray(bmat)).cuda(), torch.from_numpy(np.ascontiguousarray(brgb)).cuda()
        torch.cuda.synchronize()                      # the tensors are written on torch's stream, read on the context's
        keep.append((tm, tc))
        s.update_voxels(lo, hi, tm.data_ptr(), tc.data_ptr(), on_device=True)
    n = len(E.sequence(name)[1])
    d, h = edited(name, n, via=from_torch), edited(name, n)
    try:
        rays = rays_around(name, n - 1)
        for mode in MODES:
            assert probe(d, mode, rays).tobytes() == probe(h, mode, rays).tobytes(), mode
        a, b = frame(d), frame(h)
        assert a.tobytes() == b.tobytes()
    finally:
        d.close()
        h.close()


def test_launches_in_flight_see_the_old_grid():
    """Six accumulate calls queued, no synchronisation, then the edit: the frame is the un-edited scene's.  After a reset the frame is
    that of a context that was given the final grid from the start and the same calls."""
    name = "dense_flip"
    base, edits = E.sequence(name)
    states = E.grids(name)

    def six(s):
        for _ in range(6):
            s.accumulate(4)
    e, u, f = fresh(base, *states[0]), fresh(base, *states[0]), fresh(base, *states[1])
    try:
        six(e)
        e.update_voxels(*edits[0])
        six(u)
        a, b = e.fetch_hdr(), u.fetch_hdr()
        assert a.tobytes() == b.tobytes(), f"launches queued before the edit saw it: {(a != b).sum()} of {a.size} values differ"
        six(f)
        e.reset()
        f.reset()
        a, b = frame(e), frame(f)
        assert a.tobytes() == b.tobytes(), f"{(a != b).sum()} of {a.size} values differ"
        u.reset()
        assert a.tobytes() != frame(u).tobytes()      # (the edit is in view)
    finally:
        for s in (e, u, f):
            s.close()


def test_plain_prepare_after_edits_still_equals_fresh():
    """d_mat and d_rgb were kept current: vrt_prepare without an upload rebuilds the same grid."""
    name = "corners"
    e, f = edited(name, 2), fresh("sunlit", *E.grids(name)[2])
    try:
        e.prepare()
        rays = rays_around(name, 1)
        for mode in MODES:
            assert probe(e, mode, rays).tobytes() == probe(f, mode, rays).tobytes(), mode
        assert frame(e).tobytes() == frame(f).tobytes()
    finally:
        e.close()
        f.close()


def test_error_codes_and_the_empty_box():
    lib = _lib.load()
    mat, rgb, params = R.scene("sunlit")
    one = (np.full((1, 1, 1), 11, np.int8), np.full((1, 1, 1, 3), 200, np.uint8))

    def call(s, lo, hi, m=one[0], c=one[1], on_device=0):
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        return lib.vrt_update_voxels(C.c_void_p(s._ctx), None if lo is None else (C.c_int32 * 3)(*lo), None if hi is None else (C.c_int32 * 3)(*hi),
                                     p(m), p(c), on_device)
    s = NativeSession(lib, "vrt_", config("sunlit"))
    try:
        assert call(s, (1, 1, 1), (2, 2, 2)) == _abi.VRT_E_STATE                      # before vrt_prepare
        orc.setup(s, mat, rgb, params)
        frame(s)
        s.upload_voxels(mat, rgb)
        assert call(s, (1, 1, 1), (2, 2, 2)) == _abi.VRT_E_STATE                      # after an upload that no prepare has followed
        with pytest.raises(NativeError):
            s.update_voxels((1, 1, 1), (2, 2, 2), *one)
        s.prepare()
        for lo, hi in (((2, 1, 1), (1, 2, 2)), ((1, 1, 5), (2, 2, 4)), ((-1, 0, 0), (0, 1, 1)), ((127, 127, 127), (128, 128, 129)), ((0, 200, 0), (1, 201, 1))):
            assert call(s, lo, hi) == _abi.VRT_E_INVALID, (lo, hi)
        assert call(s, None, (1, 1, 1)) == call(s, (0, 0, 0), None) == _abi.VRT_E_INVALID
        assert call(s, (1, 1, 1), (2, 2, 2), m=None) == call(s, (1, 1, 1), (2, 2, 2), c=None) == _abi.VRT_E_INVALID
        assert call(s, (1, 1, 1), (2, 2, 2), on_device=2) == call(s, (1, 1, 1), (2, 2, 2), on_device=-1) == _abi.VRT_E_INVALID
        for lo, hi in (((5, 5, 5), (5, 9, 9)), ((128, 128, 128), (128, 128, 128)), ((0, 0, 0), (0, 0, 0))):
            assert call(s, lo, hi) == _abi.VRT_OK, (lo, hi)                           # empty boxes
        s.update_voxels((3, 3, 3), (3, 4, 4), np.zeros((0, 1, 1), np.int8), np.zeros((0, 1, 1, 3), np.uint8))
        with pytest.raises(ValueError):
            s.update_voxels((3, 3, 3), (4, 4, 4), np.zeros((2, 1, 1), np.int8), np.zeros((2, 1, 1, 3), np.uint8))
        s.reset()
        s2 = fresh("sunlit", mat, rgb)
        frame(s2)
        s2.reset()
        assert frame(s).tobytes() == frame(s2).tobytes()                              # nothing of all this changed the grid
        s2.close()
    finally:
        s.close()


def test_renderer_update_voxels_equals_authoring_everything():
    from voxel_rt2_amd.renderer import Renderer
    first = [((x, -3, z), 11, (0.8, 0.3, 0.2)) for x in range(-4, 5) for z in range(-4, 5)]
    later = [((0, -2, 0), 21, (0.2, 0.9, 0.3)), ((1, -2, 0), 2, (1.0, 1.0, 1.0)), ((-30, 17, 5), 54, (0.3, 0.3, 0.9)), ((0, -3, 0), 0, (0.0, 0.0, 0.0))]

    def renderer():
        r = Renderer(dx=1 / 64, image_res=(W, H), up=(0, 1, 0), voxel_edges=0.06, exposure=1.5, max_depth=DEPTH, seed=SEED, sky_res=0)
        r.set_directional_light((0.6, 1.0, 0.4), 0.1, (1.0, 0.95, 0.85))
        r.background_color[None] = (0.35, 0.5, 0.75)
        r.floor_height[None] = -0.3
        return r
    e, f = renderer(), renderer()
    try:
        for v in first:
            e.set_voxel(*v)
        assert e.dirty_box() == ((0, 0, 0), (128, 128, 128))                          # nothing uploaded yet: the whole grid
        e.prepare_data()
        assert e.dirty_box()[0] == e.dirty_box()[1]
        for v in later:
            e.set_voxel(*v)
        assert e.dirty_box() == ((34, 61, 64), (66, 82, 70))
        e.update_voxels()
        assert e.dirty_box()[0] == e.dirty_box()[1] and e.current_spp == 0
        for v in first + later:
            f.set_voxel(*v)
        f.update_voxels()                                                             # not prepared yet: prepare_data()
        for r in (e, f):
            r.accumulate(4)
        assert e.fetch_hdr().tobytes() == f.fetch_hdr().tobytes()
        assert e.fetch_hdr().std() > 0
    finally:
        e.session.close()
        f.session.close()
