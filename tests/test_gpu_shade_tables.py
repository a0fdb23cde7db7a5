"""The render kernels' tabulated shading terms ON THE DEVICE (packed material rows in the pooled kernels, the face-normal basis and its
guard, texel bytes over 255, the sun cone's pdf from the parameter block), bit for bit against the CPU oracle and the host build:
small frames of the three scene kinds, a material table changed between two accumulate calls of a live pipeline, and rays whose
first hit is a voxel edge or corner met on an exact tie (a step normal with two or three non-zero components)."""
import numpy as np
import pytest

import orc
import shade_tables as st
from voxel_rt2_amd import _abi, _lib, host, materials, scenes
from voxel_rt2_amd._session import NativeSession

pytestmark = pytest.mark.gpu
BUFS = (_abi.BUF_GBUF_DEPTH, _abi.BUF_GBUF_NORMAL, _abi.BUF_GBUF_POSITION, _abi.BUF_GBUF_MAT, _abi.BUF_GBUF_REFL_DEPTH,
        _abi.BUF_HISTORY_DIFFUSE, _abi.BUF_HISTORY_SPECULAR)


def pair(scene, W, H, depth, seed, scene_seed=0):
    mat, rgb, params = scenes.SCENES[scene](scene_seed)
    params = dict(params, use_physical_sky=0, use_clouds=0)
    cfg = host.make_config(W, H, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=depth, seed=seed)
    g, o = NativeSession(_lib.load(), "vrt_", cfg), orc.Oracle(cfg, threads=4)
    for s in (g, o):
        orc.setup(s, mat, rgb, params)
    return g, o


def assert_same_frames(g, o, label):
    a, b = g.fetch_hdr(), o.fetch_hdr()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{label}: {(a.view(np.uint32) != b.view(np.uint32)).sum()} HDR values differ"
    for which in BUFS:
        assert np.array_equal(g.fetch_buffer(which).view(np.uint8), o.fetch_buffer(which).view(np.uint8)), f"{label}: buffer {which}"


# S1 (black sun), the sun-lit scene (the instantiation that evaluates the light sample) and the dense fill (no culling, branchy shadow rays)
CASES = [("s1", 64, 40, 8, 4, 0), ("sunlit", 64, 40, 6, 3, 0), ("dense", 56, 40, 4, 2, 12345)]


@pytest.mark.parametrize("schedule", ["pool", "fused"])
@pytest.mark.parametrize("scene,W,H,depth,spp,scene_seed", CASES)
def test_small_frames_equal_the_oracle(scene, W, H, depth, spp, scene_seed, schedule, monkeypatch):
    monkeypatch.setenv("VRT_RENDER", schedule)
    g, o = pair(scene, W, H, depth, seed=29, scene_seed=scene_seed)
    try:
        for s in (g, o):
            s.accumulate(spp)
        assert_same_frames(g, o, f"{scene} {schedule}")
    finally:
        g.close()
        o.close()


def changed_table():
    """Every row's derived values move: roughness, anisotropy, metallic, clearcoat and its gloss, specular."""
    t = np.array(materials.load_table(), dtype=np.float32, copy=True)
    k = np.arange(128, dtype=np.float32)
    t[:, 7] = 0.15 + 0.8 * ((k * 37) % 128) / 128.0       # roughness
    t[:, 8] = ((k * 11) % 5) / 4.0                        # anisotropic 0 .. 1
    t[:, 4] = ((k * 7) % 3) / 2.0                         # metallic 0, 0.5, 1
    t[:, 5] = 0.1 + 0.9 * ((k * 13) % 16) / 16.0          # specular
    t[:, 11] = ((k * 5) % 4) / 3.0                        # clearcoat
    t[:, 12] = ((k * 3) % 7) / 6.0                        # clearcoat_gloss
    return np.ascontiguousarray(t)


@pytest.mark.parametrize("scene,W,H,depth,spp,scene_seed", CASES)
def test_material_upload_between_accumulate_calls_reaches_the_next_launch(scene, W, H, depth, spp, scene_seed, monkeypatch):
    """A stale staged row, or a launch that overtakes the refresh of the derived table, shows as the old material here."""
    monkeypatch.setenv("VRT_RENDER", "pool")
    g, o = pair(scene, W, H, depth, seed=31, scene_seed=scene_seed)
    try:
        table = changed_table()
        for s in (g, o):
            s.accumulate(spp)
            s.upload_materials(table)
            s.accumulate(spp)
        assert_same_frames(g, o, f"{scene} after the upload")
        plain_g, plain_o = pair(scene, W, H, depth, seed=31, scene_seed=scene_seed)
        plain_o.accumulate(2 * spp)
        changed = not np.array_equal(plain_o.fetch_hdr().view(np.uint32), o.fetch_hdr().view(np.uint32))
        plain_g.close()
        plain_o.close()
        assert changed, "the changed table must change the picture, or the test shows nothing"
    finally:
        g.close()
        o.close()


def edge_scene():
    """A cube of 8^3 voxels of mixed materials on the grid's diagonal: its edges and corners can be met on exact ties."""
    mat = np.zeros((128, 128, 128), np.int8)
    rgb = np.zeros((128, 128, 128, 3), np.uint8)
    x, y, z = np.meshgrid(np.arange(60, 68), np.arange(60, 68), np.arange(60, 68), indexing="ij")
    mat[60:68, 60:68, 60:68] = (1 + (x + y + z) % 5).astype(np.int8)
    mat[mat == 2] = 6                                      # (2 is the emitter: a path that ends there shades nothing)
    rgb[60:68, 60:68, 60:68, 0] = (40 + 23 * (x - 60)).astype(np.uint8)
    rgb[60:68, 60:68, 60:68, 1] = (250 - 19 * (y - 60)).astype(np.uint8)
    rgb[60:68, 60:68, 60:68, 2] = (90 + 11 * (z - 60)).astype(np.uint8)
    return mat, rgb


def tie_rays():
    """Rays along the diagonals of the cube's edges and corners, from points symmetric to them (voxel units -> world: / 64 - 1)."""
    rays = []
    s2, s3 = np.float32(np.sqrt(0.5)), np.float32(np.sqrt(1.0 / 3.0))
    lo, hi = 60.0, 68.0
    for sx in (-1, 1):
        for sy in (-1, 1):
            cx, cy = (hi if sx > 0 else lo), (hi if sy > 0 else lo)
            for k in (2.0, 3.0, 5.5):
                for w in (60.5, 63.5, 67.5):
                    rays.append(((cx + sx * k, cy + sy * k, w), (-sx * s2, -sy * s2, 0.0)))      # an edge along z
                    rays.append(((cx + sx * k, w, cy + sy * k), (-sx * s2, 0.0, -sy * s2)))      # an edge along y
                    rays.append(((w, cx + sx * k, cy + sy * k), (0.0, -sx * s2, -sy * s2)))      # an edge along x
            for sz in (-1, 1):
                cz = hi if sz > 0 else lo
                for k in (2.0, 4.0):
                    rays.append(((cx + sx * k, cy + sy * k, cz + sz * k), (-sx * s3, -sy * s3, -sz * s3)))   # a corner
    out = np.zeros(len(rays), _abi.PATH_RAY)
    for i, (o, d) in enumerate(rays):
        out[i]["origin"] = (np.array(o, np.float64) / 64.0 - 1.0).astype(np.float32)
        out[i]["dir"] = np.array(d, np.float32)
        out[i]["stream"] = 1000 + i
    return out


def test_step_normals_taken_on_ties_go_through_the_guard():
    mat, rgb = edge_scene()
    _, _, params = scenes.SCENES["sunlit"](0)
    params = dict(params, use_physical_sky=0, use_clouds=0, floor_height=-0.5)
    cfg = host.make_config(16, 8, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=6, seed=41)
    g, e = NativeSession(_lib.load(), "vrt_", cfg), st.PackedRows(cfg)
    try:
        for s in (g, e):
            orc.setup(s, mat, rgb, params)
        rays = tie_rays()
        want, ties = st.trace_counting_ties(e, rays, 3, 7)
        assert int((ties > 0).sum()) >= 8, f"only {int((ties > 0).sum())} of {len(rays)} rays shade a vertex met on a tie"
        got = g.trace_radiance(rays, 3, 7)
        same = (got["rgb"].view(np.uint32) == want["rgb"].view(np.uint32)).all(axis=1) & (got["t"].view(np.uint32) == want["t"].view(np.uint32))
        assert same.all(), f"{(~same).sum()} of {len(rays)} records differ, {(~same & (ties > 0)).sum()} of them with a tie vertex"
        assert np.isfinite(got["rgb"]).all() and (got["rgb"][ties > 0] > 0).any()
    finally:
        g.close()
        e.close()
