"""Whole frames from a matrix of camera poses: the poses, the oracle's frames (rendered once per case and left alone) and the
comparison.  Test infrastructure shared by tests/test_poses.py (the host build of the device code, no GPU) and
tests/test_gpu_poses.py.

One context per scene and schedule goes from pose to pose with set_camera + reset: a large camera change inside a live context.
Every frame is compared with the oracle's bit for bit: HDR, LDR and the seven buffers of test_hdr_matches_oracle."""
import functools

import numpy as np

import orc
import plan
from voxel_rt2_amd import _abi, camera, host, scenes

BUFS = (_abi.BUF_GBUF_DEPTH, _abi.BUF_GBUF_NORMAL, _abi.BUF_GBUF_POSITION, _abi.BUF_GBUF_MAT, _abi.BUF_GBUF_REFL_DEPTH,
        _abi.BUF_HISTORY_DIFFUSE, _abi.BUF_HISTORY_SPECULAR)
V = 1.0 / 64.0
DEPTH, SPP = 4, 2
# name: (position, looks at, vertical field of view in degrees); world units.  Written for `sunlit`: blocks of 6x6 voxels every 9,
# 3..11 voxels high on the floor y = -10 V, under a grown box of 66 x 28 x 48 voxels.
POSES = {
    "default": (camera.DEFAULT_POS, (0.0, 0.0, 0.0), 50.0),
    "gap": ((-2.5 * V, -5.5 * V, -1.5 * V), (0.4, -0.05, 0.3), 50.0),            # in a gap between blocks
    "in_block": ((2.5 * V, -5.5 * V, 2.5 * V), (0.4, 0.1, 0.3), 50.0),           # inside a solid block
    "in_grid": ((0.2, 0.8, 0.3), (0.0, 0.0, 0.0), 50.0),                         # inside the grid, outside the grown box
    "away": ((0.2, 0.8, 0.3), (0.3, 2.0, 0.5), 50.0),                            # same position, looking away: every camera ray is culled
    "below_floor": ((0.3, -0.6, 0.5), (0.0, 0.0, 0.0), 50.0),
    "opposite": ((-1.6, 0.7, -1.7), (0.0, 0.0, 0.0), 50.0),                      # the opposite octant: other entry faces
    "top_down": ((0.01, 2.5, 0.02), (0.0, 0.0, 0.0), 50.0),
    "grazing": ((0.0, -10.0 * V + 0.001, 1.5), (0.0, -10.0 * V + 0.001, 0.5), 50.0),   # along the floor, horizontally towards -z
    "on_axis": ((0.0, 0.0, 2.0), (0.0, 0.0, 0.0), 50.0),
    "far_narrow": ((3.0, 4.0, 9.0), (0.0, 0.0, 0.0), 5.0),
    "on_face": ((0.3, 0.2, 1.0), (0.0, 0.0, 0.0), 50.0),                         # on the grid's +z face
    "on_corner": ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), 50.0),
    "wide": ((0.5, 0.3, 0.9), (0.0, 0.0, 0.0), 120.0),
}
ALL = tuple(POSES)
SIX = ("default", "in_block", "away", "opposite", "on_corner", "wide")            # the reduced set of the 256^3 scene
RESTIR = ("default", "gap", "opposite")
BLACK_BY_NATURE = ("in_block", "away")
# (scene, width, height, ReSTIR, poses)
CASES = [
    ("sunlit", 64, 40, False, ALL),
    ("sunlit", 100, 60, False, ALL),        # ragged: not a multiple of the 8x8 tile
    ("s1", 64, 40, False, ALL),
    ("dense", 64, 40, False, ALL),          # the camera is inside the filled grid for half the poses; the dense kernel variant
    ("s1_256", 64, 40, False, SIX),
    ("sunlit", 64, 40, True, RESTIR),
]
IDS = [f"{s}-{w}x{h}{'-restir' if r else ''}" for s, w, h, r, _ in CASES]


@functools.lru_cache(maxsize=None)
def scene(name):
    return scenes.SCENES[name](0)


def config(name, W, H, restir=False):
    mat, _, params = scene(name)
    return host.make_config(W, H, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=DEPTH, seed=23,
                            use_restir=restir, grid_res=mat.shape[0])


def cam(W, H, pose, jitter_index=0, **kw):
    pos, look, fov = POSES[pose]
    view, proj = camera.default_matrices(W, H, pos=pos, look=look, fov=float(np.deg2rad(fov)))
    return host.make_camera(view, proj, pos, jitter_index=jitter_index, **kw)


def start(session, name):
    mat, rgb, params = scene(name)
    orc.setup(session, mat, rgb, params)
    return session


def snapshot(s):
    out = {"hdr": s.fetch_hdr(), "ldr": s.fetch_ldr()}
    for which in BUFS:
        out[which] = s.fetch_buffer(which)
    return out


def run_matrix(session, W, H, poses):
    """pose -> every buffer after SPP samples from that pose, the context carried from pose to pose."""
    frames = {}
    for k, pose in enumerate(poses):
        session.set_camera(cam(W, H, pose, jitter_index=k))
        session.reset()
        session.accumulate(SPP)
        frames[pose] = snapshot(session)
    return frames


@functools.lru_cache(maxsize=None)
def oracle_matrix(case):
    name, W, H, restir, poses = CASES[case]
    o = start(orc.Oracle(config(name, W, H, restir), threads=8), name)
    frames = run_matrix(o, W, H, poses)
    o.close()
    for f in frames.values():
        for a in f.values():
            a.setflags(write=False)
    return frames


def assert_frames_equal(got, want, label):
    for key in want:
        a, b = np.ascontiguousarray(got[key]), want[key]
        same = (a.view(np.uint8) == b.view(np.uint8)).reshape(a.shape[0], a.shape[1], -1).all(-1)
        assert same.all(), f"{label}: {key if isinstance(key, str) else 'buffer %d' % key} differs at {int((~same).sum())} of {same.size} pixels, first (v, u) {np.argwhere(~same)[:4].tolist()}"


def check_matrix(session_of, case):
    name, W, H, restir, poses = CASES[case]
    want = oracle_matrix(case)
    s = start(session_of(config(name, W, H, restir)), name)
    got = run_matrix(s, W, H, poses)
    s.close()
    for pose in poses:
        assert_frames_equal(got[pose], want[pose], f"{IDS[case]} pose {pose}")


def check_guards(report=print):
    """The oracle's frames alone: the sunlit poses show the scene (so a comparison of black frames cannot pass for coverage).
    And the `dense` cases take the twelve-wave dense kernel under the pooled schedule: the inputs (vrt_prepare: at least half of the
    4x4x4 bricks hold a voxel; ReSTIR off and a sun that emits), and the choice the library's own plan_render_variant (vrt_plan.h,
    compiled for the host) makes on them."""
    mat, _, params = scene("dense")
    G = mat.shape[0]
    dense = (mat > 0).reshape(G // 4, 4, G // 4, 4, G // 4, 4).any(axis=(1, 3, 5)).mean() >= 0.5
    sp = host.make_scene_params(**params)   # what the sessions are given (orc.setup)
    emits = any(c != 0 for c in sp.light_color) and sp.light_weight != 0
    assert dense and any(c != 0 for c in params["light_color"])
    assert not any(restir for name, _, _, restir, _ in CASES if name == "dense")
    for name, W, H, restir, _ in CASES:
        if name == "dense":
            v = plan.variant(width=W, height=H, max_depth=DEPTH, use_restir=restir, dense_grid=dense, light_emits=emits, fused=SPP)
            assert "dense12" in v and "pooled" in v, v
    for case, (name, W, H, restir, poses) in enumerate(CASES):
        if name != "sunlit":
            continue
        for pose, f in oracle_matrix(case).items():
            lit = float((f["hdr"] > 0).any(-1).mean())
            depths = len(np.unique(f[_abi.BUF_GBUF_DEPTH]))
            report(f"poses {IDS[case]:22s} {pose:12s} non-black {100 * lit:5.1f} %  distinct depths {depths}")
            if pose not in BLACK_BY_NATURE:
                assert lit > 0.9 and depths > 20, (IDS[case], pose, lit, depths)


# ---- render_scale below 1 ---------------------------------------------------------------------------------------------------------
# (width, height, steps); a step = (pose, moving, render_scale)
SCALED = [
    (64, 40, (("default", False, 0.75), ("default", False, 0.75), ("opposite", True, 0.75), ("opposite", True, 0.75))),
    (100, 60, (("default", False, 1.0), ("wide", True, 0.3), ("wide", True, 0.3))),   # 100 * 0.3 and 60 * 0.3 are not whole numbers
]


def run_scaled(session, W, H, steps):
    """A static camera at a render scale below 1, then a hop to a distant pose with the moving camera (the sequence of
    test_moving_camera_sequence: end_frame after every step, reset at the first moving step).  Returns the buffers after each step."""
    frames, was_moving = [], False
    for k, (pose, moving, scale) in enumerate(steps):
        session.set_camera(cam(W, H, pose, jitter_index=k, moving=moving, render_scale=scale, max_accum_frames=50.0 if moving else 999999999.0))
        if moving and not was_moving:
            session.reset()
        was_moving = moving
        session.accumulate(1)
        session.end_frame()
        frames.append(snapshot(session))
    return frames


@functools.lru_cache(maxsize=None)
def oracle_scaled(case):
    W, H, steps = SCALED[case]
    o = start(orc.Oracle(config("sunlit", W, H), threads=8), "sunlit")
    frames = run_scaled(o, W, H, steps)
    o.close()
    return frames


def check_scaled(session_of, case):
    W, H, steps = SCALED[case]
    want = oracle_scaled(case)
    s = start(session_of(config("sunlit", W, H)), "sunlit")
    got = run_scaled(s, W, H, steps)
    s.close()
    for k, step in enumerate(steps):
        assert_frames_equal(got[k], want[k], f"{W}x{H} step {k} {step}")
    assert (want[-1]["hdr"] > 0).any(-1).mean() > 0.5
