"""The three scene queries ON THE DEVICE on contexts in every frame state, bit for bit against the oracle on a context that has no
such state: vrt_cast_rays, vrt_trace_radiance and vrt_gather_irradiance promise to read scene data only (include/vrt_api.h), so a
query's answer must not notice ReSTIR, a moving camera, a render scale below 1, frames in flight, a pending deferred accumulation, a
row tile, row stripes, a reset, instrumented launches or reserved CUs (tests/states.py holds the states; tests/radiance.py,
tests/sensor.py and tests/cast.py the expected values and the comparisons: floats by their bits, no row left out).
  - every state x {sunlit_d5, dense_ref, s1_256} (tile, stripes, reserved_cus: sunlit_d5): radiance for every pose in one device-path
    batch and one pose on the host path, the sensors at 3 samples, the cast tests' ray families on both paths;
  - the scene changing between queries without a new vrt_prepare: vrt_set_scene (light, background, floor height) and
    vrt_set_reference_indexing off -> on -> off -- a query follows, one queued before keeps the old answer;
  - the device results the frame-independence tests of the three query suites compute and drop, compared with the oracle's;
  - the query side against the render side: Renderer.pick_ray at render scales 0.75 and 0.3 against the oracle's cast direction, and
    Renderer.pick against the g-buffer of the frame the pixel sits in, before and after an edit."""
import numpy as np
import pytest

import cast as K
import orc
import radiance as X
import sensor as S
import states as T
from voxel_rt2_amd import _abi, _lib, host
from voxel_rt2_amd._session import NativeSession

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("state,case", T.PAIRS)
def test_queries_do_not_notice_the_frame_state(state, case):
    """A context of the case put into the state (tests/states.py), then asked: every record equals the oracle's, which never saw the
    state.  Radiance and casts on tests/radiance.py's scene of the case, sensors on tests/sensor.py's (the fixtures), each on a context
    of its own in the same state; the sensors' `query` is vrt_trace_radiance on that same stated context.  `instrumented` also has
    vrt_get_stats unchanged across the queries; `big_frame` finds, after them, that the three launches' pass was the pending one."""
    label = f"{state}/{case}"
    s = T.open_session(X, case, state)
    try:
        with T.stats_unchanged(s, state == "instrumented"):
            T.check_radiance(s, case, label, staged=state == "everything")
            T.check_cast(s, case, label)
        if state in T.AFTER:
            T.AFTER[state](s)
    finally:
        s.close()
    s = T.open_session(S, case, state)
    try:
        with T.stats_unchanged(s, state == "instrumented"):
            T.check_sensors(s, case, label)
        if state in T.AFTER:
            T.AFTER[state](s)
    finally:
        s.close()


def test_queries_follow_set_scene_without_a_new_prepare():
    """vrt_set_scene after vrt_prepare on sunlit at depth 2 (plain background, no physical sky: its tables would depend on the sun):
    another light direction, colour and cone, another background, the floor one voxel lower.  Radiance and sensors equal the
    oracle's expectation for the NEW parameters (case sunlit_d2_relit: an oracle context set up with them from the start); queries
    queued on the device path before the change keep the old answers."""
    old, new = "sunlit_d2", "sunlit_d2_relit"
    n, rays, rec_old, _, _ = T.radiance_batch(old)
    n_new, rays_new, rec_new, _, _ = T.radiance_batch(new)
    assert n == n_new and rays.tobytes() == rays_new.tobytes()                           # the same camera rays, other answers
    lit = (rec_old["rgb"] > 0).any(axis=1)
    assert X.mismatches(rec_old, rec_new).size > lit.sum() // 2 and (rec_old["t"] != rec_new["t"]).any()   # colours and, by the floor, distances
    floor_rays, floor_old, _ = K.family("sunlit", "floor")
    params = dict(X.scene(new)[2])
    s = X.start(NativeSession(_lib.load(), "vrt_", X.config(old)), old)
    try:
        before = T.device_trace(s, rays, n, sync=False)
        cast_before = T.device_cast(s, floor_rays, sync=False)
        s.set_scene(host.make_scene_params(**params))
        T.check_radiance(s, new, "after vrt_set_scene")
        assert K.mismatches(s.cast_rays(floor_rays), floor_old).size > 100               # the floor moved under the casts too (radiance's t has the oracle's)
        X.check(T.read_back(before, _abi.RADIANCE), rays, rec_old, "queued before vrt_set_scene: radiance")
        K.check(T.read_back(cast_before, _abi.HIT), floor_rays, floor_old, "queued before vrt_set_scene: cast sunlit/floor")
    finally:
        s.close()
    sensors_old, sensors_new = S.sensors_of(old), S.sensors_of(new)
    s = S.start(NativeSession(_lib.load(), "vrt_", S.config(old)), old)
    try:
        want_old = S.expected(old, T.SENSOR_SAMPLES, T.device_query(s))                 # (its hemisphere rays are asked now, in the old state)
        before = T.device_gather(s, sensors_old, T.SENSOR_SAMPLES, sync=False)
        s.set_scene(host.make_scene_params(**params))
        T.check_sensors(s, new, "after vrt_set_scene")
        host_ok = sensors_new["reserved"] == 0
        want_new = S.expected(new, T.SENSOR_SAMPLES, T.device_query(s))
        S.check(s.gather_irradiance(sensors_new[host_ok], T.SENSOR_SAMPLES, S.FIRST_FRAME), sensors_new[host_ok], want_new[host_ok], "after vrt_set_scene: host path")
        S.check(T.read_back(before, _abi.IRRADIANCE), sensors_old, want_old, "queued before vrt_set_scene: sensors")
        # the same sensors under both lights: the sun term moved
        assert S.mismatches(s.gather_irradiance(sensors_old[sensors_old["reserved"] == 0], T.SENSOR_SAMPLES, S.FIRST_FRAME), want_old[sensors_old["reserved"] == 0]).size > 50
    finally:
        s.close()


def test_queries_follow_reference_indexing_toggled_on_a_live_context():
    """vrt_set_reference_indexing off -> on -> off on `dense` after vrt_prepare, queries in between: dense / dense_ref / dense in turn,
    for all three queries -- the reading of cells outside the grid AND the culling box (off with the reference's indexing) follow
    the switch.  (How many records tell the modes apart is printed by the host tests; here each mode has its own oracle records.)"""
    s = X.start(NativeSession(_lib.load(), "vrt_", X.config("dense")), "dense")
    try:
        for step, (on, case) in enumerate(((False, "dense"), (True, "dense_ref"), (False, "dense"))):
            if step:
                s.set_reference_indexing(on)
            T.check_radiance(s, case, f"step {step}: reference indexing {on}")
            T.check_cast(s, case, f"step {step}: reference indexing {on}")
    finally:
        s.close()
    s = S.start(NativeSession(_lib.load(), "vrt_", S.config("dense")), "dense")
    try:
        for step, (on, case) in enumerate(((False, "dense"), (True, "dense_ref"), (False, "dense"))):
            if step:
                s.set_reference_indexing(on)
            assert S.sensors_of(case).tobytes() == S.sensors_of("dense").tobytes()
            T.check_sensors(s, case, f"step {step}: reference indexing {on}")
    finally:
        s.close()


def test_results_of_queries_interleaved_with_frames_equal_the_oracle():
    """The interleaving of the three suites' frames-do-not-notice tests, once, with sunlit_d5: accumulate(4) x 3 at 64 x 40 under the
    overlapped pipeline, device-path queries queued after every call and kept -- and here compared with the oracle's records once the
    context is waited for.  Every query of the sequence finds a deferred accumulation pending (tests/states.py: deferral())."""
    case = "sunlit_d5"
    assert T.deferral() > 3
    n, rays, rec, _, _ = T.radiance_batch(case)
    casts = T.cast_records_of(case)
    s = X.start(NativeSession(_lib.load(), "vrt_", X.config(case, 64, 40)), case)
    try:
        kept = []
        for k in range(3):
            s.accumulate(4)
            kept.append((T.device_trace(s, rays, n, sync=False), [T.device_cast(s, r, sync=False) for _, r, _ in casts]))
        s.sync()
        for k, (traced, cast) in enumerate(kept):
            X.check(T.read_back(traced, _abi.RADIANCE), rays, rec, f"radiance queued after launch {k}")
            for (name, r, want), got in zip(casts, cast):
                K.check(T.read_back(got, _abi.HIT), r, want, f"cast {name} queued after launch {k}")
        T.AFTER["big_frame"](s)
    finally:
        s.close()
    sensors = S.sensors_of(case)
    s = S.start(NativeSession(_lib.load(), "vrt_", S.config(case, 64, 40)), case)
    try:
        kept = []
        for k in range(3):
            s.accumulate(4)
            kept.append(T.device_gather(s, sensors, T.SENSOR_SAMPLES, sync=False))
        want = S.expected(case, T.SENSOR_SAMPLES, T.device_query(s))                    # (host-path queries: they force no pass either)
        s.sync()
        for k, got in enumerate(kept):
            S.check(T.read_back(got, _abi.IRRADIANCE), sensors, want, f"sensors queued after launch {k}")
        T.AFTER["big_frame"](s)
    finally:
        s.close()


# ---- the query side against the render side ---------------------------------------------------------------------------------------
def renderer(w=32, h=16):
    """The content of the query suites' renderer() helpers: a field of voxels of material 11 over a floor, a sun, a plain background."""
    from voxel_rt2_amd.renderer import Renderer
    r = Renderer(dx=1 / 64, image_res=(w, h), up=(0, 1, 0), voxel_edges=0.06, exposure=1.5, max_depth=2, seed=7, sky_res=0)
    r.floor_height[None] = -0.3
    r.set_directional_light((0.3, 1.0, 0.2), 0.1, (1.0, 0.9, 0.8))
    r.background_color[None] = (0.2, 0.3, 0.5)
    for x in range(-20, 21):
        for z in range(-20, 21):
            r.set_voxel((x, -3 + (x * z) % 3, z), 11, (0.8, 0.3, 0.2))
    return r


@pytest.mark.parametrize("scale", [0.75, 0.3])
def test_pick_ray_equals_the_oracles_cast_direction_at_a_render_scale(scale):
    """Every pixel of a 32 x 16 camera at render scale 0.75 and 0.3 against orc_unit_cast_dir on an oracle camera with the same scale
    and camera_is_moving = 1 (no jitter): bit equality.  (tests/test_gpu_cast_rays.py covers scale 1.)"""
    from voxel_rt2_amd import camera as cam_mod
    r = renderer()
    pos = (0.7, 0.9, 1.6)
    r.set_camera_pos(*pos)
    view, proj = cam_mod.default_matrices(32, 16, pos=pos, look=(0.1, -0.2, 0.0), fov=float(np.deg2rad(38.0)))
    r.set_view_mat(cam_mod.to_glm_memory(view))
    r.set_proj_mat(cam_mod.to_glm_memory(proj))
    r.set_render_scale(scale)
    o = orc.Oracle(host.make_config(32, 16, max_depth=2, seed=7), threads=1)
    try:
        o.set_camera(host.make_camera(view, proj, pos, jitter_index=1, moving=True, render_scale=scale))
        for v in range(16):
            for u in range(32):
                origin, d = r.pick_ray(u, v)
                want = o.cast_dir(u, v)
                assert d.tobytes() == want.tobytes(), f"scale {scale} pixel ({u}, {v}): {d} != {want}"
                assert origin.tolist() == np.array(pos, np.float32).tolist()
    finally:
        o.close()
        r.session.close()


def check_pick_against_gbuffer(r, label):
    """Row order: vrt_fetch_buffer returns [H][W] arrays whose row index is the pixel's v -- the render kernels store pixel (u, v) at
    (v - row0) * W + u (path_shade, vrt_path.h; fetch_rows, vrt_api.hip) -- and v = 0 is the bottom row, which is also pick's v
    (Renderer.pick_ray: "v = 0 at the bottom").  So buffer[v, u] is pick(u, v), with no flip.
    The rule checked, for every pixel: pick misses exactly where the stored position is (0, 0, 0) -- what a primary ray into the sky
    stores (pathtracer.py:510) -- and there the material word's low byte is 0; everywhere else the low byte is pick's mat_id.
    Positions and depths are not compared: they are formed by different expressions."""
    W, H = r.image_res
    mat = r.session.fetch_buffer(_abi.BUF_GBUF_MAT)[..., 0]
    pos = r.session.fetch_buffer(_abi.BUF_GBUF_POSITION)
    assert mat.shape == (H, W) and pos.shape == (H, W, 3)
    kinds, ids = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
    for v in range(H):
        for u in range(W):
            hit = r.pick(u, v)
            kinds[v, u], ids[v, u] = hit["kind"], hit["mat_id"]
    sky = (pos == 0).all(axis=2)
    assert ((kinds == _abi.HIT_MISS) == sky).all(), f"{label}: pick misses and sky pixels differ at {np.argwhere((kinds == _abi.HIT_MISS) != sky)[:4].tolist()} (v, u)"
    low = (mat & 0xFF).astype(np.int32)
    assert (low[sky] == 0).all(), label
    assert (low == ids).all(), f"{label}: the g-buffer's material and pick's differ at {np.argwhere(low != ids)[:4].tolist()} (v, u)"
    assert {_abi.HIT_MISS, _abi.HIT_FLOOR, _abi.HIT_VOXEL} == set(np.unique(kinds).tolist()), label   # no comparison passes on one kind alone
    return kinds, ids


def test_pick_agrees_with_the_g_buffer_of_the_frame():
    """A moving camera (no jitter: the frame's camera rays are pick_ray's) at render scale 1, one frame at 32 x 16: the g-buffer's
    material and sky pixels against pick, pixel by pixel; again after one edit in view, sent with update_voxels and the reset the
    facade makes."""
    r = renderer()
    try:
        r.set_camera_is_moving(True)
        r.prepare_data()
        r.accumulate(1)
        kinds, ids = check_pick_against_gbuffer(r, "first frame")
        assert set(np.unique(ids[kinds == _abi.HIT_VOXEL]).tolist()) == {11} and set(np.unique(ids[kinds == _abi.HIT_FLOOR]).tolist()) == {1}
        hit = r.pick(16, 7)
        assert hit["kind"] == _abi.HIT_VOXEL and hit["normal"].tolist() == [0.0, 0.0, 1.0]   # the field's +z side faces the camera
        cell = hit["cell"] - 64
        for dx in range(-8, 9):                                                          # a wall in front of what the centre pixel sees: a few pixels of it
            for dy in range(1, 17):
                r.set_voxel((int(cell[0]) + dx, int(cell[1]) + dy, int(cell[2]) + 1), 21, (0.1, 0.9, 0.3))
        r.update_voxels()                                                                # (reset=True: the facade resets the accumulation)
        r.accumulate(1)
        kinds2, ids2 = check_pick_against_gbuffer(r, "after the edit")
        assert (ids2 == 21).any() and (ids2 != ids).any() and not (ids == 21).any()
    finally:
        r.session.close()
