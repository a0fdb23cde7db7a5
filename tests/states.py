"""Frame states for the scene queries: what a context can be in the middle of when vrt_cast_rays, vrt_trace_radiance or
vrt_gather_irradiance is asked -- ReSTIR, a moving camera, a render scale below 1, frames in flight with a deferred accumulation
pending, a row tile, row stripes, a reset, instrumented launches, reserved CUs -- and the device paths of the three queries.  Test
infrastructure of tests/test_gpu_query_states.py.

A state is (width, height, keyword arguments for the case's config(), apply(session)): apply runs after X.start / S.start has prepared
the scene and leaves the context in the state.  The queries' expected values are the existing ones and nothing else -- X.expected,
S.expected, tests/cast.py's records -- which come from the oracle on a context that has none of this state: a query promises to read
scene data only (include/vrt_api.h)."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np

import cast as K
import plan
import radiance as X
import sensor as S
from voxel_rt2_amd import _abi, _lib, camera as cam_mod, host
from voxel_rt2_amd._session import NativeSession

CASES = ("sunlit_d5", "dense_ref", "s1_256")     # light, voxel / floor / sky first hits, culling box; reference indexing: no culling; the other grid
SENSOR_SAMPLES = 3


def camera(pose, width, height, k=0, **kw):
    """tests/radiance.py's camera() with host.make_camera's other arguments: moving, render_scale."""
    pos, look, fov = X.POSES[pose]
    view, proj = cam_mod.default_matrices(width, height, pos=pos, look=look, fov=float(np.deg2rad(fov)))
    return host.make_camera(view, proj, pos, jitter_index=k, **kw)


def set_instrumented(s, mode):
    assert _lib.load().vrt_set_instrumented(C.c_void_p(s._ctx), int(mode)) == 0


def deferral():
    """Launches a pass accumulates together at 64 x 40 x 4 items on this machine's hardware queues, whichever kernel the scene takes."""
    queues = int(os.environ.get("GPU_MAX_HW_QUEUES", 4))
    return min(plan.shape(64 * 40 * 4, queues, heavy=heavy)[1] for heavy in (False, True))


# ---- the states -----------------------------------------------------------------------------------------------------------------
def _restir(s):
    s.accumulate(2)
    s.accumulate(2)                               # the second call's reservoir passes read what the first left


def _moving(s):
    s.set_camera(camera("street", s.W, s.H, 1, moving=True, max_accum_frames=50.0))
    s.accumulate(1)
    s.end_frame()
    s.set_camera(camera("courtyard", s.W, s.H, 2, moving=True, max_accum_frames=50.0))
    s.accumulate(1)                               # the queries run between the frames of a moving camera


def _scaled(s):
    s.set_camera(camera("default", s.W, s.H, 0, render_scale=0.3))
    s.accumulate(2)


def _big_frame(s):
    assert deferral() > 3, "launches of 64 x 40 x 4 items are not accumulated more than three at a time: nothing stays pending"
    s.set_camera(camera("default", s.W, s.H, 5))
    for _ in range(3):
        s.accumulate(4)                           # not fetched, not waited for: three launches and their one pass outstanding, frame = 12


def _big_frame_after(s):
    st = s.stats()                                # (looking forces the pass: only after the queries)
    assert st["pipeline_flags"] & 1 and st["render_launches"] == st["temporal_launches"] == 3, st


def _frames(n):
    def apply(s):
        s.accumulate(n)
    return apply


def _stripes(s):
    s.set_row_stripes(8, 2, 1)
    s.accumulate(2)


def _after_reset(s):
    s.accumulate(4)
    s.reset()


def _instrumented(s):
    set_instrumented(s, 1)                        # the render's culling rule and the queries' part ways here (plan_render_variant, query_inputs)
    s.accumulate(2)


def _reserved(s):
    s.reserve_cus(32)
    s.accumulate(2)


def _everything(s):
    """ReSTIR (config), 64 x 40, reserved CUs, instrumented, a moving camera at render scale 0.75, three frames queued and not waited for.
    What cannot be combined: a DEFERRED accumulation needs a static camera at scale 1 without ReSTIR (include/vrt_api.h, vrt_accumulate),
    so here every launch's pass is queued with it -- launches and passes are outstanding, none is pending in the library."""
    s.reserve_cus(32)
    set_instrumented(s, 1)
    for k, pose in enumerate(("street", "courtyard", "under_eaves")):
        s.set_camera(camera(pose, s.W, s.H, k + 1, moving=True, render_scale=0.75, max_accum_frames=50.0))
        s.accumulate(1)
        s.end_frame()


# name: (width, height, config keywords, apply, cases)
STATES = {
    "restir": (16, 8, dict(use_restir=True), _restir, CASES),
    "moving": (16, 8, {}, _moving, CASES),
    "scaled": (16, 8, {}, _scaled, CASES),
    "big_frame": (64, 40, {}, _big_frame, CASES),
    "tile": (64, 40, dict(rows=(13, 29)), _frames(2), CASES[:1]),         # a middle tile; static camera (a moving one needs the history exchange)
    "stripes": (64, 48, {}, _stripes, CASES[:1]),
    "after_reset": (16, 8, {}, _after_reset, CASES),
    "instrumented": (16, 8, {}, _instrumented, CASES),
    "reserved_cus": (16, 8, {}, _reserved, CASES[:1]),
    "everything": (64, 40, dict(use_restir=True), _everything, CASES),
}
AFTER = {"big_frame": _big_frame_after}
PAIRS = [(state, case) for state, (_, _, _, _, cases) in STATES.items() for case in cases]


def open_session(module, case, state):
    """A product session of `module`'s (tests/radiance.py or tests/sensor.py) case, prepared and put into the state."""
    w, h, kw, apply, _ = STATES[state]
    s = module.start(NativeSession(_lib.load(), "vrt_", module.config(case, w, h, **kw)), case)
    try:
        apply(s)
    except BaseException:
        s.close()
        raise
    return s


@contextlib.contextmanager
def stats_unchanged(s, on):
    """vrt_get_stats before == after, every field, if `on` (the instrumented state: its counters are live)."""
    before = s.stats() if on else None
    yield
    if on:
        after = s.stats()
        assert after == before, {k: (before[k], after[k]) for k in before if before[k] != after[k]}
        assert before["rays"] > 0                 # the counters were live


# ---- the device paths ----------------------------------------------------------------------------------------------------------
def _device(s, call, records, out_dtype, sync):
    """Tensors on the device, the work queued on the context's stream by call(t_in, t_out), read back after a sync."""
    import torch
    t_in = torch.from_numpy(np.array(records).view(np.uint8).reshape(-1)).cuda()   # (a copy: the shared records are read-only)
    t_out = torch.full((len(records) * out_dtype.itemsize,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                      # the tensors are written on torch's stream, read on the context's
    call(t_in, t_out)
    if not sync:
        return t_in, t_out
    s.sync()
    return t_out.cpu().numpy().view(out_dtype)


def device_cast(s, rays, sync=True):
    return _device(s, lambda i, o: s.cast_rays(i, o), rays, _abi.HIT, sync)


def device_trace(s, rays, samples, first_frame=X.FIRST_FRAME, sync=True):
    return _device(s, lambda i, o: s.trace_radiance(i, samples, first_frame, o), rays, _abi.RADIANCE, sync)


def device_gather(s, sensors, samples, first_frame=S.FIRST_FRAME, sync=True):
    return _device(s, lambda i, o: s.gather_irradiance(i, samples, first_frame, o), sensors, _abi.IRRADIANCE, sync)


def read_back(kept, dtype):
    """The records of a (t_in, t_out) pair device_*(sync=False) returned, after the session's sync."""
    return kept[1].cpu().numpy().view(dtype)


def device_query(s):
    """`query` of S.expected: vrt_trace_radiance on the same context, host path."""
    return lambda rays, frame: s.trace_radiance(rays, 1, frame)["rgb"]


# ---- what the queries must answer ----------------------------------------------------------------------------------------------
def radiance_batch(case):
    """(rays of every pose, the oracle's records, one pose's rays and records) at the case's largest sample count."""
    want = X.expected(case)
    n = max(X.SAMPLES[case])
    rays = np.concatenate([want[p][0] for p in want])
    rec = np.concatenate([want[p][1][n] for p in want])
    pose = "street" if "street" in want else next(iter(want))
    return n, rays, rec, want[pose][0], want[pose][1][n]


REF_FAMILIES = ("random", "planes", "axis")       # tests/test_cast_rays_host.py's choice for the reference's indexing


@functools.lru_cache(maxsize=None)
def cast_records(scene, reference_indexing=False):
    """[(label, rays, the oracle's records)] of the cast tests' ray families on `scene`.  With the reference's indexing the oracle is
    asked in that mode (tests/test_cast_rays_host.py: test_row_function_with_reference_indexing), on the families it takes there.
    Computed once and left alone."""
    if not reference_indexing:
        return tuple((f"{scene}/{fam}",) + K.family(scene, fam)[:2] for fam in K.families_of(scene))
    full, _ = K.oracles(scene)
    rays = np.concatenate([K.family(scene, f)[0] for f in REF_FAMILIES])
    full._lib.orc_set_reference_indexing(C.c_void_p(full._ctx), 1)
    try:
        want_inf, _ = K.expected_inf(scene, rays)
        _, want = K.with_t_max(rays, want_inf, rays["t_max"])
    finally:
        full._lib.orc_set_reference_indexing(C.c_void_p(full._ctx), 0)
    for a in (rays, want):
        a.setflags(write=False)
    return ((f"{scene}/reference indexing", rays, want),)


def cast_records_of(case):
    """cast_records for the scene of a case of tests/radiance.py (whose parameters are the cast scene's: no overrides of what a cast reads)."""
    name, _, over, ref, _ = X.CASES[case]
    assert not set(over) & {"floor_height", "floor_color", "floor_material", "voxel_edges"}
    return cast_records(name, ref)


def check_radiance(s, case, label, staged=False):
    """All poses' rays in one device-path batch (tiled up to the staged view if `staged`), one pose on the host path."""
    n, rays, rec, pose_rays, pose_rec = radiance_batch(case)
    if staged:
        k = 1
        while not X.lib().radiance_emul_staged(k * len(rays) * n, -1):
            k += 1
        rays, rec = np.tile(rays, k), np.tile(rec, k)
    assert len(X.chunks(len(rays), n)) == 1
    X.check(device_trace(s, rays, n), rays, rec, f"{label}: radiance, {len(rays)} rays x {n} samples, device path")
    X.check(s.trace_radiance(pose_rays, n, X.FIRST_FRAME), pose_rays, pose_rec, f"{label}: radiance, one pose, host path")


def check_cast(s, case, label):
    for name, rays, want in cast_records_of(case):
        K.check(s.cast_rays(rays), rays, want, f"{label}: cast {name}, host path")
        K.check(device_cast(s, rays), rays, want, f"{label}: cast {name}, device path")


def check_sensors(s, case, label):
    sensors = S.sensors_of(case)
    want = S.expected(case, SENSOR_SAMPLES, device_query(s))
    S.check(device_gather(s, sensors, SENSOR_SAMPLES), sensors, want, f"{label}: sensors x {SENSOR_SAMPLES} samples, device path")
