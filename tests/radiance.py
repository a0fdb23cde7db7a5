"""vrt_trace_radiance: cases, the oracle's values and the host build of the per-item functions (voxel_rt2_amd/csrc/vrt_radiance.h through
tests/emul/radiance_emul.cpp).  Test infrastructure shared by tests/test_radiance_host.py (no GPU) and tests/test_gpu_radiance.py.
Everything is compared bit for bit, any NaN equal to any NaN (mismatches()); no tolerance, no row left out.

Expected values come from the oracle alone (tests/emul/radiance_orc.cpp: the oracle's sources, unchanged, and one function over its public
render_pixel).  A case is a scene with settings; its rays are the camera rays of an oracle context of 16 x 8 pixels at each pose:
(camera_pos, orc_unit_cast_dir(u, v)) bit for bit, stream = v * W + u.  rgb: samples s = 0 .. n - 1 of pixel (u, v) rendered with
current_frame = first_frame + s, scrubbed, added, summed in order, divided by n.  t: orc_unit_next_hit on the same ray."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import cast as K
import edit as E
import orc
import poses as P
import rays as R
from voxel_rt2_amd import _abi, host, materials, scenes
from voxel_rt2_amd._session import NativeSession

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PATH_RAY, RADIANCE = _abi.PATH_RAY, _abi.RADIANCE
W, H = 16, 8
SEED = 23
FIRST_FRAME = 5
V = P.V
# tests/poses.py's, and three more with the camera inside the grid and below the top of `sunlit`'s blocks (3 .. 11 voxels on y = -10 V)
POSES = dict(P.POSES)
POSES.update({
    "street": ((-11.5 * V, -7.5 * V, 16.5 * V), (0.5, -0.12, -0.4), 70.0),        # down a gap, along the floor, blocks on both sides
    "courtyard": ((6.5 * V, -8.5 * V, -20.5 * V), (-0.3, -0.1, 0.4), 90.0),       # between four blocks, looking across the field
    "under_eaves": ((15.5 * V, -6.5 * V, 7.5 * V), (0.0, 0.6, 0.0), 100.0),       # low in a gap, looking up past the block tops
})
ALL = tuple(POSES)
SIX = P.SIX + ("street",)
# name: (scene, max_depth, scene-parameter overrides, reference indexing, poses)
# `sunlit_d2_relit`: sunlit_d2 under another light (direction, colour, cone), background and floor height -- what vrt_set_scene can change
# behind a prepared scene without a new vrt_prepare (tests/test_gpu_query_states.py); the floor one voxel lower, the blocks hover above it
RELIT = dict(light_direction=(0.4, 1.0, -0.7), light_color=(0.9, 0.7, 0.4), light_cone=0.3, background_color=(0.5, 0.2, 0.1), floor_height=-11.0 * V)
CASES = {f"sunlit_d{d}": ("sunlit", d, {}, False, ALL) for d in (1, 2, 5, 8)}
CASES.update({
    "sunlit_d2_relit": ("sunlit", 2, RELIT, False, ALL),
    "s1_black_sun": ("s1", 8, dict(light_color=(0.0, 0.0, 0.0)), False, ALL),
    "dense": ("dense", 4, {}, False, ALL),
    "dense_ref": ("dense", 4, {}, True, ALL),
    "s1_256": ("s1_256", 4, {}, False, SIX),
    "empty": ("empty", 4, {}, False, SIX),
    "sky": ("sunlit", 4, dict(use_physical_sky=1, use_clouds=0), False, SIX),
    "one_voxel_d2": ("one_voxel", 2, {}, False, ("default",)),                       # tests/test_gpu_radiance.py: chunks on the device
})
SAMPLES = {name: ((1, 3, 4) if name.startswith("sunlit_d") else (2,)) for name in CASES}
SKY_RES = 64


def scene(case):
    name, _, over, _, _ = CASES[case]
    mat, rgb, params = K.scene(name)
    return mat, rgb, dict(params, **over)


def config(case, width=W, height=H, **kw):
    name, depth, _, _, _ = CASES[case]
    mat, _, params = scene(case)
    return host.make_config(width, height, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=depth, seed=SEED,
                            sky_res=SKY_RES if params.get("use_physical_sky") else 0, grid_res=mat.shape[0], **kw)


def camera(pose, k=0, width=W, height=H):
    pos, look, fov = POSES[pose]
    view, proj = P.camera.default_matrices(width, height, pos=pos, look=look, fov=float(np.deg2rad(fov)))
    return host.make_camera(view, proj, pos, jitter_index=k)


# ---- the oracle with the shim ---------------------------------------------------------------------------------------------------
_SHIM = os.path.join(HERE, "emul", "_radiance_orc.so")
_EMUL = os.path.join(HERE, "emul", "_radiance_emul.so")
_libs = {}
_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-shared", "-Wall", "-Wno-unused-function",
          "-Wno-unknown-pragmas", "-Wno-misleading-indentation"]


def _build(so, src, dep_dirs, extra=()):
    deps = [src] + [os.path.join(d, f) for d in dep_dirs for f in os.listdir(d) if f.endswith((".h", ".cpp"))]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.run(["g++"] + _FLAGS + list(extra) + ["-o", so, src], check=True, capture_output=True)
    return so


def shim():
    """The oracle's library with orc_radiance_pixels added: the oracle's own build flags (oracle/Makefile)."""
    if "shim" not in _libs:
        so = _build(_SHIM, os.path.join(HERE, "emul", "radiance_orc.cpp"), [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "include")],
                    ["-fno-unsafe-math-optimizations", "-pthread"])
        lib = C.CDLL(so)
        lib.orc_radiance_pixels.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]
        _libs["shim"] = lib
    return _libs["shim"]


class ShimOracle(orc.Oracle):
    """orc.Oracle on the shim's library: the same orc_* entry points from the same sources, and radiance()."""

    def __init__(self, cfg, threads=1):
        NativeSession.__init__(self, shim(), "orc_", cfg, create_extra=(C.c_int(threads),))
        self.threads = threads

    def radiance(self, uv, n_samples, first_frame):
        uv = np.ascontiguousarray(uv, np.int32).reshape(-1, 2)
        out = np.zeros((len(uv), 3), np.float32)
        rc = self._lib.orc_radiance_pixels(C.c_void_p(self._ctx), len(uv), orc.fptr(uv), int(n_samples), int(first_frame) & 0xFFFFFFFF, orc.fptr(out))
        assert rc == 0, "the oracle context is not one the shim evaluates (ReSTIR off, static camera, render scale 1)"
        return out


@functools.lru_cache(maxsize=None)
def sky_tables():
    """The oracle's own precompute for the sky case (clouds off), once."""
    case = "sky"
    mat, rgb, params = scene(case)
    o = orc.Oracle(config(case), threads=8)
    orc.setup(o, mat, rgb, params, cloud=np.zeros((256, 256, 3), np.uint8))
    for sl in range(4):
        o.sky_compute_slice(sl, 4)
    scat, trans = o.fetch_buffer(_abi.BUF_SKY_SCATTERING), o.fetch_buffer(_abi.BUF_SKY_TRANSMITTANCE)
    o.close()
    assert np.isfinite(scat).all() and scat.max() > 0
    return scat, trans


def start(session, case):
    """Drive a session (oracle or product) to a prepared scene of the case; the sky tables are the oracle's."""
    mat, rgb, params = scene(case)
    sky = bool(params.get("use_physical_sky"))
    orc.setup(session, mat, rgb, params, cloud=np.zeros((256, 256, 3), np.uint8) if sky else None)
    if CASES[case][3]:
        if hasattr(session, "set_reference_indexing") and session._p == "vrt_":
            session.set_reference_indexing(True)
        else:
            session._lib.orc_set_reference_indexing(C.c_void_p(session._ctx), 1)
    if sky:
        scat, trans = sky_tables()
        if hasattr(session, "upload_sky"):
            session.upload_sky(scat, trans)
        else:   # the HIP library: device memory through vrt_sky_table_io
            import torch
            for which, t in ((_abi.BUF_SKY_SCATTERING, scat), (_abi.BUF_SKY_TRANSMITTANCE, trans)):
                d = torch.from_numpy(np.ascontiguousarray(t)).cuda()
                torch.cuda.synchronize()
                session.sky_table_io(which, 0, t.shape[0], d.data_ptr(), True)
                session.sync()
    return session


def camera_rays(o, pose, uv, width):
    """The rays of pixels uv of oracle context `o` at `pose`: (camera_pos, orc_unit_cast_dir(u, v)) bit for bit, stream = v * W + u."""
    rays = np.zeros(len(uv), PATH_RAY)
    rays["origin"] = np.array(POSES[pose][0], np.float32)
    rays["dir"] = [o.cast_dir(u, v) for u, v in uv]
    rays["stream"] = uv[:, 1] * width + uv[:, 0]
    return rays


@functools.lru_cache(maxsize=None)
def expected(case):
    """{pose: (rays, {n_samples: RADIANCE records})} from the oracle.  Computed once and left alone."""
    name, depth, _, _, poses = CASES[case]
    o = start(ShimOracle(config(case)), case)
    uv = np.array([(u, v) for v in range(H) for u in range(W)], np.int32)
    out = {}
    for k, pose in enumerate(poses):
        o.set_camera(camera(pose, k))
        rays = camera_rays(o, pose, uv, W)
        t = np.array([o.next_hit(r["origin"], r["dir"])["closest"] for r in rays], np.float32)
        want = {}
        for n in SAMPLES[case]:
            rec = np.zeros(len(rays), RADIANCE)
            rec["rgb"], rec["t"] = o.radiance(uv, n, FIRST_FRAME), t
            rec.setflags(write=False)
            want[n] = rec
        rays.setflags(write=False)
        out[pose] = (rays, want)
    o.close()
    return out


def walks(case, max_depth):
    """Voxel walks of sample 0 of every ray of the case, with another max_depth (the census of paths alive at the last segment)."""
    cfg = config(case)
    cfg.max_depth = max_depth
    o = start(ShimOracle(cfg), case)
    uv = np.array([(u, v) for v in range(H) for u in range(W)], np.int32)
    out = []
    for k, pose in enumerate(CASES[case][4]):
        o.set_camera(camera(pose, k))
        got = np.zeros(len(uv), np.uint32)
        assert o._lib.orc_radiance_walks(C.c_void_p(o._ctx), len(uv), orc.fptr(uv), FIRST_FRAME, orc.fptr(got)) == 0
        out.append(got)
    o.close()
    return np.concatenate(out)


def first_hit_kinds(case):
    """Of every ray of the case: 2 voxel, 1 floor, 0 sky -- the oracle's next_hit against the same call on a context without voxels."""
    name = CASES[case][0]
    _, floor = K.oracles(name)
    kinds = []
    for pose, (rays, want) in expected(case).items():
        t = next(iter(want.values()))["t"]
        f = np.array([floor.next_hit(r["origin"], r["dir"])["closest"] for r in rays], np.float32)
        kinds.append(np.where(np.isinf(t), 0, np.where(t == f, 1, 2)))
    return np.concatenate(kinds)


def mismatches(got, want):
    """Indices of the records that differ: floats by their bits, any NaN equal to any NaN."""
    return np.flatnonzero(~R.same_f32(got["rgb"], want["rgb"]).all(axis=1) | ~R.same_f32(got["t"], want["t"]))


def check(got, rays, want, label):
    bad = mismatches(got, want)
    assert bad.size == 0, (f"{label}: {bad.size} of {len(rays)} records differ: " +
                           "; ".join(f"ray {k} {rays[k]} got={got[k]} want={want[k]}" for k in bad[:3]))


# ---- the host build of the per-item functions -----------------------------------------------------------------------------------
class RadScene(C.Structure):
    _fields_ = [("grid_res", C.c_int32), ("ref_oob", C.c_int32), ("floor_material", C.c_int32), ("use_sky", C.c_int32), ("max_depth", C.c_int32),
                ("sky_res", C.c_int32), ("seed", C.c_uint32), ("pad", C.c_int32),
                ("floor_height", C.c_float), ("floor_color", C.c_float * 3), ("voxel_edges", C.c_float), ("background", C.c_float * 3),
                ("light_dir", C.c_float * 3), ("light_color", C.c_float * 3), ("light_cos_max", C.c_float), ("light_weight", C.c_float),
                ("cull", C.c_float * 8),
                ("grid", C.c_void_p), ("l0", C.c_void_p), ("l1", C.c_void_p), ("l2", C.c_void_p), ("l3", C.c_void_p),
                ("mats", C.c_void_p), ("sky_scat", C.c_void_p), ("sky_trans", C.c_void_p)]


def lib():
    if "emul" not in _libs:
        so = _build(_EMUL, os.path.join(HERE, "emul", "radiance_emul.cpp"), [os.path.join(ROOT, "voxel_rt2_amd", "csrc"), os.path.join(ROOT, "include"),
                                                                                os.path.join(HERE, "emul")], ["-Werror"])
        lib = C.CDLL(so)
        lib.radiance_emul_trace.argtypes = [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_void_p]
        lib.radiance_emul_valid.argtypes = [C.c_void_p]
        lib.radiance_emul_chunk.argtypes = [C.c_longlong, C.c_int]
        lib.radiance_emul_rays.argtypes = [C.c_longlong]
        lib.radiance_emul_rays.restype = C.c_longlong
        lib.radiance_emul_items.restype = C.c_longlong
        lib.radiance_emul_staged.argtypes = [C.c_longlong, C.c_int]
        lib.radiance_emul_poison.argtypes = [C.c_int]
        lib.radiance_emul_probe.argtypes = [C.c_void_p] * 3
        lib.radiance_emul_probe.restype = None
        _libs["emul"] = lib
    return _libs["emul"]


def poisoned():
    """tests/cast.py's poisoned() on this module's emulator."""
    return K.poisoned((lib(), "radiance"))


def probe(scene_record):
    return K.probe(scene_record, (lib(), "radiance"))


def chunks(n_rays, n_samples):
    """[(s0, count)] as sampled_query (vrt_scene_ops.hip) cuts a block's samples: plan_query_chunk whole samples at a time."""
    per = lib().radiance_emul_chunk(n_rays, n_samples)
    return [(s0, min(per, n_samples - s0)) for s0 in range(0, n_samples, max(per, 1))]


class HostScene:
    """A case's scene as k_trace_radiance reads it, built in numpy (tests/edit.py: rebuild; tests/rays.py: grown_box)."""

    def __init__(self, case):
        name, depth, _, ref, _ = CASES[case]
        mat, rgb, params = scene(case)
        sp = host.make_scene_params(**params)
        self.keep = dict(E.rebuild(mat, rgb), mats=np.ascontiguousarray(materials.load_table(), np.float32))
        s = self.s = RadScene()
        s.grid_res, s.ref_oob, s.floor_material, s.max_depth, s.seed = mat.shape[0], int(ref), sp.floor_material, depth, SEED
        s.floor_height, s.voxel_edges = sp.floor_height, params["voxel_edges"]
        s.floor_color[:], s.background[:] = list(sp.floor_color), list(sp.background_color)
        s.light_dir[:], s.light_color[:] = list(sp.light_direction), list(sp.light_color)
        s.light_cos_max, s.light_weight, s.use_sky = sp.light_cos_theta_max, sp.light_weight, sp.use_physical_sky
        if sp.use_physical_sky:
            scat, trans = sky_tables()
            self.keep.update(sky_scat=np.ascontiguousarray(scat), sky_trans=np.ascontiguousarray(trans))
            s.sky_res, s.sky_scat, s.sky_trans = SKY_RES, self.keep["sky_scat"].ctypes.data, self.keep["sky_trans"].ctypes.data
        lo, hi, active = R.grown_box(mat)
        s.cull[:] = list(lo) + list(hi) + [1.0, 0.0] if active and not ref else [-1e30] * 3 + [1e30] * 3 + [0.0, 0.0]
        for k in ("grid", "l0", "l1", "l2", "l3", "mats"):
            setattr(s, k, self.keep[k].ctypes.data)

    def trace(self, rays, n_samples, first_frame=FIRST_FRAME, staged=0, per=0):
        rays = np.ascontiguousarray(rays, PATH_RAY)
        out = np.zeros(len(rays), RADIANCE)
        assert lib().radiance_emul_trace(C.byref(self.s), int(staged), len(rays), orc.fptr(rays), int(n_samples), int(first_frame), int(per), orc.fptr(out)) == 0
        return out
