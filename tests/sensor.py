"""vrt_gather_irradiance: cases, sensors, expected records and the host build of the per-item functions (voxel_rt2_amd/csrc/vrt_sensor.h
through tests/emul/sensor_emul.cpp).  Test infrastructure shared by tests/test_sensor_host.py (no GPU) and tests/test_gpu_sensor.py.
Everything is compared bit for bit, any NaN equal to any NaN; no tolerance, no row left out.

Expected values never come from the code under test.  Per (sensor, sample) the oracle alone (tests/emul/sensor_orc.cpp: the oracle's
sources, unchanged, and one function over its sampling, next_hit and sky functions) gives the ray origin o, the sun sample with vis_s
and sun_s, the hemisphere direction w, whether the first segment escapes, whether w lies inside the sun's cone, and for an escape the
sky-only value.  What a NON-escaping hemisphere ray is worth is the radiance query's value for ray (o, w, stream), one sample, at the
sample's frame -- `query`: tests/radiance.py's host build on the CPU, vrt_trace_radiance on the device, both pinned to the oracle's
render_pixel by their own tests.  For escaping rays outside the cone the sky-only value must ALSO equal the query's (the escape rule's
cross-check).  expected() then multiplies by pi and folds in numpy float32 in the stated order.

A case is a scene of tests/radiance.py with settings; the 128^3 sun-lit ones get a few fixtures added (fixtures()): a roof slab on a
pillar (an overhang), a closed hollow box, voxels on the grid's boundary, an emissive voxel with a plain neighbour."""
import ctypes as C
import functools
import os

import numpy as np

import cast as K
import edit as E
import orc
import radiance as X
import rays as R
from voxel_rt2_amd import _abi, host, materials
from voxel_rt2_amd._session import NativeSession
from voxel_rt2_amd.renderer import VoxelStore

HERE = X.HERE
ROOT = X.ROOT
SENSOR, IRRADIANCE, PATH_RAY = _abi.SENSOR, _abi.IRRADIANCE, _abi.PATH_RAY
SEED = X.SEED
FIRST_FRAME = 5
SKY_RES = X.SKY_RES
PI32 = np.float32(3.14159274)
SAMPLES = (1, 3)
# name: (scene, max_depth, scene-parameter overrides, reference indexing)
CASES = {f"sunlit_d{d}": ("sunlit", d, {}, False) for d in (1, 2, 5, 8)}
CASES.update({
    "sky": ("sunlit", 4, dict(use_physical_sky=1, use_clouds=0), False),
    "dense": ("dense", 4, {}, False),                              # dense_ref's other mode: vrt_set_reference_indexing toggled on a live context
    "dense_ref": ("dense", 4, {}, True),
    "s1_256": ("s1_256", 4, {}, False),
    "cone": ("sunlit", 2, dict(light_cone=0.8), False),          # example5.py's wide sun
    "sunlit_d2_relit": ("sunlit", 2, X.RELIT, False),            # tests/radiance.py: what vrt_set_scene can change behind a prepared scene
})
SUNLIT = tuple(c for c in CASES if CASES[c][0] == "sunlit")
# the fixtures, in array indices (the sun-lit scene's blocks lie in x 37..87, y 54..65, z 46..78)
ROOF = ((96, 66, 96), (108, 67, 108))
BOX = ((100, 80, 50), (107, 87, 57))
EMISSIVE, NEIGHBOUR = (92, 54, 50), (93, 54, 50)


def fixtures(mat, rgb):
    mat, rgb = mat.copy(), rgb.copy()

    def put(lo, hi, m, c=(180, 170, 160)):
        box = tuple(slice(a, b) for a, b in zip(lo, hi))
        mat[box] = m
        rgb[box] = c
    put(*ROOF, 1)
    put((96, 54, 96), (97, 66, 97), 1)                                   # its pillar
    put(*BOX, 11)
    put(tuple(a + 1 for a in BOX[0]), tuple(b - 1 for b in BOX[1]), 0, (0, 0, 0))   # hollow
    put((127, 54, 60), (128, 58, 64), 1)                                 # on the grid's +x boundary
    put((0, 54, 0), (1, 56, 1), 21)                                      # in its corner
    put((64, 127, 64), (65, 128, 65), 1)                                 # on its top
    put(EMISSIVE, tuple(a + 1 for a in EMISSIVE), 2, (255, 240, 200))
    put(NEIGHBOUR, tuple(a + 1 for a in NEIGHBOUR), 1)
    return mat, rgb


@functools.lru_cache(maxsize=None)
def scene(case):
    name, _, over, _ = CASES[case]
    mat, rgb, params = K.scene(name)
    if name == "sunlit":
        mat, rgb = fixtures(mat, rgb)
    return mat, rgb, dict(params, **over)


def config(case, width=16, height=8, **kw):
    _, depth, _, _ = CASES[case]
    mat, _, params = scene(case)
    return host.make_config(width, height, voxel_edges=params["voxel_edges"], exposure=params["exposure"], max_depth=depth, seed=SEED,
                            sky_res=SKY_RES if params.get("use_physical_sky") else 0, grid_res=mat.shape[0], **kw)


def start(session, case):
    """Drive a session (oracle or product) to a prepared scene of the case; the sky tables are the oracle's (tests/radiance.py)."""
    mat, rgb, params = scene(case)
    sky = bool(params.get("use_physical_sky"))
    orc.setup(session, mat, rgb, params, cloud=np.zeros((256, 256, 3), np.uint8) if sky else None)
    if CASES[case][3]:
        if session._p == "vrt_":
            session.set_reference_indexing(True)
        else:
            session._lib.orc_set_reference_indexing(C.c_void_p(session._ctx), 1)
    if sky:
        scat, trans = X.sky_tables()
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


# ---- sensors ----------------------------------------------------------------------------------------------------------------------
def store(mat):
    """A VoxelStore (voxel_rt2_amd/renderer.py: the facade's voxel arrays, no device) holding `mat`."""
    st = VoxelStore()
    st._init_voxels(mat.shape[0])
    st.voxel_material[...] = mat
    return st


def make(pos, normal, reserved=0):
    with np.errstate(invalid="ignore"):
        pos, normal = np.asarray(pos, np.float32).reshape(-1, 3), np.asarray(normal, np.float32).reshape(-1, 3)
    s = np.zeros(max(len(pos), len(normal)), SENSOR)
    s["pos"], s["normal"], s["reserved"] = pos, normal, reserved
    return s


def world(G, idx):
    return ((np.asarray(idx, np.float64) - G / 2) * (2.0 / G)).astype(np.float32)


def invalid_sensors():
    nan, inf = np.nan, np.inf
    up = (0.0, 1.0, 0.0)
    return np.concatenate([make((nan, 0.0, 0.0), up), make((0.0, inf, 0.0), up), make((0.0, 0.0, -inf), up), make((0.1, 0.2, 0.3), (0.0, nan, 0.0)),
                           make((0.1, 0.2, 0.3), (inf, 0.0, 0.0)), make((0.1, 0.2, 0.3), (0.0, 0.0, 0.0)), make((0.1, 0.2, 0.3), (-0.0, 0.0, -0.0)),
                           make((0.1, 0.2, 0.3), up, reserved=1)])


def valid(sensors):
    """The API's gate in numpy (include/vrt_api.h): finite components, a normal that is not all zeros, reserved 0."""
    return (np.isfinite(sensors["pos"]).all(axis=1) & np.isfinite(sensors["normal"]).all(axis=1) & (sensors["normal"] != 0).any(axis=1) &
            (sensors["reserved"] == 0))


def _pick(rng, arrays, n):
    idx = np.sort(rng.choice(len(arrays[0]), size=min(n, len(arrays[0])), replace=False))
    return [a[idx] for a in arrays]


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def families(case):
    """{family: sensors} of the case, streams numbered through.  Computed once and left alone."""
    name = CASES[case][0]
    mat, _, params = scene(case)
    G = mat.shape[0]
    rng = np.random.default_rng(20261018)
    st = store(mat)
    fh = np.float32(params["floor_height"])
    up = (0.0, 1.0, 0.0)
    fam = {}

    def floor_points(x0, x1, z0, z1, n):
        p = np.stack([world(G, rng.uniform(x0, x1, n)), np.full(n, fh, np.float32), world(G, rng.uniform(z0, z1, n))], axis=1)
        return make(p, up)
    if name == "sunlit":
        fam["floor"] = floor_points(30, 100, 40, 86, 48)
        cell, face, centre, normal = st.surface_faces((37, 54, 46), (88, 66, 79))
        top = face == 3
        fam["tops"] = make(*_pick(rng, (centre[top], normal[top]), 32))
        side = (face != 3) & (face != 2)
        fam["sides"] = make(*_pick(rng, (centre[side], normal[side]), 32))
        edge = [st.surface_faces(lo, hi) for lo, hi in (((127, 54, 60), (128, 58, 64)), ((0, 54, 0), (1, 56, 1)), ((64, 127, 64), (65, 128, 65)))]
        fam["boundary"] = make(np.concatenate([e[2] for e in edge]), np.concatenate([e[3] for e in edge]))
        fam["overhang"] = floor_points(97, 107, 97, 107, 24)
        cell, face, centre, normal = st.surface_faces(*ROOF)
        fam["away"] = make(*_pick(rng, (centre[face == 2], normal[face == 2]), 24))            # the roof from below: normal -y, ndl <= 0
        cell, face, centre, normal = st.surface_faces(*BOX)
        inner = ((cell + normal.astype(np.int32) > np.array(BOX[0])) & (cell + normal.astype(np.int32) < np.array(BOX[1]) - 1)).all(axis=1)
        fam["closed_box"] = make(*_pick(rng, (centre[inner], normal[inner]), 32))
        n = _unit(rng, 32)
        fam["oblique"] = make(np.stack([world(G, rng.uniform(40, 100, 32)), world(G, rng.uniform(56, 76, 32)), world(G, rng.uniform(44, 84, 32))], axis=1), n)
        near = [st.surface_faces(tuple(np.array(c)), tuple(np.array(c) + 1)) for c in (EMISSIVE, NEIGHBOUR)]
        beside = floor_points(EMISSIVE[0] - 2, EMISSIVE[0] + 4, EMISSIVE[2] - 2, EMISSIVE[2] + 3, 12)
        fam["emissive"] = np.concatenate([make(np.concatenate([e[2] for e in near]), np.concatenate([e[3] for e in near])), beside])
    elif name == "dense":
        cell, face, centre, normal = st.surface_faces((118, 118, 118), (128, 128, 128))
        outer = ((cell + normal.astype(np.int32) < 0) | (cell + normal.astype(np.int32) >= G)).any(axis=1)
        fam["boundary"] = make(*_pick(rng, (centre[outer], normal[outer]), 32))
        fam["faces"] = make(*_pick(rng, (centre[~outer], normal[~outer]), 64))
        cell, face, centre, normal = st.surface_faces((0, 60, 60), (6, 68, 68))
        fam["corner"] = make(*_pick(rng, (centre, normal), 32))
        fam["oblique"] = make(world(G, rng.uniform(-4, G + 4, (24, 3))), _unit(rng, 24))
    else:
        solid = np.argwhere(mat > 0)
        lo, hi = solid.min(axis=0), solid.max(axis=0) + 1
        cell, face, centre, normal = st.surface_faces(lo, hi)
        fam["tops"] = make(*_pick(rng, (centre[face == 3], normal[face == 3]), 40))
        fam["sides"] = make(*_pick(rng, (centre[face != 3], normal[face != 3]), 40))
        fam["floor"] = floor_points(lo[0] - 8, hi[0] + 8, lo[2] - 8, hi[2] + 8, 24)
        fam["oblique"] = make(world(G, rng.uniform(lo - 4, hi + 4, (24, 3))), _unit(rng, 24))
    fam["invalid"] = invalid_sensors()
    k = 0
    for f in fam.values():
        f["stream"] = (np.arange(k, k + len(f), dtype=np.uint64) * 7 + 3).astype(np.uint32)
        k += len(f)
        f.setflags(write=False)
    return fam


def sensors_of(case):
    return np.concatenate(list(families(case).values()))


def family_slices(case):
    out, k = {}, 0
    for name, f in families(case).items():
        out[name] = slice(k, k + len(f))
        k += len(f)
    return out


# ---- the oracle with the shim ---------------------------------------------------------------------------------------------------
_SHIM = os.path.join(HERE, "emul", "_sensor_orc.so")
_EMUL = os.path.join(HERE, "emul", "_sensor_emul.so")
_libs = {}
ROW = 20


def shim():
    """The oracle's library with orc_sensor_samples added: the oracle's own build flags (oracle/Makefile)."""
    if "shim" not in _libs:
        so = X._build(_SHIM, os.path.join(HERE, "emul", "sensor_orc.cpp"), [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "include")],
                      ["-fno-unsafe-math-optimizations", "-pthread"])
        lib = C.CDLL(so)
        lib.orc_sensor_samples.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]
        _libs["shim"] = lib
    return _libs["shim"]


class ShimOracle(orc.Oracle):
    def __init__(self, cfg, threads=1):
        NativeSession.__init__(self, shim(), "orc_", cfg, create_extra=(C.c_int(threads),))
        self.threads = threads

    def sensor_samples(self, sensors, n_samples, first_frame):
        sensors = np.ascontiguousarray(sensors, SENSOR)
        out = np.zeros((len(sensors), n_samples, ROW), np.float32)
        assert self._lib.orc_sensor_samples(C.c_void_p(self._ctx), len(sensors), orc.fptr(sensors), int(n_samples), int(first_frame) & 0xFFFFFFFF, orc.fptr(out)) == 0
        return out


@functools.lru_cache(maxsize=None)
def oracle_rows(case, n_samples=max(SAMPLES), first_frame=FIRST_FRAME):
    """float32[n][n_samples][ROW] of the case's sensors from the oracle (tests/emul/sensor_orc.cpp's layout); zeros for invalid sensors,
    which the oracle is not asked about.  Sample s of a call with fewer samples is row s of this."""
    sensors = sensors_of(case)
    ok = valid(sensors)
    o = start(ShimOracle(config(case)), case)
    rows = np.zeros((len(sensors), n_samples, ROW), np.float32)
    rows[ok] = o.sensor_samples(sensors[ok], n_samples, first_frame)
    o.close()
    rows.setflags(write=False)
    return rows


def census(case):
    """From the oracle's data alone: samples that escape inside the sun's cone, that see the sun, that face it and are shadowed."""
    rows = oracle_rows(case).reshape(-1, ROW)[np.repeat(valid(sensors_of(case)), max(SAMPLES))]
    return dict(escape_in_cone=int(((rows[:, 14] == 1) & (rows[:, 15] == 1)).sum()), visible=int((rows[:, 7] == 1).sum()),
                shadowed=int(((rows[:, 7] == 0) & (rows[:, 6] > 0)).sum()), facing_away=int((rows[:, 6] <= 0).sum()),
                escapes=int((rows[:, 14] == 1).sum()), hits=int((rows[:, 14] == 0).sum()), samples=len(rows))


def expected(case, n_samples, query, sensors=None, rows=None, first_frame=FIRST_FRAME):
    """The IRRADIANCE records of the case's sensors.  query(rays, frame) -> float32[n][3]: the radiance query's rgb for one sample of
    `rays` at `frame`."""
    sensors = sensors_of(case) if sensors is None else sensors
    rows = oracle_rows(case) if rows is None else rows
    ok = valid(sensors)
    acc = np.zeros((len(sensors), 8), np.float32)
    for s in range(n_samples):
        row = rows[ok, s]
        rays = np.zeros(len(row), PATH_RAY)
        rays["origin"], rays["dir"], rays["stream"] = row[:, 0:3], row[:, 11:14], sensors["stream"][ok]
        L = np.asarray(query(rays, (first_frame + s) & 0xFFFFFFFF), np.float32)
        esc, cone = row[:, 14] == 1, row[:, 15] == 1
        out_of_cone = esc & ~cone
        bad = np.flatnonzero(~R.same_f32(L[out_of_cone], row[out_of_cone, 16:19]).all(axis=1))
        assert bad.size == 0, f"{case} sample {s}: the oracle's sky-only value differs from the radiance query's for {bad.size} escaping rays outside the cone"
        L = np.where(esc[:, None], row[:, 16:19], L).astype(np.float32)
        # the query's gate on the derived ray (finite o and w, w not all zeros): such a sample is walked, any other is all zeros
        ray = np.isfinite(row[:, 0:3]).all(axis=1) & np.isfinite(row[:, 11:14]).all(axis=1) & (row[:, 11:14] != 0).any(axis=1)
        term = np.zeros((len(sensors), 8), np.float32)
        term[ok, 0:3] = np.where(ray[:, None], L * PI32, np.float32(0))
        term[ok, 3] = np.where(ray, row[:, 14], np.float32(0))
        term[ok, 4:7] = np.where(ray[:, None], row[:, 8:11], np.float32(0))
        term[ok, 7] = np.where(ray, row[:, 7], np.float32(0))
        acc = acc + term
    out = (acc / np.float32(n_samples)).astype(np.float32)
    return np.ascontiguousarray(out).view(IRRADIANCE).reshape(-1)


def as_floats(rec):
    return np.ascontiguousarray(rec).view(np.float32).reshape(-1, 8)


def mismatches(got, want):
    return np.flatnonzero(~R.same_f32(as_floats(got), as_floats(want)).all(axis=1))


def check(got, sensors, want, label):
    bad = mismatches(got, want)
    assert bad.size == 0, (f"{label}: {bad.size} of {len(sensors)} records differ: " +
                           "; ".join(f"sensor {k} {sensors[k]} got={got[k]} want={want[k]}" for k in bad[:3]))


# ---- the host builds ----------------------------------------------------------------------------------------------------------------
def lib():
    if "emul" not in _libs:
        so = X._build(_EMUL, os.path.join(HERE, "emul", "sensor_emul.cpp"), [os.path.join(ROOT, "voxel_rt2_amd", "csrc"), os.path.join(ROOT, "include"),
                                                                              os.path.join(HERE, "emul")], ["-Werror"])
        lib = C.CDLL(so)
        lib.sensor_emul_gather.argtypes = [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_void_p]
        lib.sensor_emul_valid.argtypes = [C.c_void_p]
        lib.sensor_emul_chunk.argtypes = [C.c_longlong, C.c_int]
        lib.sensor_emul_rays.argtypes = [C.c_longlong]
        lib.sensor_emul_rays.restype = C.c_longlong
        lib.sensor_emul_items.restype = C.c_longlong
        lib.sensor_emul_item_bytes.restype = C.c_longlong
        lib.sensor_emul_fold.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int]
        lib.sensor_emul_fold.restype = None
        lib.sensor_emul_poison.argtypes = [C.c_int]
        lib.sensor_emul_probe.argtypes = [C.c_void_p] * 3
        lib.sensor_emul_probe.restype = None
        _libs["emul"] = lib
    return _libs["emul"]


def poisoned():
    """tests/cast.py's poisoned() on this module's emulator."""
    return K.poisoned((lib(), "sensor"))


def probe(scene_record):
    return K.probe(scene_record, (lib(), "sensor"))


def blocks(n):
    """[(at, m)] as vrt_gather_irradiance cuts a call into blocks of sensors."""
    per = lib().sensor_emul_rays(n)
    return [(at, min(per, n - at)) for at in range(0, n, max(per, 1))]


def chunks(n_sensors, n_samples):
    """[(s0, count)] as sampled_query (vrt_scene_ops.hip) cuts a block's samples: plan_query_chunk whole samples at a time."""
    per = lib().sensor_emul_chunk(n_sensors, n_samples)
    return [(s0, min(per, n_samples - s0)) for s0 in range(0, n_samples, max(per, 1))]


class HostScene(X.HostScene):
    """A case's scene as k_gather_irradiance reads it (tests/radiance.py's record, on this module's scenes).  trace(): the radiance
    query's host build (tests/emul/radiance_emul.cpp) -- `query` of expected(); gather(): the host build of vrt_sensor.h."""

    def __init__(self, case):
        _, depth, _, ref = CASES[case]
        mat, rgb, params = scene(case)
        sp = host.make_scene_params(**params)
        self.keep = dict(E.rebuild(mat, rgb), mats=np.ascontiguousarray(materials.load_table(), np.float32))
        s = self.s = X.RadScene()
        s.grid_res, s.ref_oob, s.floor_material, s.max_depth, s.seed = mat.shape[0], int(ref), sp.floor_material, depth, SEED
        s.floor_height, s.voxel_edges = sp.floor_height, params["voxel_edges"]
        s.floor_color[:], s.background[:] = list(sp.floor_color), list(sp.background_color)
        s.light_dir[:], s.light_color[:] = list(sp.light_direction), list(sp.light_color)
        s.light_cos_max, s.light_weight, s.use_sky = sp.light_cos_theta_max, sp.light_weight, sp.use_physical_sky
        if sp.use_physical_sky:
            scat, trans = X.sky_tables()
            self.keep.update(sky_scat=np.ascontiguousarray(scat), sky_trans=np.ascontiguousarray(trans))
            s.sky_res, s.sky_scat, s.sky_trans = SKY_RES, self.keep["sky_scat"].ctypes.data, self.keep["sky_trans"].ctypes.data
        lo, hi, active = R.grown_box(mat)
        s.cull[:] = list(lo) + list(hi) + [1.0, 0.0] if active and not ref else [-1e30] * 3 + [1e30] * 3 + [0.0, 0.0]
        for k in ("grid", "l0", "l1", "l2", "l3", "mats"):
            setattr(s, k, self.keep[k].ctypes.data)

    def query(self, rays, frame):
        return self.trace(rays, 1, first_frame=frame)["rgb"]

    def gather(self, sensors, n_samples, first_frame=FIRST_FRAME, staged=0, per=0):
        sensors = np.ascontiguousarray(sensors, SENSOR)
        out = np.zeros(len(sensors), IRRADIANCE)
        assert lib().sensor_emul_gather(C.byref(self.s), int(staged), len(sensors), orc.fptr(sensors), int(n_samples), int(first_frame) & 0xFFFFFFFF, int(per),
                                        orc.fptr(out)) == 0
        return out


@functools.lru_cache(maxsize=None)
def host_scene(case):
    return HostScene(case)


@functools.lru_cache(maxsize=None)
def expected_host(case, n_samples):
    """expected() with the radiance query's host build.  Computed once and left alone."""
    want = expected(case, n_samples, host_scene(case).query)
    want.setflags(write=False)
    return want
