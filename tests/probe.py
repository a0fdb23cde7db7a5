"""vrt_gather_probes: cases, probes, expected records and the host build of the per-item functions (voxel_rt2_amd/csrc/vrt_probe_sh.h
through tests/emul/probe_emul.cpp).  Test infrastructure shared by tests/test_probe_host.py (no GPU), tests/test_gpu_probes.py and
tests/test_gpu_probe_states.py.  Everything is compared bit for bit, any NaN equal to any NaN; no tolerance, no row left out.

Expected values never come from the code under test.  Per (probe, sample) the oracle alone (tests/emul/probe_orc.cpp: the oracle's
sources, unchanged, and one function over its sampling, next_hit and sky functions) gives the sun sample with vis_s and sun_s, the
sphere direction w, whether the first segment escapes, whether w lies inside the sun's cone, and for an escape the sky-only value.
What a NON-escaping ray is worth is the radiance query's value for ray (pos, w, stream), one sample, at the sample's frame -- `query`:
tests/radiance.py's host build on the CPU, vrt_trace_radiance on the device, both pinned to the oracle's render_pixel by their own
tests.  For escaping rays outside the cone the sky-only value must ALSO equal the query's (the escape rule's cross-check).  expected()
then forms the basis, the products and the ordered sums in numpy float32, exactly as include/vrt_api.h writes them.

The cases are tests/sensor.py's, fixtures included; that module is imported and left unchanged."""
import ctypes as C
import functools
import os

import numpy as np

import cast as K
import orc
import radiance as X
import rays as R
import sensor as S
from voxel_rt2_amd import _abi
from voxel_rt2_amd._session import NativeSession

HERE = X.HERE
ROOT = X.ROOT
PROBE, SH_PROBE, PATH_RAY = _abi.PROBE, _abi.SH_PROBE, _abi.PATH_RAY
FIRST_FRAME = 5
SAMPLES = (1, 3)
CASES = S.CASES
SUNLIT = S.SUNLIT
scene, config, start, world = S.scene, S.config, S.start, S.world
K4 = np.float32(12.5663706)
ROW = 16
ITEM = np.dtype([("L", np.float32, 3), ("sky", np.float32), ("w", np.float32, 3), ("vis", np.float32), ("sun", np.float32, 3), ("pad", np.float32)])
assert ITEM.itemsize == 48


def basis(w):
    """Y0 .. Y8 of include/vrt_api.h at float32[n][3], in numpy float32, each line left to right: float32[n][9]."""
    f = np.float32
    w = np.asarray(w, f).reshape(-1, 3)
    x, y, z = w[:, 0], w[:, 1], w[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        Y = [np.full(len(w), f(0.282094792), f), f(0.488602512) * y, f(0.488602512) * z, f(0.488602512) * x, f(1.09254843) * (x * y), f(1.09254843) * (y * z),
             f(0.315391565) * (f(3.0) * (z * z) - f(1.0)), f(1.09254843) * (x * z), f(0.546274215) * (x * x - y * y)]
    out = np.stack(Y, axis=1)
    assert out.dtype == f
    return out


# ---- probes -----------------------------------------------------------------------------------------------------------------------
def make(pos, stream=0):
    with np.errstate(invalid="ignore"):
        pos = np.asarray(pos, np.float32).reshape(-1, 3)
    p = np.zeros(len(pos), PROBE)
    p["pos"], p["stream"] = pos, stream
    return p


def invalid_probes():
    """NaN, +inf and -inf in each component."""
    out = []
    for bad in (np.nan, np.inf, -np.inf):
        for a in range(3):
            pos = [0.1, 0.2, 0.3]
            pos[a] = bad
            out.append(make(pos))
    return np.concatenate(out)


def valid(probes):
    """The API's gate in numpy (include/vrt_api.h): finite components."""
    return np.isfinite(probes["pos"]).all(axis=1)


@functools.lru_cache(maxsize=None)
def toward_sun_streams(case, want=16, limit=1 << 16):
    """Streams whose sphere direction lies inside the sun's cone for one of the first max(SAMPLES) samples: w depends on (seed, frame,
    stream) alone, so they are found by asking the oracle about candidate streams at one position.  A choice of INPUTS."""
    o = start(ShimOracle(config(case)), case)
    try:
        found, at = [], 0
        while len(found) < want and at < limit:
            cand = make(np.tile(np.float32((0.0, 0.5, 0.0)), (4096, 1)), np.arange(at, at + 4096, dtype=np.uint32))
            rows = o.probe_samples(cand, max(SAMPLES), FIRST_FRAME)
            found += (at + np.flatnonzero((rows[:, :, 11] == 1).any(axis=1))).tolist()
            at += 4096
    finally:
        o.close()
    return tuple(found[:want])


@functools.lru_cache(maxsize=None)
def families(case):
    """{family: probes} of the case, streams numbered through (toward_sun: chosen streams).  Computed once and left alone."""
    name = CASES[case][0]
    mat, _, params = scene(case)
    G = mat.shape[0]
    rng = np.random.default_rng(20261019)
    fh = float(params["floor_height"])
    fam = {}

    def box(lo, hi, n):
        return make(world(G, rng.uniform(lo, hi, (n, 3))))

    def below_floor(x0, x1, z0, z1, n):
        return make(np.stack([world(G, rng.uniform(x0, x1, n)), (fh - rng.uniform(0.01, 0.3, n)).astype(np.float32), world(G, rng.uniform(z0, z1, n))], axis=1))

    def faces(n):
        """On and outside the grid's faces, up to 4 cells out: one coordinate ON a face (index 0 or G: exact in binary32) or beyond it."""
        idx = rng.uniform(0, G, (n, 3))
        for k in range(n):
            a, far = k % 3, (k // 3) % 2
            out = (0.0, 1.0, 2.5, 4.0)[(k // 6) % 4]
            idx[k, a] = G + out if far else -out
        return make(world(G, idx))

    def solid_centres(lo, hi, n):
        cells = np.argwhere(mat[tuple(slice(a, b) for a, b in zip(lo, hi))] > 0) + np.array(lo)
        return make(world(G, cells[np.sort(rng.choice(len(cells), size=min(n, len(cells)), replace=False))] + 0.5))
    if name == "sunlit":
        fam["open_air"] = box((30, 68, 40), (100, 100, 86), 32)
        fam["toward_sun"] = box((40, 90, 50), (80, 100, 80), 16)
        fam["among_blocks"] = box((37, 54, 46), (88, 66, 79), 32)                       # some inside voxels, most between them: shadowed suns
        fam["under_roof"] = box((97, 55, 97), (107, 65.5, 107), 24)
        fam["closed_box"] = box(tuple(a + 1.1 for a in S.BOX[0]), tuple(b - 1.1 for b in S.BOX[1]), 24)
        e = np.array(S.EMISSIVE, np.float64) + 0.5
        fam["emissive"] = make(world(G, e + rng.uniform(-3, 3, (16, 3)) * (1, 0, 1) + rng.uniform(0, 3, (16, 1)) * (0, 1, 0)))
        fam["solid"] = solid_centres((37, 54, 46), (108, 88, 108), 24)
        fam["below_floor"] = below_floor(30, 100, 40, 86, 16)
        fam["faces"] = faces(24)
    elif name == "dense":
        fam["corner"] = np.concatenate([box((-4, -4, -4), (6, 6, 6), 16), box((G - 6, G - 6, G - 6), (G + 4, G + 4, G + 4), 16),
                                        box((-4, G - 6, 60), (6, G + 4, 68), 16)])
        fam["solid"] = solid_centres((0, 0, 0), (8, 8, 8), 16)
        fam["inside"] = box((40, 40, 40), (90, 90, 90), 16)
        fam["above"] = box((0, G, 0), (G, G + 4, G), 16)
        fam["faces"] = faces(24)
    else:
        solid = np.argwhere(mat > 0)
        lo, hi = solid.min(axis=0), solid.max(axis=0) + 1
        fam["open_air"] = box((lo[0] - 8, hi[1], lo[2] - 8), (hi[0] + 8, hi[1] + 30, hi[2] + 8), 32)
        fam["among"] = box(lo - 2, hi + 2, 40)
        fam["solid"] = solid_centres(lo, hi, 24)
        fam["below_floor"] = below_floor(lo[0], hi[0], lo[2], hi[2], 16)
        fam["faces"] = faces(24)
    fam["invalid"] = invalid_probes()
    k = 0
    for f in fam.values():
        f["stream"] = (np.arange(k, k + len(f), dtype=np.uint64) * 7 + 3).astype(np.uint32)
        k += len(f)
    if "toward_sun" in fam:
        st = toward_sun_streams(case)
        fam["toward_sun"]["stream"][:len(st)] = np.array(st, np.uint32)
    for f in fam.values():
        f.setflags(write=False)
    return fam


def probes_of(case):
    return np.concatenate(list(families(case).values()))


def family_slices(case):
    out, k = {}, 0
    for name, f in families(case).items():
        out[name] = slice(k, k + len(f))
        k += len(f)
    return out


# ---- the oracle with the shim ---------------------------------------------------------------------------------------------------
_SHIM = os.path.join(HERE, "emul", "_probe_orc.so")
_EMUL = os.path.join(HERE, "emul", "_probe_emul.so")
_libs = {}


def shim():
    """The oracle's library with orc_probe_samples added: the oracle's own build flags (oracle/Makefile)."""
    if "shim" not in _libs:
        so = X._build(_SHIM, os.path.join(HERE, "emul", "probe_orc.cpp"), [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "include")],
                      ["-fno-unsafe-math-optimizations", "-pthread"])
        lib = C.CDLL(so)
        lib.orc_probe_samples.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]
        _libs["shim"] = lib
    return _libs["shim"]


class ShimOracle(orc.Oracle):
    def __init__(self, cfg, threads=1):
        NativeSession.__init__(self, shim(), "orc_", cfg, create_extra=(C.c_int(threads),))
        self.threads = threads

    def probe_samples(self, probes, n_samples, first_frame):
        probes = np.ascontiguousarray(probes, PROBE)
        out = np.zeros((len(probes), n_samples, ROW), np.float32)
        assert self._lib.orc_probe_samples(C.c_void_p(self._ctx), len(probes), orc.fptr(probes), int(n_samples), int(first_frame) & 0xFFFFFFFF, orc.fptr(out)) == 0
        return out


@functools.lru_cache(maxsize=None)
def oracle_rows(case, n_samples=max(SAMPLES), first_frame=FIRST_FRAME):
    """float32[n][n_samples][ROW] of the case's probes from the oracle (tests/emul/probe_orc.cpp's layout); zeros for invalid probes,
    which the oracle is not asked about.  Sample s of a call with fewer samples is row s of this."""
    probes = probes_of(case)
    ok = valid(probes)
    o = start(ShimOracle(config(case)), case)
    rows = np.zeros((len(probes), n_samples, ROW), np.float32)
    rows[ok] = o.probe_samples(probes[ok], n_samples, first_frame)
    o.close()
    rows.setflags(write=False)
    return rows


def census(case):
    """From the oracle's data alone: how many samples see the sun, are shadowed, escape, hit, escape inside the sun's cone."""
    rows = oracle_rows(case).reshape(-1, ROW)[np.repeat(valid(probes_of(case)), max(SAMPLES))]
    return dict(visible=int((rows[:, 3] == 1).sum()), shadowed=int((rows[:, 3] == 0).sum()), escapes=int((rows[:, 10] == 1).sum()),
                hits=int((rows[:, 10] == 0).sum()), escape_in_cone=int(((rows[:, 10] == 1) & (rows[:, 11] == 1)).sum()), samples=len(rows))


def sample_terms(case, s, query, probes, rows, first_frame):
    """float32[n][12] in ITEM's layout: the terms of sample s of every probe (zeros for invalid probes and for rays the gate refuses)."""
    ok = valid(probes)
    row = rows[ok, s]
    rays = np.zeros(len(row), PATH_RAY)
    rays["origin"], rays["dir"], rays["stream"] = probes["pos"][ok], row[:, 7:10], probes["stream"][ok]
    L = np.asarray(query(rays, (first_frame + s) & 0xFFFFFFFF), np.float32)
    esc, cone = row[:, 10] == 1, row[:, 11] == 1
    out_of_cone = esc & ~cone
    bad = np.flatnonzero(~R.same_f32(L[out_of_cone], row[out_of_cone, 12:15]).all(axis=1))
    assert bad.size == 0, f"{case} sample {s}: the oracle's sky-only value differs from the radiance query's for {bad.size} escaping rays outside the cone"
    L = np.where(esc[:, None], row[:, 12:15], L).astype(np.float32)
    # the query's gate on the derived ray (finite w, not all zeros): such a sample is walked, any other is all zeros
    ray = np.isfinite(row[:, 7:10]).all(axis=1) & (row[:, 7:10] != 0).any(axis=1)
    term = np.zeros((len(probes), 12), np.float32)
    term[ok, 0:3] = np.where(ray[:, None], L, np.float32(0))
    term[ok, 3] = np.where(ray, row[:, 10], np.float32(0))
    term[ok, 4:7] = np.where(ray[:, None], row[:, 7:10], np.float32(0))
    term[ok, 7] = np.where(ray, row[:, 3], np.float32(0))
    term[ok, 8:11] = np.where(ray[:, None], row[:, 4:7], np.float32(0))
    return term


def fold(acc, term):
    """One sample's 32 terms added to float32[n][32] `acc` (SH_PROBE's layout), as steps 4 and 5 of include/vrt_api.h write them."""
    Lw = term[:, 0:3] * K4
    Y = basis(term[:, 4:7])
    add = np.zeros_like(acc)
    with np.errstate(invalid="ignore", over="ignore"):
        add[:, 0:27] = (Lw[:, None, :] * Y[:, :, None]).reshape(-1, 27)              # sh[i][ch] = Lw[ch] * Yi
    add[:, 27] = term[:, 3]
    add[:, 28:31] = term[:, 8:11]
    add[:, 31] = term[:, 7]
    assert add.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        return acc + add


def expected(case, n_samples, query, probes=None, rows=None, first_frame=FIRST_FRAME):
    """The SH_PROBE records of the case's probes.  query(rays, frame) -> float32[n][3]: the radiance query's rgb for one sample of
    `rays` at `frame`."""
    probes = probes_of(case) if probes is None else probes
    rows = oracle_rows(case) if rows is None else rows
    acc = np.zeros((len(probes), 32), np.float32)
    for s in range(n_samples):
        acc = fold(acc, sample_terms(case, s, query, probes, rows, first_frame))
    with np.errstate(invalid="ignore"):
        out = (acc / np.float32(n_samples)).astype(np.float32)
    return np.ascontiguousarray(out).view(SH_PROBE).reshape(-1)


def as_floats(rec):
    return np.ascontiguousarray(rec).view(np.float32).reshape(-1, 32)


def mismatches(got, want):
    return np.flatnonzero(~R.same_f32(as_floats(got), as_floats(want)).all(axis=1))


def check(got, probes, want, label):
    bad = mismatches(got, want)
    assert bad.size == 0, (f"{label}: {bad.size} of {len(probes)} records differ: " +
                           "; ".join(f"probe {k} {probes[k]} got={got[k]} want={want[k]}" for k in bad[:2]))


# ---- the host builds ----------------------------------------------------------------------------------------------------------------
def lib():
    if "emul" not in _libs:
        so = X._build(_EMUL, os.path.join(HERE, "emul", "probe_emul.cpp"), [os.path.join(ROOT, "voxel_rt2_amd", "csrc"), os.path.join(ROOT, "include"),
                                                                             os.path.join(HERE, "emul")], ["-Werror"])
        lib = C.CDLL(so)
        lib.probe_emul_gather.argtypes = [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_void_p]
        lib.probe_emul_valid.argtypes = [C.c_void_p]
        lib.probe_emul_chunk.argtypes = [C.c_longlong, C.c_int]
        lib.probe_emul_rays.argtypes = [C.c_longlong]
        lib.probe_emul_rays.restype = C.c_longlong
        lib.probe_emul_items.restype = C.c_longlong
        lib.probe_emul_item_bytes.restype = C.c_longlong
        lib.probe_emul_basis.argtypes = [C.c_float, C.c_float, C.c_float, C.c_void_p]
        lib.probe_emul_basis.restype = None
        lib.probe_emul_fold.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int]
        lib.probe_emul_fold.restype = None
        lib.probe_emul_poison.argtypes = [C.c_int]
        lib.probe_emul_probe.argtypes = [C.c_void_p] * 3
        lib.probe_emul_probe.restype = None
        _libs["emul"] = lib
    return _libs["emul"]


def poisoned():
    """tests/cast.py's poisoned() on this module's emulator."""
    return K.poisoned((lib(), "probe"))


def probe(scene_record):
    return K.probe(scene_record, (lib(), "probe"))


def blocks(n):
    """[(at, m)] as vrt_gather_probes cuts a call into blocks of probes."""
    per = lib().probe_emul_rays(n)
    return [(at, min(per, n - at)) for at in range(0, n, max(per, 1))]


def chunks(n_probes, n_samples):
    """[(s0, count)] as sampled_query (vrt_scene_ops.hip) cuts a block's samples: plan_query_chunk whole samples at a time."""
    per = lib().probe_emul_chunk(n_probes, n_samples)
    return [(s0, min(per, n_samples - s0)) for s0 in range(0, n_samples, max(per, 1))]


class HostScene(S.HostScene):
    """tests/sensor.py's scene record of a case; gather(): the host build of vrt_probe_sh.h."""

    def gather(self, probes, n_samples, first_frame=FIRST_FRAME, staged=0, per=0):
        probes = np.ascontiguousarray(probes, PROBE)
        out = np.zeros(len(probes), SH_PROBE)
        assert lib().probe_emul_gather(C.byref(self.s), int(staged), len(probes), orc.fptr(probes), int(n_samples), int(first_frame) & 0xFFFFFFFF, int(per),
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
