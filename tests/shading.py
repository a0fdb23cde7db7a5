"""Rows for the shading probes (vrt_shade_probe on the device, emu_shade_probe on the host build of the same code, vrt_shade_probe.h):
named classes of edge rows, a seeded random set, the oracle's answers (orc_unit_*), the row layouts of the probe's ops and the
comparison.  Test infrastructure shared by tests/golden/make_reference_vectors.py (edge_function_vectors writes what the reference's
own source computes for edge_rows() into tests/golden/reference/functions_edges.npz), tests/test_shade_probe.py (no GPU) and
tests/test_gpu_shade_probe.py -- the role tests/rays.py has for single rays.

Everything is compared bit for bit, any NaN equal to any NaN.  There is no tolerance; ZERO_SIGN_OPEN names the one class on which
the sign of a zero result is left open, and why.

Layouts (one row per lane; integers and bit patterns travel as float bit patterns):
  op 0  EVAL      mat 14, v 3, n 3, l 3, form                    -> diffuse rgb, specular rgb, pdf_all               (orc_unit_bsdf_eval)
  op 1  LOBE_PDF  mat 14, v 3, n 3, l 3, lobe, form              -> pdf of the lobe                                   (orc_unit_lobe_pdf)
  op 2  SAMPLE    mat 14, v 3, n 3, seed, count                  -> count x (direction, brdf rgb, pdf, lobe)          (orc_unit_bsdf_sample)
  op 3  CONE      cos_max, n 3, seed, count                      -> count x direction                                 (orc_unit_sample_cone)
  op 4  OCT_ENC   v 3 -> code (two binary16)          op 5  OCT_DEC   code -> v 3
  op 6  MAT_ENC   id, albedo 3 -> code                op 7  ALBEDO    code -> albedo 3
  op 8  HASH3     x, y, z -> hash                     op 9  UCHIMURA  x -> y
  op 10 RESERVOIR sample 21, M, weight -> the same 23 after encode -> decode                                           (orc_unit_reservoir_roundtrip)
  op 11 SHIFT     dst_pos 3, dst_n 3, dst_mat 14, src_pos 3, sample 21, view 3, dst_M
                  -> diffuse rgb, specular rgb, jacobian (shift_sample), shift_jacobian, shift_is_constant             (orc_unit_shift)
form: 0 the render kernels' eval_lobes / pdf_all / pdf_lobe on surf_init; 1 bsdf_eval_pdf on surf_set + surf_shared with the
material-derived terms through the per-id table; 2 bsdf_eval_pdf_pre on surf_shared_view + mat_colours + dir_terms."""
import ctypes as C
import functools
import os

import numpy as np

import orc
from voxel_rt2_amd import host, materials, scenes

HERE = os.path.dirname(os.path.abspath(__file__))
OP = dict(EVAL=0, LOBE_PDF=1, SAMPLE=2, CONE=3, OCT_ENC=4, OCT_DEC=5, MAT_ENC=6, ALBEDO=7, HASH3=8, UCHIMURA=9, RESERVOIR=10, SHIFT=11)
FORMS = (0, 1, 2)
ROWS_PER_CLASS = 8
NAN_ROWS = 12              # rows of a class that is there for its NaNs (the census wants at least 10 of them to be NaN in the reference)
SAMPLE_SEED = 77           # row k draws from seed SAMPLE_SEED + k (function_vectors' rule)
CONE_SEED = 4
EDGE_DRAWS = 2             # draws per row of the edge file (functions.npz has 4 per material, 3 per cone)
MAT_FIELDS = ["subsurface", "metallic", "specular", "specular_tint", "roughness", "anisotropic", "sheen", "sheen_tint", "clearcoat",
              "clearcoat_gloss", "ior_minus_one"]
COL = {name: 3 + j for j, name in enumerate(MAT_FIELDS)}
LOBE_CODES = (0, 1, 2, 9, 5, -3)         # the three lobes, LOBE_ALL, and the two out-of-range codes of emu_bsdf_selftest
# Classes whose rows hold a product n.l that is exactly -0.0.  The reference clamps it with ti.max(x, 0.0): llvm.maxnum, which leaves the
# sign of max(-0, +0) to the target.  The emulation the fixtures were written under returns its first operand (-0, and the shifted
# integrand becomes 0 * -0 = -0); the numeric contract (include/vrt_detmath.h) is the gfx950 instruction, which orders -0 below +0.
# On these classes a zero equals a zero of either sign; every other value, and every other class, is compared bit for bit.
ZERO_SIGN_OPEN = ("shift/dst_nl_0",)
# (a coincident vertex gives the shift a NaN direction, but its clamps and the Jacobian's guard leave zeros: no NaN comes out of it)
NAN_CLASSES = {"bsdf": ("dir/l_eq_minus_v",), "shift": ()}
F32 = np.float32


def f32(x):
    return np.asarray(x, dtype=np.float32)


def bits(a):
    """Integers as float bit patterns."""
    return np.ascontiguousarray(np.asarray(a).astype(np.int64) & 0xFFFFFFFF, dtype=np.uint32).view(np.float32)


def same(got, want):
    got, want = f32(got), f32(want)
    return (np.ascontiguousarray(got).view(np.uint32) == np.ascontiguousarray(want).view(np.uint32)) | (np.isnan(got) & np.isnan(want))


def same_shift(got, want, cls=None):
    """same(), with the sign of a zero left open on the rows of ZERO_SIGN_OPEN."""
    ok = same(got, want)
    if cls is not None:
        open_rows = np.isin(np.asarray(cls), ZERO_SIGN_OPEN)
        ok |= open_rows[:, None] & (f32(got) == 0) & (f32(want) == 0)
    return ok


def same_half_pair(got, want):
    """Two binary16 codes in one word (oct_encode): equal, or both halves NaN codes."""
    g, w = np.ascontiguousarray(f32(got)).view(np.uint32), np.ascontiguousarray(f32(want)).view(np.uint32)
    ok = np.ones(g.shape, bool)
    for sh in (0, 16):
        a, b = (g >> sh) & 0xFFFF, (w >> sh) & 0xFFFF
        nan = lambda h: ((h & 0x7C00) == 0x7C00) & ((h & 0x3FF) != 0)  # noqa: E731
        ok &= (a == b) | (nan(a) & nan(b))
    return ok


def _unit(rng, k):
    v = rng.normal(size=(k, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _normalize(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def csv_ids():
    """Ids of the material table whose row differs from the default: the rows of the CSV."""
    t = materials.load_table()
    return tuple(int(i) for i in range(128) if not np.array_equal(t[i], materials.default_row()))


def oct_roundtrip(v):
    """A normal as the g-buffer hands it to the reuse pass: through its two binary16 codes (the oracle's helpers)."""
    L = orc.lib()
    v = np.ascontiguousarray(v, np.float32)
    code, out = np.zeros(2, np.uint16), np.zeros(3, np.float32)
    L.orc_unit_oct_encode(orc.fptr(v), orc.fptr(code))
    L.orc_unit_oct_decode(orc.fptr(code), orc.fptr(out))
    return out


AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)


def renderer_normals():
    """The seven normals the renderer produces -- the six voxel faces and the floor's +y -- as the walk returns them and as the
    reuse pass decodes them from the g-buffer."""
    raw = np.concatenate([AXES, AXES[2:3]])
    return np.concatenate([raw, np.array([oct_roundtrip(n) for n in raw], np.float32)])


def _with_dot(rng, n_axis, t):
    """A unit vector whose dot product with the axis-aligned normal is exactly t (the two other products are exact zeros)."""
    a = int(np.argmax(np.abs(n_axis)))
    phi = rng.uniform(0, 2 * np.pi)
    s = np.sqrt(max(0.0, 1.0 - float(t) ** 2))
    o = [k for k in range(3) if k != a]
    v = np.zeros(3, np.float32)
    v[o[0]], v[o[1]] = F32(s * np.cos(phi)), F32(s * np.sin(phi))
    v[a] = F32(t) * n_axis[a]
    return v


def _live_material(rng):
    return rng.uniform(0.05, 0.95, 14).astype(np.float32)


def _spread():
    """Materials the direction classes are crossed with: CSV rows, the all-zero and all-one rows, a mirror, a rough dielectric."""
    t = materials.load_table()
    ids = csv_ids()
    rows = [t[ids[k * len(ids) // 5]].copy() for k in range(5)]
    rows += [np.zeros(14, np.float32), np.ones(14, np.float32)]
    mid = np.full(14, 0.5, np.float32)
    mid[0:3] = (0.8, 0.3, 0.1)
    rows.append(mid)
    return np.array(rows, np.float32)


def _front(rng, n):
    """A direction on n's side, not grazing."""
    while True:
        d = _unit(rng, 1)[0]
        c = float(np.dot(d, n))
        if abs(c) > 0.05:
            return d if c > 0 else (-d).astype(np.float32)


class _Rows:
    def __init__(self, width_names):
        self.cols = {k: [] for k in width_names}
        self.cls = []

    def add(self, cls, **kw):
        assert set(kw) == set(self.cols)
        for k, v in kw.items():
            self.cols[k].append(np.asarray(v))
        self.cls.append(cls)

    def done(self, dtypes):
        out = {k: np.ascontiguousarray(np.array(v), dtype=dtypes.get(k, np.float32)) for k, v in self.cols.items()}
        out["cls"] = np.array(self.cls)
        return out


GRAZING = {"1e-7": (1e-7, -1e-7), "1e-5": (np.nextafter(F32(1e-5), F32(0)), F32(1e-5), np.nextafter(F32(1e-5), F32(1)),
                                           -np.nextafter(F32(1e-5), F32(0)), -F32(1e-5), -np.nextafter(F32(1e-5), F32(1))),
           "1e-3": (1e-3,)}


@functools.lru_cache(maxsize=None)
def edge_bsdf_rows():
    """Material classes (each parameter at the ends of its range, every CSV row) and direction classes (the renderer's normals, the
    ortho_basis branch boundary, grazing n.l and n.v, coincident / opposite / mirrored directions, either below the surface, every
    lobe code): ROWS_PER_CLASS rows each, NAN_ROWS for the classes of NAN_CLASSES."""
    rng = np.random.default_rng([20240901, 1])
    R = _Rows(["mat", "v", "n", "l", "lobe"])
    table = materials.load_table()

    def generic(cls, mat_of, k=ROWS_PER_CLASS):
        for j in range(k):
            n = _unit(rng, 1)[0] if j % 2 else AXES[rng.integers(0, 6)]
            R.add(cls, mat=mat_of(j), v=_front(rng, n), n=n, l=_front(rng, n), lobe=LOBE_CODES[j % 4])

    for i in csv_ids():
        def row(j, i=i):
            m = table[i].copy()
            if j % 2:
                m[0:3] = rng.integers(0, 256, 3) / F32(255.0)          # a voxel's colour instead of the table's white
            return m
        generic(f"mat/csv_{i}", row)
    generic("mat/all_zero", lambda j: np.zeros(14, np.float32))
    generic("mat/all_one", lambda j: np.ones(14, np.float32))

    def pinned(**pins):
        def row(j):
            m = _live_material(rng)
            for name, val in pins.items():
                if name == "base":
                    m[0:3] = val
                else:
                    m[COL[name]] = val
            return m
        return row
    for name in ("roughness", "metallic"):
        for val in (0, 1):
            generic(f"mat/{name}_{val}", pinned(**{name: val}))
    for val in (0, 1):
        generic(f"mat/anisotropic_{val}_roughness_0", pinned(anisotropic=val, roughness=0))
    generic("mat/base_0", pinned(base=0))
    for cc in (0, 1):
        for gl in (0, 1):
            generic(f"mat/clearcoat_{cc}_gloss_{gl}", pinned(clearcoat=cc, clearcoat_gloss=gl))
    generic("mat/specular_0", pinned(specular=0))
    for val in (0, 1):
        generic(f"mat/sheen_1_tint_{val}", pinned(sheen=1, sheen_tint=val))

    spread = _spread()
    mat = lambda j: spread[j % len(spread)]  # noqa: E731
    for j, n in enumerate(renderer_normals()):
        R.add("dir/renderer_normals", mat=mat(j), v=_front(rng, n), n=n, l=_front(rng, n), lobe=LOBE_CODES[j % 4])
    edge = F32(0.9)                                 # ortho_basis: |n.y| > 0.9 picks the other helper axis
    for j, y in enumerate([edge, np.nextafter(edge, F32(1)), np.nextafter(edge, F32(0)), -edge, -np.nextafter(edge, F32(1)), -np.nextafter(edge, F32(0)),
                           np.nextafter(np.nextafter(edge, F32(1)), F32(1)), F32(0.90001)]):
        phi = rng.uniform(0, 2 * np.pi)
        s = np.sqrt(1.0 - float(y) ** 2)
        n = np.array([s * np.cos(phi), y, s * np.sin(phi)], np.float32)
        R.add("dir/ortho_basis_boundary", mat=mat(j), v=_front(rng, n), n=n, l=_front(rng, n), lobe=LOBE_CODES[j % 4])
    for which in ("nl", "nv"):
        for name, vals in GRAZING.items():
            for j in range(ROWS_PER_CLASS if name != "1e-5" else 12):
                n = AXES[j % 6]
                g = _with_dot(rng, n, vals[j % len(vals)])
                o = _front(rng, n)
                R.add(f"dir/{which}_{name}", mat=mat(j), v=o if which == "nl" else g, n=n, l=g if which == "nl" else o, lobe=LOBE_CODES[j % 4])
    for j in range(ROWS_PER_CLASS):
        n = _unit(rng, 1)[0] if j % 2 else AXES[j % 6]
        v = _front(rng, n)
        R.add("dir/l_eq_v", mat=mat(j), v=v, n=n, l=v.copy(), lobe=LOBE_CODES[j % 4])
    for j in range(NAN_ROWS):
        n = _unit(rng, 1)[0] if j % 2 else AXES[j % 6]
        v = _front(rng, n)
        R.add("dir/l_eq_minus_v", mat=mat(j), v=v, n=n, l=(-v).astype(np.float32), lobe=LOBE_CODES[j % 4])
    for j in range(ROWS_PER_CLASS):
        n = _unit(rng, 1)[0] if j % 2 else AXES[j % 6]
        v = _front(rng, n)
        l = (F32(2.0) * F32(np.dot(n, v)) * n - v).astype(np.float32)
        R.add("dir/l_eq_reflect_v", mat=mat(j), v=v, n=n, l=l, lobe=LOBE_CODES[j % 4])
    for cls, sv, sl in (("dir/l_below", 1, -1), ("dir/v_below", -1, 1), ("dir/both_below", -1, -1)):
        for j in range(ROWS_PER_CLASS):
            n = _unit(rng, 1)[0] if j % 2 else AXES[j % 6]
            R.add(cls, mat=mat(j), v=_front(rng, n) * F32(sv), n=n, l=_front(rng, n) * F32(sl), lobe=LOBE_CODES[j % 4])
    for j in range(2 * len(LOBE_CODES)):
        n = _unit(rng, 1)[0] if j % 2 else AXES[j % 6]
        R.add("dir/lobe_codes", mat=_live_material(rng), v=_front(rng, n), n=n, l=_front(rng, n), lobe=LOBE_CODES[j % len(LOBE_CODES)])
    out = R.done({"lobe": np.int32})
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def edge_cone_rows():
    """cone_dir through ortho_basis: the renderer's normals and normals on either side of the branch of ortho_basis."""
    rng = np.random.default_rng([20240901, 2])
    edge = F32(0.9)
    ns = [n for n in renderer_normals()[:7]]
    for y in (edge, np.nextafter(edge, F32(1)), np.nextafter(edge, F32(0)), -edge, -np.nextafter(edge, F32(1)), -np.nextafter(edge, F32(0)), F32(0.90001), F32(0.89999)):
        phi = rng.uniform(0, 2 * np.pi)
        s = np.sqrt(1.0 - float(y) ** 2)
        ns.append(np.array([s * np.cos(phi), y, s * np.sin(phi)], np.float32))
    cls = ["cone/renderer_normals"] * 7 + ["cone/ortho_basis_boundary"] * 8
    # cone cosines: the sun-lit scene's own, 1 (a zero-width cone) and 0 (a hemisphere)
    cos = np.resize(np.array([np.cos(0.05), 1.0, 0.0, 0.5, np.cos(0.0125)], np.float32), len(ns))
    out = dict(cos=cos, n=np.array(ns, np.float32), cls=np.array(cls))
    for a in out.values():
        a.setflags(write=False)
    return out


def camera_pos():
    return np.array(list(host.default_camera(16, 8).pos), np.float32)


def _pack_info(mat_id, rgb):
    return np.uint32(int(mat_id) | (int(rgb[0]) << 8) | (int(rgb[1]) << 16) | (int(rgb[2]) << 24))


def _sample(rng, dst_pos, *, ids=(1, 10, 11, 20, 21, 30, 40, 50, 80)):
    """One unstored sample (21 floats) of the ordinary kind: a reconnection vertex near the destination that faces it, a
    continuation and a visible sun sample."""
    s = np.zeros(21, np.float32)
    s[0:3] = rng.uniform(0, 3, 3)
    d = _unit(rng, 1)[0]
    s[3:6] = dst_pos + d * F32(rng.uniform(0.1, 1.5))
    rn = _unit(rng, 1)[0]
    if np.dot(rn, -d) < 0 and rng.random() < 0.8:
        rn = -rn
    s[6:9] = rn
    s[9:12] = _front(rng, rn)
    s[12:15] = rng.uniform(0, 4, 3)
    s[15:18] = _front(rng, rn)
    s[18] = np.array([_pack_info(rng.choice(ids), rng.integers(0, 256, 3))], np.uint32).view(np.float32)[0]
    s[19] = rng.uniform(0.01, 20)
    s[20] = rng.integers(0, 3) * 10 + rng.integers(0, 3)
    return s


def _shift_row(rng, cam):
    """An ordinary shift: a destination that mostly faces the camera and the sample."""
    dst_pos = rng.uniform(-0.6, 0.6, 3).astype(np.float32)
    s = _sample(rng, dst_pos)
    n = _unit(rng, 1)[0]
    to_rc = _normalize(s[3:6] - dst_pos)
    if rng.random() < 0.8:
        n = _normalize(_normalize(cam - dst_pos) + to_rc + n * F32(0.3))      # sees both the camera and the vertex
    return dict(dst_pos=dst_pos, dst_n=n, dst_mat=rng.uniform(0, 1, 14).astype(np.float32),
                src_pos=(dst_pos + rng.uniform(-0.05, 0.05, 3)).astype(np.float32), sample=s, dst_M=F32(rng.integers(1, 40)))


@functools.lru_cache(maxsize=None)
def edge_shift_rows():
    """Shift classes: the kinds of sample (escape, last vertex, sun sample invisible, emissive), the two geometric tests straddled, a
    coincident vertex, the cached Jacobian term and the destination's M at their special values, a material row outside [0, 1],
    every `lobes` code."""
    rng = np.random.default_rng([20240901, 3])
    cam = camera_pos()
    R = _Rows(["dst_pos", "dst_n", "dst_mat", "src_pos", "sample", "dst_M"])

    def each(cls, edit, k=ROWS_PER_CLASS):
        for j in range(k):
            r = _shift_row(rng, cam)
            edit(r, j)
            R.add(cls, **r)

    def escape(r, j):
        r["sample"][6:9] = 0.0
        d = _normalize(_normalize(cam - r["dst_pos"]) + r["dst_n"] + _unit(rng, 1)[0] * F32(0.5))
        r["sample"][3:6] = d if j % 4 else -d          # rc_pos is a direction; one in four behind the surface
    each("shift/escape", escape)
    each("shift/last_vertex", lambda r, j: r["sample"].__setitem__(slice(9, 12), 0.0))
    each("shift/nee_invisible", lambda r, j: r["sample"].__setitem__(slice(15, 18), 0.0))

    def emissive(r, j):
        r["sample"][18] = np.array([_pack_info(2, rng.integers(0, 256, 3))], np.uint32).view(np.float32)[0]
        if j % 2:
            r["sample"][9:12] = 0.0
    each("shift/emissive", emissive)

    def dst_nl(vals):
        def edit(r, j):     # an axis normal and an ESCAPE sample whose direction has exactly that n.l (odd rows: a vertex at that angle)
            n = AXES[j % 6]
            d = _with_dot(rng, n, vals[j % len(vals)])
            r["dst_n"] = n
            if j % 2 == 0:
                r["sample"][6:9] = 0.0
                r["sample"][3:6] = d
            else:
                r["sample"][3:6] = r["dst_pos"] + d * F32(0.75)
                r["sample"][6:9] = -d
        return edit
    each("shift/dst_nl_0", dst_nl((1e-7, -1e-7, 0.0, -0.0)))
    each("shift/dst_nl_1e-5", dst_nl(GRAZING["1e-5"][:3]), k=12)

    def rc_nl(r, j):
        n = AXES[j % 6]
        t = GRAZING["1e-5"][j % 3]
        r["sample"][6:9] = n
        r["sample"][3:6] = r["dst_pos"] - _with_dot(rng, n, t) * F32(0.5 + 0.25 * (j % 3))    # n . (-l) ~ t
        r["sample"][9:12] = _front(rng, n)
        r["sample"][15:18] = _front(rng, n)
    each("shift/rc_nl_1e-5", rc_nl, k=12)
    each("shift/same_pos", lambda r, j: r["sample"].__setitem__(slice(3, 6), r["dst_pos"]), k=NAN_ROWS)
    for name, val in (("negative", -3.0), ("zero", 0.0), ("inf", np.inf), ("nan", np.nan)):
        each(f"shift/jacobian_term_{name}", lambda r, j, val=val: r["sample"].__setitem__(19, val))

    def out_of_range(r, j):
        col = 3 + j % 10
        r["dst_mat"][col] = (1.5, -0.25, 1.0000001, -1e-9)[j % 4]
    each("shift/material_outside_unit_range", out_of_range)
    for name, val in (("zero", 0.0), ("inf", np.inf), ("nan", np.nan)):
        each(f"shift/dst_M_{name}", lambda r, j, val=val: r.__setitem__("dst_M", F32(val)))
    codes = (0, 1, 2, 9)
    each("shift/lobes", lambda r, j: r["sample"].__setitem__(20, codes[j // 4] * 10 + codes[j % 4]), k=16)
    out = R.done({})
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def edge_misc_rows():
    """Arguments of the single-function ops at their edges: the renderer's normals, the zero vector and near-axis vectors for the
    octahedral code; ids and albedos at the ends and on byte fractions; hash words of all zeros / ones; the tone curve at its segment
    joints, below zero, inf and NaN; reservoirs whose half-precision fields overflow, underflow or hold inf / NaN."""
    rng = np.random.default_rng([20240901, 4])
    tiny = np.array([[1, 1e-7, 0], [0, -1, 1e-7], [1e-7, 0, -1], [1e-20, 1, 1e-20], [-1e-7, -1e-7, 1], [0.5, 0.5, 0], [0.5, -0.5, -1e-7], [1, 1, 1]], np.float64)
    oct_in = np.concatenate([renderer_normals(), np.zeros((1, 3), np.float32), _normalize(tiny), -AXES * F32(0.5)]).astype(np.float32)
    ids = np.array([0, 1, 2, 127, 64, 100, 3, 2, 127, 0, 55, 82], np.int32)
    alb = rng.integers(0, 256, (len(ids), 3)) / 255.0
    alb[0], alb[1], alb[2], alb[3], alb[4] = 0.0, 1.0, 0.999999, 0.5, (1.0 / 255.0, 254.5 / 255.0, 2.0 / 255.0)
    hash_in = np.array([[0, 0, 0], [0xFFFFFFFF] * 3, [1, 0, 0], [0, 1, 0], [0, 0, 1], [0x80000000, 0, 0], [2, 2, 0], [0, 0, 0xFFFFFFFF],
                        [0xFFFFFFFF, 0, 0], [1, 2, 3]], np.uint32)
    j = F32(0.22), F32(0.22 + (1.0 - 0.22) * 0.4)
    uch = np.array([0.0, -0.0, -1.0, 1e-45, j[0], np.nextafter(j[0], F32(0)), np.nextafter(j[0], F32(1)), j[1], np.nextafter(j[1], F32(0)),
                    np.nextafter(j[1], F32(1)), 1.0, 1e30, np.inf, np.nan], np.float32)
    K = 16
    res = np.zeros((K, 23), np.float32)
    for k in range(K):
        res[k, :21] = _sample(rng, np.zeros(3, np.float32))
        res[k, 21], res[k, 22] = rng.integers(1, 40), rng.uniform(0, 60)
    res[0, 21], res[1, 21], res[2, 21], res[3, 21] = 65504.0, 65520.0, 1e9, 0.0            # M: the largest half, the first that rounds to inf
    res[4, 22], res[5, 22], res[6, 22], res[7, 22] = 1e-8, 6e-8, np.inf, np.nan              # weight: below the smallest subnormal half
    res[8, 19], res[9, 19], res[10, 19] = np.inf, np.nan, -1.0
    res[11, 20], res[12, 20], res[13, 20] = 99.0, 0.0, 90.0
    res[14, 6:9], res[14, 9:12], res[14, 15:18] = 0.0, 0.0, 0.0
    res[15, 6:9], res[15, 15:18] = AXES[3], AXES[5]
    out = dict(oct_in=oct_in, matenc_id=ids, matenc_albedo=alb.astype(np.float32), hash_in=hash_in, uchimura_in=uch, res_in=res)
    for a in out.values():
        a.setflags(write=False)
    return out


def classes(rows):
    return sorted(set(rows["cls"].tolist()))


# ---- the seeded random set (compared with the oracle) ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_rows(n_bsdf=3000, n_shift=400, seed=20240902):
    """function_vectors' recipe at a larger size: all fourteen material parameters uniform with 15 % at the 0 / 1 extremes, unit
    vectors mostly on the surface's side; shifts with samples of every kind."""
    rng = np.random.default_rng(seed)
    n = n_bsdf
    mats = rng.uniform(0.0, 1.0, (n, 14)).astype(np.float32)
    ext = rng.random((n, 14)) < 0.15
    mats[ext] = rng.integers(0, 2, int(ext.sum())).astype(np.float32)
    nrm, view, lgt = _unit(rng, n), _unit(rng, n), _unit(rng, n)
    flip = (view * nrm).sum(1) < 0
    view[flip & (rng.random(n) < 0.9)] *= -1.0
    flip = (lgt * nrm).sum(1) < 0
    lgt[flip & (rng.random(n) < 0.5)] *= -1.0
    bsdf = dict(mat=mats, v=view, n=nrm, l=lgt, lobe=rng.choice(LOBE_CODES, n).astype(np.int32), cls=np.array(["random"] * n))
    cam = camera_pos()
    R = _Rows(["dst_pos", "dst_n", "dst_mat", "src_pos", "sample", "dst_M"])
    for k in range(n_shift):
        r = _shift_row(rng, cam)
        m = r["dst_mat"]
        e = rng.random(14) < 0.15
        m[e] = rng.integers(0, 2, int(e.sum()))
        s = r["sample"]
        if k % 4 == 0:
            s[6:9] = 0.0
            s[3:6] = _normalize(_normalize(cam - r["dst_pos"]) + r["dst_n"] + _unit(rng, 1)[0])
        if k % 5 == 1:
            s[9:12] = 0.0
        if k % 3 == 2:
            s[15:18] = 0.0
        if k % 7 == 3:
            s[20] = rng.choice((0, 1, 2, 9)) * 10 + rng.choice((0, 1, 2, 9))
        R.add("random", **r)
    shift = R.done({})
    cone = dict(cos=rng.uniform(0.5, 0.99999, 200).astype(np.float32), n=_unit(rng, 200), cls=np.array(["random"] * 200))
    for d in (bsdf, shift, cone):
        for a in d.values():
            a.setflags(write=False)
    return bsdf, cone, shift


# ---- the oracle's answers ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle():
    """The context every shade probe uses: 16x8 frame, max_depth 2, the sun-lit scene, default camera."""
    mat, rgb, params = scenes.scene_sunlit(0)
    o = orc.Oracle(host.make_config(16, 8, max_depth=2), threads=1)
    orc.setup(o, mat, rgb, params)
    return o


def view_vectors(dst_pos):
    """normalize(camera - x1) as the oracle's shift computes it (orc_unit_view)."""
    dst_pos = np.ascontiguousarray(dst_pos, np.float32)
    out = np.zeros_like(dst_pos)
    orc.lib().orc_unit_view(C.c_void_p(oracle()._ctx), len(dst_pos), orc.fptr(dst_pos), orc.fptr(out))
    return out


def oracle_bsdf(rows, draws, seed0=SAMPLE_SEED):
    L, f = orc.lib(), orc.fptr
    n = len(rows["mat"])
    ev, lp, sm = np.zeros((n, 7), np.float32), np.zeros(n, np.float32), np.zeros((n, draws, 8), np.float32)
    for k in range(n):
        a = [np.ascontiguousarray(rows[key][k]) for key in ("mat", "v", "n", "l")]
        L.orc_unit_bsdf_eval(*[f(x) for x in a], f(ev[k]))
        L.orc_unit_lobe_pdf(*[f(x) for x in a], int(rows["lobe"][k]), f(lp[k:k + 1]))
        L.orc_unit_bsdf_sample(f(a[0]), f(a[1]), f(a[2]), C.c_uint32(seed0 + k), draws, f(sm[k]))
    return dict(eval=ev, lobe_pdf=lp, sample=sm)


def oracle_cone(rows, draws, seed=CONE_SEED):
    out = np.zeros((len(rows["cos"]), draws, 3), np.float32)
    for k in range(len(out)):
        orc.lib().orc_unit_sample_cone(C.c_float(float(rows["cos"][k])), orc.fptr(np.ascontiguousarray(rows["n"][k])), C.c_uint32(seed), draws, orc.fptr(out[k]))
    return out


def oracle_shift(rows):
    o, L, f = oracle(), orc.lib(), orc.fptr
    out = np.zeros((len(rows["dst_pos"]), 7), np.float32)
    for k in range(len(out)):
        a = [np.ascontiguousarray(rows[key][k]) for key in ("dst_pos", "dst_n", "dst_mat", "src_pos", "sample")]
        L.orc_unit_shift(C.c_void_p(o._ctx), *[f(x) for x in a], f(out[k]))
    return out


# ---- rows of the probe's ops -------------------------------------------------------------------------------------------------
def _cat(*cols):
    n = len(cols[0])
    return np.ascontiguousarray(np.concatenate([f32(c).reshape(n, -1) for c in cols], axis=1), dtype=np.float32)


def _col(n, value):
    return np.full((n, 1), value, np.float32)


def eval_rows(r, form):
    return _cat(r["mat"], r["v"], r["n"], r["l"], bits(np.full(len(r["mat"]), form)))


def lobe_rows(r, form):
    return _cat(r["mat"], r["v"], r["n"], r["l"], bits(r["lobe"]), bits(np.full(len(r["mat"]), form)))


def sample_rows(r, draws, seed0=SAMPLE_SEED):
    n = len(r["mat"])
    return _cat(r["mat"], r["v"], r["n"], bits(seed0 + np.arange(n)), bits(np.full(n, draws)))


def cone_rows(r, draws, seed=CONE_SEED):
    n = len(r["cos"])
    return _cat(r["cos"], r["n"], bits(np.full(n, seed)), bits(np.full(n, draws)))


def shift_rows(r, view=None):
    view = view_vectors(r["dst_pos"]) if view is None else view
    return _cat(r["dst_pos"], r["dst_n"], r["dst_mat"], r["src_pos"], r["sample"], view, r["dst_M"])


def _report(name, ok, got, want):
    ok = np.asarray(ok).reshape(len(ok), -1).all(axis=1)
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, f"{name}: {bad.size} of {len(ok)} rows differ, first {bad[:4].tolist()}: got {np.asarray(got)[bad[0]].tolist()}, want {np.asarray(want)[bad[0]].tolist()}"


def check_bsdf(run, rows, want, label, draws):
    """The BSDF ops in all three formulations; the sampler (it has one formulation)."""
    for form in FORMS:
        got = run(OP["EVAL"], eval_rows(rows, form), 7)
        _report(f"{label}: evaluation + pdf_all, form {form}", same(got, want["eval"]), got, want["eval"])
        got = run(OP["LOBE_PDF"], lobe_rows(rows, form), 1)[:, 0]
        _report(f"{label}: lobe pdf, form {form}", same(got, want["lobe_pdf"]), got, want["lobe_pdf"])
    got = run(OP["SAMPLE"], sample_rows(rows, draws), 8 * draws).reshape(len(rows["mat"]), draws, 8)
    _report(f"{label}: sample_bsdf", same(got, want["sample"][:, :draws]), got, want["sample"])


def check_cone(run, rows, want, label, draws, seed=CONE_SEED):
    got = run(OP["CONE"], cone_rows(rows, draws, seed), 3 * draws).reshape(len(rows["cos"]), draws, 3)
    _report(f"{label}: cone_dir", same(got, want), got, want)


def check_shift(run, rows, want, label, view=None):
    """diffuse, specular and Jacobian against `want`; shift_jacobian == the Jacobian shift_sample returns, on every row; where
    shift_is_constant says 1, the shift of that row has a zero Jacobian, finite outputs and a finite M >= 0.  Returns the flags."""
    got = run(OP["SHIFT"], shift_rows(rows, view), 9)
    _report(f"{label}: shift", same_shift(got[:, :7], want, rows.get("cls")), got[:, :7], want)
    _report(f"{label}: shift_jacobian vs shift_sample's", same(got[:, 7], got[:, 6]), got[:, 7], got[:, 6])
    flag = got[:, 8]
    assert np.isin(flag, (0.0, 1.0)).all()
    const = flag == 1.0
    M = f32(rows["dst_M"])
    ok = ~const | (((np.ascontiguousarray(want[:, 6]).view(np.uint32) & 0x7FFFFFFF) == 0) & np.isfinite(want[:, :6]).all(axis=1) & np.isfinite(M) & (M >= 0))
    _report(f"{label}: shift_is_constant claims a shift that is not a finite value times a zero Jacobian", ok, got, want)
    return const


def check_reference(run, *, shift=True, bsdf=True):
    """Every row of functions.npz and functions_edges.npz, as the reference's own source computed it."""
    v = np.load(os.path.join(HERE, "golden", "reference", "functions.npz"))
    e = np.load(os.path.join(HERE, "golden", "reference", "functions_edges.npz"))
    rows = dict(mat=v["mat"], v=v["v"], n=v["n"], l=v["l"], lobe=v["lobe"])
    check_bsdf(run, rows, dict(eval=v["eval"], lobe_pdf=v["lobe_pdf"], sample=v["sample"]), "functions.npz", 4)
    check_cone(run, dict(cos=v["cone_cos"], n=v["cone_n"]), v["cone"], "functions.npz", 3)
    eb = edge_bsdf_rows()
    assert_fixture_rows(e, "bsdf", eb, ("mat", "v", "n", "l", "lobe"))
    check_bsdf(run, eb, dict(eval=e["bsdf_eval"], lobe_pdf=e["bsdf_lobe_pdf"], sample=e["bsdf_sample"]), "functions_edges.npz", EDGE_DRAWS)
    ec = edge_cone_rows()
    assert_fixture_rows(e, "cone", ec, ("cos", "n"))
    check_cone(run, ec, e["cone_out"], "functions_edges.npz", EDGE_DRAWS)
    # single functions
    for name, vv in (("functions.npz", v), ("functions_edges.npz", e)):
        got = run(OP["OCT_ENC"], f32(vv["oct_in"]), 1)[:, 0]
        want = (vv["oct_code"].astype(np.uint32)[:, 0] | (vv["oct_code"].astype(np.uint32)[:, 1] << 16)).view(np.float32)
        _report(f"{name}: oct_encode", same_half_pair(got, want), got.view(np.uint32), want.view(np.uint32))
        got = run(OP["OCT_DEC"], want.reshape(-1, 1), 3)
        _report(f"{name}: oct_decode", same(got, vv["oct_out"]), got, vv["oct_out"])
        got = run(OP["MAT_ENC"], _cat(bits(vv["matenc_id"]), vv["matenc_albedo"]), 1)[:, 0]
        _report(f"{name}: pack_material", got.view(np.uint32) == vv["matenc"], got.view(np.uint32), vv["matenc"])
        got = run(OP["HASH3"], vv["hash_in"].view(np.float32), 1)[:, 0]
        _report(f"{name}: hash3", got.view(np.uint32) == vv["hash_out"], got.view(np.uint32), vv["hash_out"])
        got = run(OP["UCHIMURA"], f32(vv["uchimura_in"]).reshape(-1, 1), 1)[:, 0]
        _report(f"{name}: uchimura1", same(got, vv["uchimura_out"]), got, vv["uchimura_out"])
        got = run(OP["RESERVOIR"], f32(vv["res_in"]), 23)
        _report(f"{name}: reservoir round trip", same(got, vv["res_out"]), got, vv["res_out"])
    got = run(OP["ALBEDO"], e["matenc"].view(np.float32).reshape(-1, 1), 3)
    _report("functions_edges.npz: unpack_albedo", same(got, e["albedo_out"]), got, e["albedo_out"])
    # shifts
    old = dict(dst_pos=v["shift_dst_pos"], dst_n=v["shift_dst_n"], dst_mat=v["shift_dst_mat"], src_pos=v["shift_src_pos"], sample=v["shift_sample"],
               dst_M=np.ones(len(v["shift_out"]), np.float32))
    flags = [check_shift(run, old, v["shift_out"], "functions.npz")]
    es = edge_shift_rows()
    assert_fixture_rows(e, "shift", es, ("dst_pos", "dst_n", "dst_mat", "src_pos", "sample", "dst_M"))
    _report("functions_edges.npz: the view vector of the reference's shift", same(view_vectors(es["dst_pos"]), e["shift_view"]), view_vectors(es["dst_pos"]), e["shift_view"])
    flags.append(check_shift(run, es, e["shift_out"], "functions_edges.npz", view=e["shift_view"]))
    return np.concatenate(flags)


def assert_fixture_rows(e, prefix, rows, keys):
    """The fixture was generated from exactly the rows this module builds now."""
    for k in keys:
        a, b = np.ascontiguousarray(e[f"{prefix}_{k}"]), np.ascontiguousarray(rows[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), \
            f"functions_edges.npz was generated from other {prefix} rows than tests/shading.py builds ({k}): run make_reference_vectors.py functions_edges"
    assert e[f"{prefix}_cls"].tolist() == rows["cls"].tolist()


@functools.lru_cache(maxsize=None)
def oracle_random():
    bsdf, cone, shift = random_rows()
    return oracle_bsdf(bsdf, 2), oracle_cone(cone, 3), oracle_shift(shift)


def check_oracle_rows(run):
    bsdf, cone, shift = random_rows()
    wb, wc, ws = oracle_random()
    check_bsdf(run, bsdf, wb, "random rows vs oracle", 2)
    check_cone(run, cone, wc, "random rows vs oracle", 3)
    const = check_shift(run, shift, ws, "random rows vs oracle")
    n = len(const)
    assert 10 * const.sum() >= n and 10 * (~const).sum() >= n, f"{int(const.sum())} of {n} random shifts are constant"


def check_guards(call, not_prepared):
    """call(op, rows, in_stride, out_stride) on a prepared context, not_prepared(...) on one that is not -> the C return code."""
    rows = eval_rows({k: a[:1] for k, a in edge_bsdf_rows().items()}, 0)
    assert call(OP["EVAL"], rows, rows.shape[1], 7) == 0
    assert call(-1, rows, rows.shape[1], 7) == -1 and call(len(OP), rows, rows.shape[1], 7) == -1          # VRT_E_INVALID
    assert call(OP["EVAL"], rows, rows.shape[1] - 1, 7) == -1 and call(OP["EVAL"], rows, rows.shape[1], 6) == -1
    assert call(OP["SHIFT"], rows, rows.shape[1], 9) == -1
    assert call(OP["EVAL"], None, rows.shape[1], 7) == -1
    if not_prepared is not None:
        assert not_prepared(OP["EVAL"], rows, rows.shape[1], 7) == -3                                           # VRT_E_STATE
