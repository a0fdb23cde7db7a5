"""Single shading functions of the device code, compiled for the host (emu_shade_probe, tests/emul/emul.cpp: the row function
vrt_shade_probe runs on the device, vrt_shade_probe.h): every row of tests/golden/reference/functions.npz and functions_edges.npz as
the reference's own source computed it, a larger random set against the oracle's probes, the shift_is_constant property and the
hook's guards -- bit for bit, the BSDF rows in all three formulations of vrt_bsdf.h.  test_classes_are_what_they_claim checks, from
the oracle and the fixtures alone, that the row classes of tests/shading.py are what their names say.  The same checker drives the
device in tests/test_gpu_shade_probe.py."""
import ctypes as C
import os

import numpy as np
import pytest

import emu
import orc
import shading
from voxel_rt2_amd import host, scenes

HERE = os.path.dirname(os.path.abspath(__file__))


def _session(prepare=True):
    mat, rgb, params = scenes.scene_sunlit(0)
    e = emu.Emulated(host.make_config(16, 8, max_depth=2))
    if prepare:
        orc.setup(e, mat, rgb, params)
    return e


def _call(session):
    def call(op, rows, in_stride, out_stride):
        n = 1 if rows is None else len(rows)
        out = np.zeros((n, max(out_stride, 1)), np.float32)
        return emu.lib().emu_shade_probe(C.c_void_p(session._ctx), int(op), n, None if rows is None else orc.fptr(rows), int(in_stride), orc.fptr(out), int(out_stride))
    return call


@pytest.fixture(scope="module")
def run():
    e = _session()

    def run(op, rows, n_out):
        rows = np.ascontiguousarray(rows, np.float32)
        out = np.zeros((len(rows), n_out), np.float32)
        assert emu.lib().emu_shade_probe(C.c_void_p(e._ctx), int(op), len(rows), orc.fptr(rows), rows.shape[1], orc.fptr(out), n_out) == 0
        return out
    yield run
    e.close()


def test_emulated_shading_equals_reference_source(run):
    shading.check_reference(run)


def test_emulated_shading_equals_oracle(run):
    shading.check_oracle_rows(run)


def test_guards():
    e, cold = _session(), _session(prepare=False)
    shading.check_guards(_call(e), _call(cold))
    e.close()
    cold.close()


def test_classes_are_what_they_claim():
    """Conditions on the rows themselves, from the oracle and the reference fixture alone (nothing here runs the code under test)."""
    v = np.load(os.path.join(HERE, "golden", "reference", "functions.npz"))
    e = np.load(os.path.join(HERE, "golden", "reference", "functions_edges.npz"))
    eb, es, ec = shading.edge_bsdf_rows(), shading.edge_shift_rows(), shading.edge_cone_rows()
    # every class the issue lists is there, with its minimum number of rows
    names = set(shading.classes(eb)) | set(shading.classes(es)) | set(shading.classes(ec))
    want = {f"mat/csv_{i}" for i in shading.csv_ids()} | {"mat/all_zero", "mat/all_one", "mat/roughness_0", "mat/roughness_1", "mat/metallic_0", "mat/metallic_1",
            "mat/anisotropic_0_roughness_0", "mat/anisotropic_1_roughness_0", "mat/base_0", "mat/clearcoat_0_gloss_0", "mat/clearcoat_0_gloss_1",
            "mat/clearcoat_1_gloss_0", "mat/clearcoat_1_gloss_1", "mat/specular_0", "mat/sheen_1_tint_0", "mat/sheen_1_tint_1",
            "dir/renderer_normals", "dir/ortho_basis_boundary", "dir/nl_1e-7", "dir/nl_1e-5", "dir/nl_1e-3", "dir/nv_1e-7", "dir/nv_1e-5", "dir/nv_1e-3",
            "dir/l_eq_v", "dir/l_eq_minus_v", "dir/l_eq_reflect_v", "dir/l_below", "dir/v_below", "dir/both_below", "dir/lobe_codes",
            "shift/escape", "shift/last_vertex", "shift/nee_invisible", "shift/emissive", "shift/dst_nl_0", "shift/dst_nl_1e-5", "shift/rc_nl_1e-5",
            "shift/same_pos", "shift/jacobian_term_negative", "shift/jacobian_term_zero", "shift/jacobian_term_inf", "shift/jacobian_term_nan",
            "shift/material_outside_unit_range", "shift/dst_M_zero", "shift/dst_M_inf", "shift/dst_M_nan", "shift/lobes",
            "cone/renderer_normals", "cone/ortho_basis_boundary"}
    assert len(shading.csv_ids()) == 18
    assert want <= names, sorted(want - names)
    for rows in (eb, es):
        for c in shading.classes(rows):
            assert (rows["cls"] == c).sum() >= shading.ROWS_PER_CLASS, c
    assert (ec["cls"] == "cone/ortho_basis_boundary").sum() >= shading.ROWS_PER_CLASS
    # the classes are what their names say
    nl, nv = (eb["n"] * eb["l"]).sum(1), (eb["n"] * eb["v"]).sum(1)
    for which, dot in (("nl", nl), ("nv", nv)):
        for name, vals in shading.GRAZING.items():
            got = set(np.float32(x).item() for x in dot[eb["cls"] == f"dir/{which}_{name}"])
            assert got == set(np.float32(x).item() for x in vals), (which, name, got)
    assert (nl[eb["cls"] == "dir/l_below"] < 0).all() and (nv[eb["cls"] == "dir/l_below"] > 0).all()
    assert (nv[eb["cls"] == "dir/v_below"] < 0).all() and (nl[eb["cls"] == "dir/v_below"] > 0).all()
    assert (nv[eb["cls"] == "dir/both_below"] < 0).all() and (nl[eb["cls"] == "dir/both_below"] < 0).all()
    assert set(eb["lobe"][eb["cls"] == "dir/lobe_codes"].tolist()) == set(shading.LOBE_CODES)
    ob = np.abs(eb["n"][eb["cls"] == "dir/ortho_basis_boundary"][:, 1])
    assert (ob > np.float32(0.9)).any() and (ob <= np.float32(0.9)).any() and (ob == np.float32(0.9)).any()
    s = es["sample"]
    zero = lambda a: (a * a).sum(1) < 1e-7  # noqa: E731
    assert zero(s[es["cls"] == "shift/escape", 6:9]).all() and zero(s[es["cls"] == "shift/last_vertex", 9:12]).all()
    assert zero(s[es["cls"] == "shift/nee_invisible", 15:18]).all()
    assert ((np.ascontiguousarray(s[es["cls"] == "shift/emissive", 18]).view(np.uint32) & 255) == 2).all()
    lobes = set(int(x) for x in s[es["cls"] == "shift/lobes", 20])
    assert lobes == {a * 10 + b for a in (0, 1, 2, 9) for b in (0, 1, 2, 9)}
    out = es["dst_mat"][es["cls"] == "shift/material_outside_unit_range", 3:13]
    assert ((out < 0) | (out > 1)).any(axis=1).all()
    # every lobe is drawn by the sampler, in the reference's rows and in the oracle's
    wb, wc, ws = shading.oracle_random()
    for smp in (v["sample"], e["bsdf_sample"], wb["sample"]):
        assert {int(x) for x in smp[..., 7].ravel()} == {0, 1, 2}
    # no op was only ever asked for zeros or NaNs: a quarter of its rows at least have a result that is neither
    live = lambda a: (np.nan_to_num(np.asarray(a, np.float64).reshape(len(a), -1), nan=0.0, posinf=1.0, neginf=1.0) != 0).any(axis=1)  # noqa: E731
    for name, a in (("eval", e["bsdf_eval"]), ("lobe_pdf", e["bsdf_lobe_pdf"]), ("sample", e["bsdf_sample"]), ("cone", e["cone_out"]), ("shift", e["shift_out"][:, :6]),
                    ("oct", e["oct_out"]), ("albedo", e["albedo_out"]), ("hash", e["hash_out"]), ("uchimura", e["uchimura_out"]), ("reservoir", e["res_out"]),
                    ("random eval", wb["eval"][:, :6]), ("random lobe_pdf", wb["lobe_pdf"]), ("random sample", wb["sample"]), ("random cone", wc),
                    ("random shift", ws[:, :6])):
        assert 4 * live(a).sum() >= len(a), (name, int(live(a).sum()), len(a))
    # shifts: at least a tenth can be constant (a zero Jacobian) and at least a tenth must be evaluated, in each set
    for name, out in (("edges", e["shift_out"]), ("random", ws)):
        z = (np.ascontiguousarray(out[:, 6]).view(np.uint32) & 0x7FFFFFFF) == 0
        assert 10 * z.sum() >= len(z) and 10 * (~z).sum() >= len(z), (name, int(z.sum()), len(z))
    # the classes that are there for their NaNs give NaN in the reference
    for c in shading.NAN_CLASSES["bsdf"]:
        sel = eb["cls"] == c
        assert (np.isnan(e["bsdf_eval"][sel]).any(axis=1) | np.isnan(e["bsdf_lobe_pdf"][sel])).sum() >= 10, c
    for c in shading.NAN_CLASSES["shift"]:
        assert np.isnan(e["shift_out"][es["cls"] == c]).any(axis=1).sum() >= 10, c
