// vrt_shade_probe.h -- TEST HOOK: one row of arguments through one shading function (vrt_shade_probe, include/vrt_api.h; the host
// build of tests/emul/emul.cpp runs the same function).  Only k_shade_probe and emu_shade_probe call it.  Row layouts: those of the
// oracle's orc_unit_* probes (oracle/orc_api.cpp), integers and bit patterns as float bit patterns; tests/shading.py packs them.
#ifndef VRT_SHADE_PROBE_H
#define VRT_SHADE_PROBE_H

#include "vrt_bsdf.h"
#include "vrt_path.h"
#include "vrt_restir.h"
#include "vrt_temporal.h"

namespace vrt {

enum { SHADE_EVAL = 0,        // mat 14, v, n, l, form                  -> diffuse rgb, specular rgb, pdf_all
       SHADE_LOBE_PDF = 1,    // mat 14, v, n, l, lobe, form            -> pdf of the lobe (PDF_LOBE)
       SHADE_SAMPLE = 2,      // mat 14, v, n, seed, count              -> count x (direction, brdf rgb, pdf, lobe): sample_bsdf, stream (seed, 0, i, 0)
       SHADE_CONE = 3,        // cos_max, n, seed, count                -> count x direction: cone_dir through ortho_basis
       SHADE_OCT_ENCODE = 4, SHADE_OCT_DECODE = 5, SHADE_PACK_MATERIAL = 6, SHADE_UNPACK_ALBEDO = 7, SHADE_HASH3 = 8, SHADE_UCHIMURA = 9,
       SHADE_RESERVOIR = 10,  // sample 21, M, weight                   -> the same 23 after reservoir_encode -> reservoir_decode
       SHADE_SHIFT = 11,      // dst_pos, dst_n, dst_mat 14, src_pos, sample 21, view, dst_M
                              //                                         -> diffuse rgb, specular rgb, jacobian, shift_jacobian, shift_is_constant
       SHADE_OP_COUNT = 12 };
// `form` of the two BSDF ops: which of the three formulations of vrt_bsdf.h evaluates the row
enum { SHADE_FORM_RENDER = 0,   // surf_init + eval_lobes / pdf_all / pdf_lobe: the render kernels
       SHADE_FORM_SHARED = 1,   // surf_set + surf_shared + bsdf_eval_pdf, material-derived terms through the per-id table: the reuse pass
       SHADE_FORM_PRE = 2,      // surf_shared_view + mat_colours + dir_terms + bsdf_eval_pdf_pre: a reconnection vertex from the prepare pass's records
       SHADE_FORM_COUNT = 3 };
#define VRT_SHADE_MAX_DRAWS 16
// floats of the two per-lane tables the SHIFT op looks its two materials up in, by id, as the kernels do: [128][14] + [128][8]
#define VRT_SHADE_LANE_TABLE (128 * 14 + 128 * 8)

VRT_DEV int shade_probe_in_width(int op) {
    const int w[SHADE_OP_COUNT] = {24, 25, 22, 6, 3, 1, 4, 1, 3, 1, 23, 48};
    return (op >= 0 && op < SHADE_OP_COUNT) ? w[op] : -1;
}
// floats out of a row; the two sampling ops: per draw
VRT_DEV int shade_probe_out_width(int op) {
    const int w[SHADE_OP_COUNT] = {7, 1, 8, 3, 1, 3, 1, 3, 1, 1, 23, 9};
    return (op >= 0 && op < SHADE_OP_COUNT) ? w[op] : -1;
}

VRT_DEV Material shade_probe_material(const float* a) { return load_material(a, 0); }
VRT_DEV void shade_probe_sample_in(const float* a, Reservoir& r) {
    r.z.F = mk3(a[0], a[1], a[2]); r.z.rc_pos = mk3(a[3], a[4], a[5]); r.z.rc_normal = mk3(a[6], a[7], a[8]);
    r.z.rc_incident_dir = mk3(a[9], a[10], a[11]); r.z.rc_incident_L = mk3(a[12], a[13], a[14]); r.z.rc_nee_dir = mk3(a[15], a[16], a[17]);
    r.z.rc_mat_info = dm_f2u(a[18]); r.z.jac = a[19]; r.z.lobes = (int)a[20];
}

// eval_lobes(lobe) with pdf_all (pdf_mode PDF_ALL) or pdf_lobe (PDF_LOBE) of one direction, in formulation `form`
VRT_DEV void shade_probe_bsdf(const Material& m, f3 v, f3 n, f3 l, int lobe, int pdf_mode, int form, f3& d, f3& s, float& pdf) {
    if (form == SHADE_FORM_RENDER) {
        Surf a;
        surf_init(a, m, n, v);
        eval_lobes(a, l, lobe, d, s);
        pdf = pdf_mode == PDF_ALL ? pdf_all(a, l) : pdf_lobe(a, l, lobe);
        return;
    }
    float table[8];   // one entry of the per-material-id table (k_mat_derived), read back the way k_gris reads it
    store_mat_derived(table, 0, mat_derive(m), material_unit_range(m));
    f3 tx, ty;
    ortho_basis(n, tx, ty);
    Surf b;
    surf_set(b, m, load_mat_derived(table, 0), n, v, cross3(n, ty), ty);
    const bool all = pdf_mode == PDF_ALL;
    const bool g_d = all || lobe_has(lobe, LOBE_DIFFUSE), g_s = all || lobe_has(lobe, LOBE_SPEC), g_c = all || lobe_has(lobe, LOBE_CLEARCOAT);
    if (form == SHADE_FORM_SHARED) {
        bsdf_eval_pdf(b, surf_shared(b, g_d, g_s, g_c), l, lobe, pdf_mode, d, s, pdf);
    } else {
        const SurfShared cv = surf_shared_view(b, mat_colours(m), g_d, g_s, g_c);
        bsdf_eval_pdf_pre(b, cv, l, dir_terms(b.n, b.tx, b.ty, b.ax, b.ay, l), lobe, pdf_mode, d, s, pdf);
    }
}

// The centre -> neighbour shift of the reuse pass's first tap loop for one (destination, sample) pair, with the data passed the way
// k_gris_prepare / k_gris_classify / k_gris_first pass it: both pixels' records from gris_fill_geo / gris_fill_src, the sample back out of its
// GrisSrc record through gris_load_src, the destination's shading point out of its GrisGeo record as gris_first_term() builds it, the
// classify test on the GrisTest records.  The two materials are looked up by id in `lane` ([128][14] rows, then [128][8] derived
// terms): the sample's row copied from the context's tables, the destination's row -- which need not be a row of the context's
// table -- at another id.
VRT_DEV void shade_probe_shift(const FrameParams& fp, const SceneData& sc, const float* mats_x, const float* a, float* o, float* lane) {
    const f3 dst_pos = mk3(a[0], a[1], a[2]), dst_n = mk3(a[3], a[4], a[5]), src_pos = mk3(a[20], a[21], a[22]), view = mk3(a[44], a[45], a[46]);
    const Material dm = shade_probe_material(a + 6);
    Reservoir smp, none;
    reservoir_init(smp);
    reservoir_init(none);
    shade_probe_sample_in(a + 23, smp);
    smp.M = 1.0f; smp.weight = 1.0f;
    none.M = a[47];
    float* lane_mats = lane;
    float* lane_x = lane + 128 * 14;
    const int rc_row = (int)(smp.z.rc_mat_info & 127u), dst_id = (rc_row + 1) & 127;
    for (int k = 0; k < 14; k++) { lane_mats[14 * rc_row + k] = sc.mats[14 * rc_row + k]; lane_mats[14 * dst_id + k] = a[6 + k]; }
    for (int k = 0; k < 8; k++) lane_x[8 * rc_row + k] = mats_x[8 * rc_row + k];
    store_mat_derived(lane_x, dst_id, mat_derive(dm), material_unit_range(dm));
    SceneData lsc = sc;
    lsc.mats = lane_mats;

    // the source pixel (its sample, its own primary vertex) and the destination pixel (its shading point and M; an empty reservoir)
    GrisGeo sg, dg;
    GrisSrc ss, dsrc;
    bool s_ok, d_ok;
    int id;
    const uint32_t src_mat = (uint32_t)dst_id, dst_mat = (uint32_t)dst_id;
    Material m = material_from_bits(lsc.mats, src_mat, id);
    m.base = dm.base;
    gris_fill_geo(lane_x, dst_n, src_pos, src_mat, m, id, norm3(fp.camera_pos - src_pos), smp.M, sg, s_ok);
    sg.dist = len3(sg.x1 - fp.camera_pos);
    gris_fill_src(fp, lsc, lane_x, smp, ss);
    m = material_from_bits(lsc.mats, dst_mat, id);
    m.base = dm.base;
    gris_fill_geo(lane_x, dst_n, dst_pos, dst_mat, m, id, view, none.M, dg, d_ok);
    dg.dist = len3(dg.x1 - fp.camera_pos);
    gris_fill_src(fp, lsc, lane_x, none, dsrc);
    const GrisTest st = gris_test_record(sg.n, sg.dist, sg.x1, sg.M, s_ok, ss), dt = gris_test_record(dg.n, dg.dist, dg.x1, dg.M, d_ok, dsrc);

    Reservoir center;
    f3 rc_ty, sky_t;
    RcPre pre;
    reservoir_init(center);
    gris_load_src(center, rc_ty, sky_t, pre, ss);
    // gris_first_term(): the neighbour's shading point from its record
    const int nmat_id = (int)(dg.mat & 255u);
    Material nmat = load_material(lsc.mats, nmat_id);
    nmat.base = dg.base;
    Surf nds;
    surf_set(nds, nmat, load_mat_derived(lane_x, nmat_id), dg.n, dg.v, cross3(dg.n, dg.ty), dg.ty);
    SurfShared ndsc;
    ndsc.lambert = dg.lambert; ndsc.sheen_col = dg.sheen_col; ndsc.spec_col = dg.spec_col; ndsc.fv = dg.fv; ndsc.g_v = dg.g_v; ndsc.gc_v = dg.gc_v;
    f3 cd, cs;
    float cjac;
    TraceStats ts;
    stats_zero(ts);
    shift_sample(fp, lsc, lane_x, dg.x1, nds, ndsc, center, rc_ty, sky_t, pre, cd, cs, cjac, ts, 0);
    o[0] = cd.x; o[1] = cd.y; o[2] = cd.z; o[3] = cs.x; o[4] = cs.y; o[5] = cs.z; o[6] = cjac;
    o[7] = shift_jacobian(dt.x1, dt.n, st.rc_pos, st.rc_normal, st.jac);
    o[8] = shift_is_constant(dt.x1, dt.n, dt.dst_ok != 0u, dt.M, st.rc_pos, st.rc_normal, st.jac) ? 1.0f : 0.0f;   // gris_classify_pixel
}

// `a`: the row's arguments; `o`: its results (out_width floats, the sampling ops count x out_width); `lane`: VRT_SHADE_LANE_TABLE
// floats of the lane's own (SHADE_SHIFT only).  The caller has checked op and the strides against the widths above.
VRT_DEV void shade_probe_row(const FrameParams& fp, const SceneData& sc, const float* mats_x, int op, const float* a, float* o, int out_stride, float* lane) {
    switch (op) {
        case SHADE_EVAL: case SHADE_LOBE_PDF: {
            const Material m = shade_probe_material(a);
            const f3 v = mk3(a[14], a[15], a[16]), n = mk3(a[17], a[18], a[19]), l = mk3(a[20], a[21], a[22]);
            f3 d, s;
            float pdf;
            if (op == SHADE_EVAL) {
                shade_probe_bsdf(m, v, n, l, LOBE_ALL, PDF_ALL, (int)dm_f2u(a[23]), d, s, pdf);
                o[0] = d.x; o[1] = d.y; o[2] = d.z; o[3] = s.x; o[4] = s.y; o[5] = s.z; o[6] = pdf;
            } else {
                shade_probe_bsdf(m, v, n, l, (int)dm_f2u(a[23]), PDF_LOBE, (int)dm_f2u(a[24]), d, s, pdf);
                o[0] = pdf;
            }
            break;
        }
        case SHADE_SAMPLE: {
            const Material m = shade_probe_material(a);
            Surf s;
            surf_init(s, m, mk3(a[17], a[18], a[19]), mk3(a[14], a[15], a[16]));
            const uint32_t seed = dm_f2u(a[20]);
            const int count = (int)dm_f2u(a[21]);
            for (int i = 0; i < count && i < VRT_SHADE_MAX_DRAWS && 8 * (i + 1) <= out_stride; i++) {
                dm_rng rng = dm_rng_init(seed, 0u, (uint32_t)i, 0u);
                f3 brdf;
                float pdf;
                int lobe;
                const f3 d = sample_bsdf(s, rng, brdf, pdf, lobe);
                float* q = o + 8 * i;
                q[0] = d.x; q[1] = d.y; q[2] = d.z; q[3] = brdf.x; q[4] = brdf.y; q[5] = brdf.z; q[6] = pdf; q[7] = (float)lobe;
            }
            break;
        }
        case SHADE_CONE: {
            const f3 n = mk3(a[1], a[2], a[3]);
            f3 bx, by;
            ortho_basis(n, bx, by);
            const uint32_t seed = dm_f2u(a[4]);
            const int count = (int)dm_f2u(a[5]);
            for (int i = 0; i < count && i < VRT_SHADE_MAX_DRAWS && 3 * (i + 1) <= out_stride; i++) {
                dm_rng rng = dm_rng_init(seed, 0u, (uint32_t)i, 0u);
                const f3 d = cone_dir(a[0], n, bx, by, rng);
                o[3 * i] = d.x; o[3 * i + 1] = d.y; o[3 * i + 2] = d.z;
            }
            break;
        }
        case SHADE_OCT_ENCODE: o[0] = dm_u2f(oct_encode(mk3(a[0], a[1], a[2]))); break;
        case SHADE_OCT_DECODE: { const f3 d = oct_decode(dm_f2u(a[0])); o[0] = d.x; o[1] = d.y; o[2] = d.z; break; }
        case SHADE_PACK_MATERIAL: o[0] = dm_u2f(pack_material((int)dm_f2u(a[0]), mk3(a[1], a[2], a[3]))); break;
        case SHADE_UNPACK_ALBEDO: { const f3 c = unpack_albedo(dm_f2u(a[0])); o[0] = c.x; o[1] = c.y; o[2] = c.z; break; }
        case SHADE_HASH3: o[0] = dm_u2f(hash3(dm_f2u(a[0]), dm_f2u(a[1]), dm_f2u(a[2]))); break;
        case SHADE_UCHIMURA: o[0] = uchimura1(a[0]); break;
        case SHADE_RESERVOIR: {
            Reservoir r, q;
            reservoir_init(r);
            shade_probe_sample_in(a, r);
            r.M = a[21]; r.weight = a[22];
            const ReservoirRec e = reservoir_encode(r);
            reservoir_init(q);
            reservoir_decode(q, e);
            const f3 f[6] = {q.z.F, q.z.rc_pos, q.z.rc_normal, q.z.rc_incident_dir, q.z.rc_incident_L, q.z.rc_nee_dir};
            for (int k = 0; k < 6; k++) { o[3 * k] = f[k].x; o[3 * k + 1] = f[k].y; o[3 * k + 2] = f[k].z; }
            o[18] = dm_u2f(q.z.rc_mat_info); o[19] = q.z.jac; o[20] = (float)q.z.lobes; o[21] = q.M; o[22] = q.weight;
            break;
        }
        case SHADE_SHIFT: shade_probe_shift(fp, sc, mats_x, a, o, lane); break;
        default: break;
    }
}

}  // namespace vrt
#endif
