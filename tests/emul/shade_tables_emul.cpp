// shade_tables_emul.cpp -- TEST TOOLING (tests/test_shade_tables.py): the shading terms the render kernels take from a table or a
// shorter form -- the packed material row the pooled kernels stage (pack_material_row / load_material_packed, vrt_path.h), the
// basis of a face normal (ortho_basis_axis_normal, vrt_bsdf.h), a texel byte over 255 (byte_over_255, vrt_types.h) -- beside the
// expressions they stand for, on the host build of the same headers; and the pooled-schedule emulation of emul.cpp run WITH the
// packed rows (`emt_` entry points: emul.cpp's own, except that accumulate renders through a pyramid type that says
// mats_packed and a SceneData whose `mats` is the staged table -- what render_pool_body builds on the device).
#include "emul.cpp"
#include "../../voxel_rt2_amd/csrc/vrt_radiance.h"

namespace {

// GlobalPyramid as the pooled kernels' pyramid types present themselves to path_shade()
template <int G>
struct PackedPyramid : GlobalPyramid<G> { static constexpr bool mats_packed = true; };

// render_pool_body's staging loop: from the derived table when the SceneData has one, else derived in place
void stage_packed(const SceneData& sc, float* staged) {
    for (int id = 0; id < 128; id++) {
        const Material m = load_material(sc.mats, id);
        pack_material_row(staged + MP_COUNT * id, m, sc.mats_x ? load_mat_derived(sc.mats_x, id) : mat_derive(m));
    }
}

// render_all_pool (emul.cpp) without ReSTIR, through pyramid type PyrT
template <int G, class PyrT>
void render_pool_with(Emu* c, const FrameParams& fp, const SceneData& sc, const PixelBuffers& out) {
    PyrT P;
    P.p = sc.pyr;
    const bool black_sun = !((fp.light_color.x != 0.0f || fp.light_color.y != 0.0f || fp.light_color.z != 0.0f) && fp.light_weight != 0.0f);
    for (int v = fp.row0; v < fp.row1; v++)
        for (int u = 0; u < fp.W; u++) {
            if (outside_render_area(fp, (float)u, (float)v)) continue;
            uint32_t slot[PF_COUNT] = {0}, cold[ColdLine<false>::count] = {0};
            SlotRef s{slot, 1};
            int st = pool_begin<G>(fp, sc.cull, s, u, v, 0, c->ts);
            while (st != SLOT_EMPTY) {
                if (st == SLOT_RAY) {
                    RayWalk w;
                    walk_load<G>(s, w);
                    BrickCache bc{-1, 0ULL};
                    CoarseWords cw;
                    coarse_fetch(P, w.ix, w.iy, w.iz, cw);
                    const int iters0 = w.iters;
                    for (int k = 1;; k++) {
                        int nq;
                        const bool fin = walk_trip(P, w, bc, cw, nq);
                        c->ts.queries += (unsigned)nq;
                        if (fin) break;
                        if (k % 3 == 0) { walk_store(s, w); walk_load<G>(s, w); bc.key = -1; coarse_fetch(P, w.ix, w.iy, w.iz, cw); }
                    }
                    c->ts.iters += (unsigned)(w.iters - iters0);
                    walk_store(s, w);
                    st = slot_state_after_walk<G>(w.t, s.f(PF_FLOOR_T));
                } else if (st == SLOT_SHADE) {
                    st = black_sun ? pool_shade<HIT_SOMETHING, true>(fp, sc, P, out, s, cold, c->ts)
                                   : pool_shade<HIT_SOMETHING, false>(fp, sc, P, out, s, cold, c->ts);
                } else {
                    st = pool_shade<HIT_NOTHING, false, false>(fp, sc, P, out, s, cold, c->ts);
                }
            }
        }
}

// accumulate_g (emul.cpp) for a context without ReSTIR at full render scale, the render stage through the packed rows.
// table: 0 = the staged rows come from the derived table (SceneData::mats_x set), 1 = the SceneData has none (derived while staging)
template <int G>
int accumulate_packed(Emu* c, int n_samples, int table) {
    if (c->cfg.use_restir || c->cam.render_scale != 1.0f) return VRT_E_INVALID;
    for (int smp = 0; smp < n_samples; smp++) {
        FrameParams fp = frame_params(c);
        SceneData sc{};   // (mats_x: null unless set below)
        sc.pyr.l0 = c->l0.data(); sc.pyr.l1 = c->l1.data(); sc.pyr.l2 = c->l2.data(); sc.pyr.l3 = c->l3.data();
        sc.pyr.l0c = c->l0c.data(); sc.pyr.l0c_base = c->l0c_base.data(); sc.pyr.l0c_count = c->l0c_base.data() + 512;
        sc.pyr.ref_oob = c->ref_oob ? 1 : 0;
        sc.grid = c->grid.data(); sc.mats = c->mats.data();
        sc.sky.scattering = c->sky_scat.data(); sc.sky.transmittance = c->sky_trans.data();
        sc.sky.res = c->cfg.sky_res; sc.sky.fres = c->cfg.sky_res > 0 ? (float)(1.0 / (double)c->cfg.sky_res) : 0.0f;
        sc.counters = nullptr;
        sc.cull = c->cull + 8;
        if (table == 0) {
            if (c->mats_x.empty()) derive_materials(c);
            sc.mats_x = c->mats_x.data();
        }
        float staged[128 * MP_COUNT];
        stage_packed(sc, staged);
        SceneData scl = sc;
        scl.mats = staged;
        PixelBuffers out;
        f3* rt = c->cbuf[c->cidx].data();
        f3* hdr = c->cbuf[c->cidx ^ 1].data();
        out.color_d = rt; out.color_s = c->color_s.data();
        out.gb_normal = c->gb_normal[c->cur].data(); out.gb_depth = c->gb_depth[c->cur].data();
        out.gb_refl_depth = c->gb_refl.data(); out.gb_position = c->gb_pos.data(); out.gb_mat = c->gb_mat.data();
        out.reservoir = c->res[0].data();
        out.sample_stride = 0;
        render_pool_with<G, PackedPyramid<G>>(c, fp, scl, out);
        TemporalBuffers tb;
        tb.color_d = rt; tb.color_s = c->color_s.data();
        tb.gb_normal = out.gb_normal; tb.gb_depth = out.gb_depth; tb.gb_mat = out.gb_mat;
        tb.gb_refl_raw = c->gb_refl.data(); tb.gb_refl_filtered = c->gb_refl_f.data();
        tb.hist_d_in = c->hist_d[c->hist_in].data(); tb.hist_d_out = c->hist_d[c->hist_in ^ 1].data();
        tb.hist_s_in = c->hist_s[c->hist_in].data(); tb.hist_s_out = c->hist_s[c->hist_in ^ 1].data();
        tb.prev_normal = c->gb_normal[c->cur ^ 1].data(); tb.prev_depth = c->gb_depth[c->cur ^ 1].data();
        tb.hdr = hdr;
        tb.sample_stride = 0;
        tb.prev_view = c->prev_view; tb.prev_proj = c->prev_proj;
        tb.tile = nullptr; tb.tile_row0 = 0;
        for (int v = c->own0; v < c->own1; v++)
            for (int u = 0; u < fp.W; u++) temporal_pixel(fp, tb, u, v, 1);
        c->hist_in ^= 1;
        c->cur ^= 1;
        c->cidx ^= 1;
        c->frame += 1;
    }
    return 0;
}

int g_table_mode = 0;   // accumulate_packed's `table` for emt_accumulate (emt_set_table_mode)

}  // namespace

extern "C" {

// ---- the session ABI under the prefix `emt_`: emul.cpp's, with the packed-row render stage ----
Emu* emt_create(const vrt_config* cfg) { return emu_create(cfg); }
void emt_destroy(Emu* c) { emu_destroy(c); }
int emt_upload_voxels(Emu* c, const int8_t* mat, const uint8_t* rgb) { return emu_upload_voxels(c, mat, rgb); }
int emt_upload_materials(Emu* c, const float* t) { return emu_upload_materials(c, t); }
int emt_upload_cloud_texture(Emu* c, const uint8_t* rgb) { return emu_upload_cloud_texture(c, rgb); }
int emt_set_scene(Emu* c, const vrt_scene_params* s) { return emu_set_scene(c, s); }
int emt_set_camera(Emu* c, const vrt_camera* cam) { return emu_set_camera(c, cam); }
int emt_prepare(Emu* c) { return emu_prepare(c); }
int emt_reset(Emu* c) { return emu_reset(c); }
int emt_end_frame(Emu* c) { return emu_end_frame(c); }
int emt_fetch_hdr(Emu* c, float* out) { return emu_fetch_hdr(c, out); }
int emt_fetch_ldr(Emu* c, float* out) { return emu_fetch_ldr(c, out); }
int emt_fetch_buffer(Emu* c, int which, void* out) { return emu_fetch_buffer(c, which, out); }
int emt_get_stats(Emu* c, vrt_stats* s) { return emu_get_stats(c, s); }
void emt_set_table_mode(int table) { g_table_mode = table; }
int emt_accumulate(Emu* c, int n_samples) {
    return c->cfg.grid_res == 256 ? accumulate_packed<256>(c, n_samples, g_table_mode) : accumulate_packed<128>(c, n_samples, g_table_mode);
}

// ---- the pieces, beside the expressions they stand for --------------------------------------------------------------------
// rows: n raw material rows of 14 floats.  got: per row the eight raw columns and the six derived values as path_shade() reads them
// from the row's packed form (table = 0: through the [8]-float derived table entry, as staged on the device; 1: derived while
// staging); want: the same fourteen from load_material() and mat_derive() of the raw row.
void emt_packed_rows(int n, const float* rows, int table, float* got, float* want) {
    for (int i = 0; i < n; i++) {
        const Material m = load_material(rows + 14 * i, 0);
        float entry[8], packed[MP_COUNT];
        store_mat_derived(entry, 0, mat_derive(m), material_unit_range(m));
        pack_material_row(packed, m, table == 0 ? load_mat_derived(entry, 0) : mat_derive(m));
        MatDerived x;
        const Material r = load_material_packed(packed, 0, mk3(0.25f, 0.5f, 0.75f), x);
        const MatDerived w = mat_derive(m);
        const float g[14] = {r.subsurface, r.metallic, r.specular, r.specular_tint, r.roughness, r.sheen, r.sheen_tint, r.clearcoat,
                             x.ax, x.ay, x.cc_alpha, x.w_d, x.w_s, x.w_c};
        const float e[14] = {m.subsurface, m.metallic, m.specular, m.specular_tint, m.roughness, m.sheen, m.sheen_tint, m.clearcoat,
                             w.ax, w.ay, w.cc_alpha, w.w_d, w.w_s, w.w_c};
        memcpy(got + 14 * i, g, sizeof(g));
        memcpy(want + 14 * i, e, sizeof(e));
    }
}
// the 64 normal codes (normal_decode, vrt_pool.h): decoded normal [3], basis from ortho_basis_axis_normal [6] and from ortho_basis [6],
// and whether the short form was taken
void emt_normal_bases(float* normals, float* got, float* want, int* fast) {
    for (uint32_t code = 0; code < 64u; code++) {
        const f3 n = normal_decode(code);
        f3 x, y, rx, ry;
        fast[code] = ortho_basis_axis_normal(n, x, y) ? 1 : 0;
        ortho_basis(n, rx, ry);
        const float nn[3] = {n.x, n.y, n.z}, g[6] = {x.x, x.y, x.z, y.x, y.y, y.z}, e[6] = {rx.x, rx.y, rx.z, ry.x, ry.y, ry.z};
        memcpy(normals + 3 * code, nn, sizeof(nn));
        memcpy(got + 6 * code, g, sizeof(g));
        memcpy(want + 6 * code, e, sizeof(e));
    }
}
// every byte: byte_over_255 beside the division, and the material id hit_voxel() takes beside the reference's round trip
void emt_bytes_over_255(float* got, float* want, int* id_got, int* id_want) {
    for (int k = 0; k < 256; k++) {
        volatile float kf = (float)k;   // (no constant folding of the quotient)
        got[k] = byte_over_255(kf);
        want[k] = kf / 255.0f;
        const uint32_t texel = ((uint32_t)k << 24) | 0x00c0ffeeu;
        id_got[k] = (int)(texel >> 24);   // hit_voxel()'s reading of the alpha byte
        const float a = kf / 255.0f;
        id_want[k] = (int)(a * 255.0f);
    }
}
// Frame constants: for each cos_max[i] and each cos_theta[j], light_cone_pdf() with the quotient in the parameter block (got), with the
// block's field left 0 or holding a NaN (got_unset; -1 where the two differ), and cone_pdf() evaluated in place with a divisor the compiler cannot see through (want); [n][m] each
void emt_cone_pdfs(int n, const float* cos_max, int m, const float* cos_theta, float* got, float* got_unset, float* want) {
    for (int i = 0; i < n; i++) {
        FrameParams fp;
        memset(&fp, 0, sizeof(fp));
        fp.light_cos_max = cos_max[i];
        FrameParams fq = fp;
        fq.light_cone_pdf = cone_pdf_inside(fq.light_cos_max);   // as make_frame_params does (vrt_api.hip)
        for (int j = 0; j < m; j++) {
            volatile float den = DM_TWO_PI * (1.0f - cos_max[i]);
            got[i * m + j] = light_cone_pdf(fq, cos_theta[j]);
            got_unset[i * m + j] = light_cone_pdf(fp, cos_theta[j]);
            FrameParams fn = fp;
            fn.light_cone_pdf = dm_u2f(0x7fc00000u);   // the poison of tests/emul/query_emul.h: as good as unset
            if (dm_f2u(light_cone_pdf(fn, cos_theta[j])) != dm_f2u(got_unset[i * m + j])) got_unset[i * m + j] = -1.0f;
            want[i * m + j] = (cos_theta[j] >= cos_max[i]) ? 1.0f / den : 0.0f;
        }
    }
}
// pixel_texcoord() at full render scale beside the two divisions by render_scale it leaves out, for pixels (u, v)[n] of a W x H frame
void emt_texcoords(int n, const int* uv, int W, int H, float* got, float* want) {
    FrameParams fp;
    memset(&fp, 0, sizeof(fp));
    fp.W = W; fp.H = H;
    fp.inv_res = mk2((float)(1.0 / (double)W), (float)(1.0 / (double)H));
    fp.render_scale = 1.0f;
    volatile float scale = 1.0f;
    for (int i = 0; i < n; i++) {
        const float u = (float)uv[2 * i], v = (float)uv[2 * i + 1];
        const f2 t = pixel_texcoord(fp, u, v);
        got[2 * i] = t.x; got[2 * i + 1] = t.y;
        want[2 * i] = (u + 0.5f) * fp.inv_res.x / scale; want[2 * i + 1] = (v + 0.5f) * fp.inv_res.y / scale;
    }
}
// vrt_trace_radiance's items (radiance_item, vrt_radiance.h) over the context's scene, segment by segment, counting per ray the shaded
// vertices whose normal has two or three non-zero components (a DDA step taken on an exact tie): the vertices that take
// ortho_basis_axis_normal()'s guard.  out: the RADIANCE records vrt_trace_radiance returns (mean rgb, first-hit distance).
int emt_trace_counting_ties(Emu* c, int n, const vrt_path_ray* rays, int n_samples, uint32_t first_frame, vrt_radiance* out, int* ties) {
    if (c->cfg.grid_res != 128 || c->cfg.use_restir) return VRT_E_INVALID;
    const FrameParams fp = frame_params(c);
    SceneData sc{};
    sc.pyr.l0 = c->l0.data(); sc.pyr.l1 = c->l1.data(); sc.pyr.l2 = c->l2.data(); sc.pyr.l3 = c->l3.data();
    sc.pyr.l0c = c->l0c.data(); sc.pyr.l0c_base = c->l0c_base.data(); sc.pyr.l0c_count = c->l0c_base.data() + 512;
    sc.pyr.ref_oob = 0;
    sc.grid = c->grid.data(); sc.mats = c->mats.data();
    sc.sky.scattering = c->sky_scat.data(); sc.sky.transmittance = c->sky_trans.data();
    sc.sky.res = c->cfg.sky_res; sc.sky.fres = c->cfg.sky_res > 0 ? (float)(1.0 / (double)c->cfg.sky_res) : 0.0f;
    sc.counters = nullptr;
    sc.cull = c->cull;   // the grown box, as the library's queries use it
    GlobalPyramid<128> P;
    P.p = sc.pyr;
    for (int i = 0; i < n; i++) {
        ties[i] = 0;
        f3 sum = mk3(0.0f);
        float t_first = DM_INF;
        if (!radiance_ray_valid(rays[i])) return VRT_E_INVALID;
        for (int smp = 0; smp < n_samples; smp++) {
            Path<false> p;
            radiance_begin(fp, p, rays[i], first_frame + (uint32_t)smp);
            TraceStats ts;
            stats_zero(ts);
            for (;;) {   // path_segment (vrt_path.h), its two halves apart
                Hit h;
                next_hit<false>(fp, sc, P, p.pos, p.d, h, ts);
                if (p.depth == 0) t_first = h.closest;
                const bool surface = !h.hit_light && h.closest < DM_INF;
                const int nz = (h.normal.x != 0.0f) + (h.normal.y != 0.0f) + (h.normal.z != 0.0f);
                if (surface && nz >= 2) ties[i]++;
                if (path_shade<false, HIT_ANY, false, false, true>(fp, sc, P, PixelBuffers{}, 0, p, h, ts)) break;
            }
            const f3 value = radiance_value(p);
            sum = radiance_fold(sum, &value, 0, 1);
        }
        const f3 mean = radiance_mean(sum, n_samples);
        out[i].rgb[0] = mean.x; out[i].rgb[1] = mean.y; out[i].rgb[2] = mean.z; out[i].t = t_first;
    }
    return 0;
}
// unpack_albedo() beside its three divisions, for packed words enc[n]
void emt_unpack_albedo(int n, const uint32_t* enc, float* got, float* want) {
    for (int i = 0; i < n; i++) {
        const f3 a = unpack_albedo(enc[i]);
        volatile float r = (float)((enc[i] >> 8) & 255u), g = (float)((enc[i] >> 16) & 255u), b = (float)((enc[i] >> 24) & 255u);
        got[3 * i] = a.x; got[3 * i + 1] = a.y; got[3 * i + 2] = a.z;
        want[3 * i] = r / 255.0f; want[3 * i + 1] = g / 255.0f; want[3 * i + 2] = b / 255.0f;
    }
}

}  // extern "C"
