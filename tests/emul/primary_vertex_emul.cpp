// primary_vertex_emul.cpp -- TEST TOOLING: emul.cpp plus the render stage as a launch behind k_primary_vertex runs it, on the host.
// What this covers and what it does not: launches of ONE sample (sample index 0; a call of n samples is n launches, as in emul.cpp), one
// pixel at a time -- so the per-pixel functions, the record's packing and the queue's layout and consumption, but neither samples 1-3
// of a fused launch nor the wave's ballot compaction and atomics, which only tests/test_gpu_primary_vertex.py and
// tests/test_gpu_primary_routes.py exercise.  Of the three routes a record that fails its check takes, the `spoil` option here covers
// two in their per-pixel form, for sample 0: the pixel left to the pool as a depth-0 item (`left = live && !known`) and that item begun
// by pool_begin (the `!known` arm of the QUEUED BEGIN, without its record store).  The device test (the development build's hook
// VRT_TEST_SPOIL_RECORDS) covers all three on the wave's own code: the first for samples 0-3 through the ballot compaction and the atomics,
// the second with sample 0's record store and the later samples that find it or do not, and the third, which this file has nothing of:
// the `!known` arm for sample 0 of the SERVED instantiation (VRT_PRIMARY=0 behind a pre-pass).
// Per tile and pixel, tiles in the kernel's order: the camera ray's record (primary_record_walk), the hit rebuilt once a pixel
// (primary_vertex_hit), the sample through primary_vertex_sample; a path that goes on is packed into the queue of head (tile % 8)
// (primary_cont_pack) or, where the head's records are used up, left as a depth-0 item.  Then the queue is consumed head by head
// the way the QUEUED instantiation's BEGIN does -- pool_begin_queued for a record, pool_begin_known for a leftover -- and every slot
// is stepped to its end by the pool's stage functions, as emul.cpp's render_all_pool steps them.
#include <algorithm>
#include "emul.cpp"
#include "../../voxel_rt2_amd/csrc/vrt_primary.h"
#include "../../voxel_rt2_amd/csrc/vrt_plan.h"

template <int G, bool BLACK_SUN>
static void pv_run_slot(Emu* c, const FrameParams& fp, const SceneData& sc, const PixelBuffers& out, const SlotRef& s, uint32_t* cold, int st) {
    GlobalPyramid<G> P;
    P.p = sc.pyr;
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
            st = pool_shade<HIT_SOMETHING, BLACK_SUN>(fp, sc, P, out, s, cold, c->ts);
        } else {
            st = pool_shade<HIT_NOTHING, false, false>(fp, sc, P, out, s, cold, c->ts);
        }
    }
}

struct PvCounts { unsigned long long finished, sent_on, leftovers; };

template <int G, bool BLACK_SUN, bool CULL>
static void pv_render(Emu* c, const FrameParams& fp, const SceneData& sc, const PixelBuffers& out, long long knob_cap, bool spoil, PvCounts& n) {
    GlobalPyramid<G> P;
    P.p = sc.pyr;
    constexpr int PW = PrimaryContWords<BLACK_SUN>::count;
    const uint32_t tag = fp.frame + 1u;
    const int tiles_x = (fp.W + 7) >> 3, tiles = tiles_x * launch_tile_rows(fp);
    const PrimaryCaps caps = plan_primary_caps((unsigned)tiles, 1, knob_cap);
    std::vector<uint32_t> counts(VRT_PV_HEADS * VRT_PV_COUNT_STRIDE, 0u), entries((size_t)VRT_PV_HEADS * caps.cap * PW + 1, 0u),
        leftovers((size_t)VRT_PV_HEADS * caps.left_cap + 1, 0u);
    std::vector<PrimaryRecord> prim((size_t)(fp.row1 - fp.row0) * fp.W);
    for (int tile = 0; tile < tiles; tile++)   // k_primary_records
        for (int in = 0; in < 64; in++) {
            const int u = (tile % tiles_x) * 8 + (in & 7), v = launch_tile_row(fp, tile / tiles_x) + (in >> 3);
            if (!(u < fp.W && v < fp.row1 && launch_renders_row(fp, v) && !outside_render_area(fp, (float)u, (float)v))) continue;
            PrimaryRecord r = primary_record_walk<G, CULL>(fp, P, sc.cull, u, v, tag);
            if (spoil && ((u * 7 + v * 3) % 11) == 0) r.w ^= 1u;   // a record that does not check out: its pixel is left to the pool
            primary_record_store(&prim[(size_t)(v - fp.row0) * fp.W + u], r);
        }
    for (int tile = 0; tile < tiles; tile++) {   // k_primary_vertex
        const unsigned head = (unsigned)tile & (VRT_PV_HEADS - 1u);
        for (int in = 0; in < 64; in++) {
            const int u = (tile % tiles_x) * 8 + (in & 7), v = launch_tile_row(fp, tile / tiles_x) + (in >> 3);
            if (!(u < fp.W && v < fp.row1 && launch_renders_row(fp, v) && !outside_render_area(fp, (float)u, (float)v))) continue;
            const PrimaryRecord rec = primary_record_load(&prim[(size_t)(v - fp.row0) * fp.W + u]);
            bool left = !primary_record_valid(rec, tag);
            if (!left) {
                Hit h;
                const int state = primary_vertex_hit<G>(fp, sc, rec, h, c->ts);
                primary_vertex_gbuffer(fp, out, u, v, rec, h);
                Path<false> p;
                if (primary_vertex_sample<G, BLACK_SUN, CULL>(fp, sc, P, out, u, v, 0, rec, h, state, p, c->ts)) {
                    const uint32_t at = counts[head * VRT_PV_COUNT_STRIDE]++;
                    if (at < caps.cap) { primary_cont_pack<BLACK_SUN>(&entries[((size_t)head * caps.cap + at) * PW], p); n.sent_on++; }
                    else left = true;
                } else n.finished++;
            }
            if (left) {
                const uint32_t at = counts[head * VRT_PV_COUNT_STRIDE + 1]++;
                if (at < caps.left_cap) leftovers[(size_t)head * caps.left_cap + at] = primary_leftover_item(u, v, 0);
                n.leftovers++;
            }
        }
    }
    for (unsigned head = 0; head < VRT_PV_HEADS; head++) {   // BEGIN of the QUEUED instantiation, and the pool behind it
        const uint32_t n_cont = std::min(counts[head * VRT_PV_COUNT_STRIDE], caps.cap), n_left = std::min(counts[head * VRT_PV_COUNT_STRIDE + 1], caps.left_cap);
        for (uint32_t my = 0; my < n_cont + n_left; my++) {
            uint32_t slot[PF_COUNT] = {0}, cold[ColdLine<false>::count] = {0};
            SlotRef s{slot, 1};
            int st;
            if (my < n_cont) st = pool_begin_queued<G, CULL, BLACK_SUN>(fp, sc.cull, s, cold, &entries[((size_t)head * caps.cap + my) * PW], c->ts);
            else {
                const uint32_t item = leftovers[(size_t)head * caps.left_cap + (my - n_cont)];
                const int u = (int)(item & 0xfffu), v = (int)((item >> 12) & 0xfffu), sample = (int)(item >> 28);
                const PrimaryRecord rec = primary_record_load(&prim[(size_t)(v - fp.row0) * fp.W + u]);
                if (primary_record_valid(rec, tag)) st = pool_begin_known<G>(fp, s, u, v, sample, rec);
                else st = pool_begin<G, CULL>(fp, sc.cull, s, u, v, sample, c->ts);
            }
            pv_run_slot<G, BLACK_SUN>(c, fp, sc, out, s, cold, st);
        }
    }
}

template <int G>
static int pv_accumulate(Emu* c, int n_samples, int cull, long long knob_cap, int spoil, PvCounts& n) {
    for (int smp = 0; smp < n_samples; smp++) {   // (accumulate_g of emul.cpp, ReSTIR off, with the render stage above)
        FrameParams fp = frame_params(c);
        SceneData sc;
        memset(&sc, 0, sizeof(sc));
        sc.pyr.l0 = c->l0.data(); sc.pyr.l1 = c->l1.data(); sc.pyr.l2 = c->l2.data(); sc.pyr.l3 = c->l3.data();
        sc.pyr.l0c = c->l0c.data(); sc.pyr.l0c_base = c->l0c_base.data(); sc.pyr.l0c_count = c->l0c_base.data() + 512;
        sc.pyr.ref_oob = 0;
        sc.grid = c->grid.data(); sc.mats = c->mats.data();
        sc.sky.scattering = c->sky_scat.data(); sc.sky.transmittance = c->sky_trans.data();
        sc.sky.res = c->cfg.sky_res; sc.sky.fres = c->cfg.sky_res > 0 ? (float)(1.0 / (double)c->cfg.sky_res) : 0.0f;
        sc.counters = nullptr;
        sc.cull = c->cull + (cull ? 0 : 8);
        PixelBuffers out;
        f3* rt = c->cbuf[c->cidx].data();
        out.color_d = rt; out.color_s = c->color_s.data();
        out.gb_normal = c->gb_normal[c->cur].data(); out.gb_depth = c->gb_depth[c->cur].data();
        out.gb_refl_depth = c->gb_refl.data(); out.gb_position = c->gb_pos.data(); out.gb_mat = c->gb_mat.data();
        out.reservoir = nullptr;
        out.sample_stride = 0;
        const bool black_sun = !((fp.light_color.x != 0.0f || fp.light_color.y != 0.0f || fp.light_color.z != 0.0f) && fp.light_weight != 0.0f);
        if (black_sun) { if (cull) pv_render<G, true, true>(c, fp, sc, out, knob_cap, spoil != 0, n); else pv_render<G, true, false>(c, fp, sc, out, knob_cap, spoil != 0, n); }
        else { if (cull) pv_render<G, false, true>(c, fp, sc, out, knob_cap, spoil != 0, n); else pv_render<G, false, false>(c, fp, sc, out, knob_cap, spoil != 0, n); }
        TemporalBuffers tb;
        tb.color_d = rt; tb.color_s = c->color_s.data();
        tb.gb_normal = out.gb_normal; tb.gb_depth = out.gb_depth; tb.gb_mat = out.gb_mat;
        tb.gb_refl_raw = c->gb_refl.data(); tb.gb_refl_filtered = c->gb_refl_f.data();
        tb.hist_d_in = c->hist_d[c->hist_in].data(); tb.hist_d_out = c->hist_d[c->hist_in ^ 1].data();
        tb.hist_s_in = c->hist_s[c->hist_in].data(); tb.hist_s_out = c->hist_s[c->hist_in ^ 1].data();
        tb.prev_normal = c->gb_normal[c->cur ^ 1].data(); tb.prev_depth = c->gb_depth[c->cur ^ 1].data();
        tb.hdr = c->cbuf[c->cidx ^ 1].data();
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

extern "C" {
// n_samples launches of one sample each behind the primary-vertex kernel.  cull: the scene's culling box, not the open one; knob_cap:
// Knobs::primary_cap (0: the rule's); spoil: every eleventh record fails its check.  counts[3]: paths finished ahead of the pool,
// sent on through the queue, left to the pool as depth-0 items.
int emu_accumulate_primary(Emu* c, int n_samples, int cull, long long knob_cap, int spoil, unsigned long long* counts) {
    if (c->cfg.use_restir || c->cam.render_scale != 1.0f) return VRT_E_INVALID;
    PvCounts n{0ULL, 0ULL, 0ULL};
    const int rc = c->cfg.grid_res == 256 ? pv_accumulate<256>(c, n_samples, cull, knob_cap, spoil, n) : pv_accumulate<128>(c, n_samples, cull, knob_cap, spoil, n);
    counts[0] = n.finished; counts[1] = n.sent_on; counts[2] = n.leftovers;
    return rc;
}
}
