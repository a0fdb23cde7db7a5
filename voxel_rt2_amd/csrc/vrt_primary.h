// vrt_primary.h -- the primary vertex of a camera path, shaded per pixel ahead of the pooled launch.
//
// Once a launch's camera-ray records are there (k_primary_records, vrt_pool.h), everything up to and including the set-up of the first
// bounce ray depends on (record, pixel, sample) alone: path_begin_along, the hit rebuilt from the record, the g-buffer, path_shade at
// depth 0, floor_probe and walk_prepare of the bounce ray.  k_primary_vertex (vrt_kernels.hip) does that with one lane a pixel of an
// 8x8 tile -- no pool, no scheduler, every lane at the same depth -- and finishes the paths that end there: sky pixels, emissive
// surfaces, max_depth 1, and bounce rays that have nothing to walk and miss the floor (their escape is shaded with the state still in
// registers).  What the fused samples of a pixel share is made once, ahead of the sample loop: the hit, the g-buffer and the shading
// point of a surface hit (primary_vertex_surf).  A path that goes on is appended to a queue in device memory as a PrimaryCont record, from which the pooled launch's
// BEGIN (the QUEUED instantiation of render_pool_body) resumes it at depth 1; BEGIN sets the bounce ray up again (pool_launch_ray:
// the same functions on the same bits).  Every function called here is the one the pool calls; results do not depend on who
// evaluates them.
//
// The queue is split over the work heads (VRT_WORK_HEADS) like the items of a launch without it: tile t appends to head t % 8, a
// pooled wave pulls from its XCD's head and moves on.  Per head: `cap` continuation records and `left_cap` leftover words.  A
// leftover is a depth-0 work item (u | v << 12 | sample << 28) that the pool takes the way it always did: the samples of a pixel
// whose record does not check out, and continuations that found their head's records full.  left_cap holds every item of the head's
// tiles, so no path is ever dropped; cap may be anything (plan_primary_caps, vrt_plan.h).
#ifndef VRT_PRIMARY_H
#define VRT_PRIMARY_H

#include "vrt_pool.h"

namespace vrt {

enum {  // dwords of a continuation record: the hot words of a slot at depth 1 and the cold line, less what is a constant there
    PV_POS = 0, PV_DIR = 3, PV_THR = 6, PV_RNG = 9,
    PV_IDS = 10,      // pix_u | pix_v << 12 | first_lobe << 24 | sample << 28: pack_ids with the lobe where the depth (1, always) would be
    PV_INVPDF = 11, PV_MAT = 12, PV_PPOS = 13,
    PV_COUNT = 16,                                    // black sun: the light-sample sums are the zeros they began as
    PV_NEE_D = 16, PV_NEE_S = 19, PV_COUNT_SUN = 24   // emitting sun (22 words, rounded up to whole 16-byte stores)
};
template <bool BLACK_SUN> struct PrimaryContWords { static constexpr int count = BLACK_SUN ? (int)PV_COUNT : (int)PV_COUNT_SUN; };
#define VRT_PV_COUNT_STRIDE 32   // uints between the heads' counter pairs (a 128-byte line each): [0] continuations, [1] leftovers appended

struct PrimaryQueue {
    uint32_t* counts;      // [VRT_PV_HEADS][VRT_PV_COUNT_STRIDE], zeroed in stream order ahead of k_primary_vertex
    uint32_t* entries;     // [VRT_PV_HEADS][cap] records
    uint32_t* leftovers;   // [VRT_PV_HEADS][left_cap] items
    uint32_t cap, left_cap;
    unsigned long long* report;   // development builds: [0] paths finished ahead of the pool, [1] paths sent on (or null)
};
#define VRT_PV_HEADS 8   // = VRT_WORK_HEADS (vrt_kernels.h asserts it)

VRT_DEV uint32_t primary_leftover_item(int u, int v, int sample) { return (uint32_t)u | ((uint32_t)v << 12) | ((uint32_t)sample << 28); }

// The closest hit of the camera ray, rebuilt from its record as pool_shade rebuilds it from the slot pool_begin_known filled.
// Returns the state that slot would be in: SLOT_SHADE or SLOT_ESCAPE.
template <int G>
VRT_DEV int primary_vertex_hit(const FrameParams& fp, const SceneData& sc, const PrimaryRecord& rec, Hit& h, TraceStats& ts) {
    hit_init(h);
    const int state = slot_state_after_walk<G>(dm_u2f(rec.x), dm_u2f(rec.ft));
    if (state == SLOT_SHADE) {
        const f3 d = mk3(dm_u2f(rec.dx), dm_u2f(rec.dy), dm_u2f(rec.dz));
        const float ft = dm_u2f(rec.ft);
        if (ft < DM_INF) hit_floor(fp, d, ft, h);
        const uint32_t a = rec.y, b = rec.z;
        TraceOut tr;
        walk_result(d, dm_u2f(rec.x), (int)(int16_t)(a & 0xffffu), (int)(int16_t)(a >> 16), (int)(int16_t)(b & 0xffffu), normal_decode(b >> 20), 0, tr);
        hit_voxel<false, G>(fp, sc, world_to_voxel<G>(fp.camera_pos), d, tr, h, ts);
    }
    return state;
}

// The g-buffer of pixel (u, v), once for all its samples: the four stores path_shade makes at depth 0 for sample 0 (vrt_path.h, the
// same expressions on the same operands -- the camera ray from fp.camera_pos along the record's direction, and its hit).
VRT_DEV void primary_vertex_gbuffer(const FrameParams& fp, const PixelBuffers& out, int u, int v, const PrimaryRecord& rec, const Hit& h) {
    const int local_idx = (v - fp.row0) * fp.W + u;
    const f3 hit_pos = fp.camera_pos + h.closest * mk3(dm_u2f(rec.dx), dm_u2f(rec.dy), dm_u2f(rec.dz));
    const f3 ppos = (h.closest == DM_INF) ? mk3(0.0f) : hit_pos;
    stream_store(&out.gb_normal[local_idx], oct_encode(h.normal));
    stream_store3(&out.gb_position[local_idx], ppos);
    stream_store(&out.gb_mat[local_idx], pack_material(h.mat_id, h.albedo));
    stream_store(&out.gb_depth[local_idx], view_to_screen(xform(fp.view, ppos, 1.0f), fp.proj).z);
}

// The shading point of the pixel's primary vertex, once for all its samples: camera, jitter and scene are the launch's, so the hit, the
// view vector (minus the record's direction, which is every sample's p.d at depth 0) and with them path_surf() are the same for every
// fused sample.  Built only where path_shade treats the hit as a surface (its own test); returns whether it was.
template <class PyrT>
VRT_DEV bool primary_vertex_surf(const SceneData& sc, const PrimaryRecord& rec, const Hit& h, int state, Surf& s) {
    if (!(state == SLOT_SHADE && !h.hit_light && h.closest < DM_INF)) return false;
    path_surf<PyrT>(sc, h, mk3(dm_u2f(rec.dx), dm_u2f(rec.dy), dm_u2f(rec.dz)), s);
    return true;
}

// Sample `sample` of pixel (u, v) from its camera ray's record and hit (primary_vertex_hit) up to where the pool has to take over.
// True: the path goes on -- `p` is what SHADE would have stored at depth 0 (path_store_hot, path_store_cold).  False: it is finished
// and its pixel values are written.  SHARED_SURF: `surf` is the pixel's primary_vertex_surf (read only where that returned true);
// otherwise path_shade builds the shading point for this sample alone.
template <int G, bool BLACK_SUN, bool CULL, bool SHARED_SURF = false, class PyrT>
VRT_DEV bool primary_vertex_sample(const FrameParams& fp, const SceneData& sc, const PyrT& P, const PixelBuffers& out, int u, int v, int sample,
                                   const PrimaryRecord& rec, const Hit& h, int state, Path<false>& p, TraceStats& ts, const Surf* surf = nullptr) {
    path_begin_along(fp, p, u, v, sample, mk3(dm_u2f(rec.dx), dm_u2f(rec.dy), dm_u2f(rec.dz)));
    const int local_idx = (v - fp.row0) * fp.W + u;
    VRT_PV_CLOCK(ts, PVR_BEGIN);
    bool done;   // (STORE = false: the g-buffer is the pixel's, primary_vertex_gbuffer)
    if (state == SLOT_SHADE) {
        done = path_shade<false, HIT_SOMETHING, BLACK_SUN, false, true, SHARED_SURF>(fp, sc, P, out, local_idx, p, h, ts, surf);
        VRT_PV_CLOCK(ts, PVR_SAMPLE);   // (from path_shade's own point behind the shading point: draws, sample_bsdf, the light sample; all of an emissive hit)
    } else done = path_shade<false, HIT_NOTHING, false, false>(fp, sc, P, out, local_idx, p, h, ts);
    if (!done) {
        // pool_launch_ray's test of the bounce ray: one that has nothing to walk and misses the floor is ESCAPE's at once
        const float ft = floor_probe(fp, p.pos, p.d);
        RayWalk w;
        const bool alive = walk_prepare<G, CULL>(world_to_voxel<G>(p.pos), p.d, w, sc.cull);
        VRT_PV_CLOCK(ts, PVR_BOUNCE_RAY);
        if (alive || slot_state_after_walk<G>(w.t, ft) != SLOT_ESCAPE) return true;
        Hit none;
        hit_init(none);
        (void)path_shade<false, HIT_NOTHING, false>(fp, sc, P, out, local_idx, p, none, ts);
    }
    path_finish<false>(fp, sc, out, local_idx, p, ts);
    VRT_PV_CLOCK(ts, PVR_FINISH);   // (the escape's shade and path_finish)
    return false;
}

// A path that goes on, as the record the pool resumes it from.  Not in it: contrib and refl_dist (0 after a primary vertex that
// goes on), sky_primary (0: it found a surface), the depth (1), and primary_albedo: path_finish reads it under a moving camera only, and
// a launch of fused samples -- the only kind that is served -- has none (vrt_pipeline.hip, can_fuse); the pool gets path_begin's value.
template <bool BLACK_SUN>
VRT_DEV void primary_cont_pack(uint32_t* e, const Path<false>& p) {
    e[PV_POS] = dm_f2u(p.pos.x); e[PV_POS + 1] = dm_f2u(p.pos.y); e[PV_POS + 2] = dm_f2u(p.pos.z);
    e[PV_DIR] = dm_f2u(p.d.x); e[PV_DIR + 1] = dm_f2u(p.d.y); e[PV_DIR + 2] = dm_f2u(p.d.z);
    e[PV_THR] = dm_f2u(p.thr.x); e[PV_THR + 1] = dm_f2u(p.thr.y); e[PV_THR + 2] = dm_f2u(p.thr.z);
    e[PV_RNG] = p.rng.s;
    e[PV_IDS] = pack_ids(p.pix_u, p.pix_v, p.first_lobe, p.sample);
    e[PV_INVPDF] = dm_f2u(p.first_invpdf);
    e[PV_MAT] = p.primary_mat_info;
    e[PV_PPOS] = dm_f2u(p.primary_pos.x); e[PV_PPOS + 1] = dm_f2u(p.primary_pos.y); e[PV_PPOS + 2] = dm_f2u(p.primary_pos.z);
    if constexpr (!BLACK_SUN) {
        e[PV_NEE_D] = dm_f2u(p.nee_d.x); e[PV_NEE_D + 1] = dm_f2u(p.nee_d.y); e[PV_NEE_D + 2] = dm_f2u(p.nee_d.z);
        e[PV_NEE_S] = dm_f2u(p.nee_s.x); e[PV_NEE_S + 1] = dm_f2u(p.nee_s.y); e[PV_NEE_S + 2] = dm_f2u(p.nee_s.z);
        e[PV_NEE_S + 3] = 0u; e[PV_NEE_S + 4] = 0u;
        static_assert(PV_NEE_S + 5 == PV_COUNT_SUN, "the record's padding");
    }
}
// BEGIN of the QUEUED instantiation: the slot's hot words and cold line from the record, then the bounce ray (pool_launch_ray), as
// SHADE leaves a path that goes on from depth 0.  Returns the slot's state.
template <int G, bool CULL, bool BLACK_SUN>
VRT_DEV int pool_begin_queued(const FrameParams& fp, const float* cull, const SlotRef& s, uint32_t* cold_line, const uint32_t* e, TraceStats& ts) {
    Path<false> p;
    p.pos = mk3(dm_u2f(e[PV_POS]), dm_u2f(e[PV_POS + 1]), dm_u2f(e[PV_POS + 2]));
    p.d = mk3(dm_u2f(e[PV_DIR]), dm_u2f(e[PV_DIR + 1]), dm_u2f(e[PV_DIR + 2]));
    p.thr = mk3(dm_u2f(e[PV_THR]), dm_u2f(e[PV_THR + 1]), dm_u2f(e[PV_THR + 2]));
    p.contrib = mk3(0.0f);
    p.rng.s = e[PV_RNG];
    const uint32_t ids = e[PV_IDS];
    p.pix_u = (int)(ids & 0xfffu); p.pix_v = (int)((ids >> 12) & 0xfffu);
    p.depth = 1; p.sample = (int)(ids >> 28);
    p.first_lobe = (int)((ids >> 24) & 15u); p.sky_primary = 0;
    p.refl_dist = 0.0f;
    p.first_invpdf = dm_u2f(e[PV_INVPDF]);
    p.primary_mat_info = e[PV_MAT];
    p.primary_pos = mk3(dm_u2f(e[PV_PPOS]), dm_u2f(e[PV_PPOS + 1]), dm_u2f(e[PV_PPOS + 2]));
    p.primary_albedo = mk3(1.0f);
    if constexpr (BLACK_SUN) { p.nee_d = mk3(0.0f); p.nee_s = mk3(0.0f); }
    else {
        p.nee_d = mk3(dm_u2f(e[PV_NEE_D]), dm_u2f(e[PV_NEE_D + 1]), dm_u2f(e[PV_NEE_D + 2]));
        p.nee_s = mk3(dm_u2f(e[PV_NEE_S]), dm_u2f(e[PV_NEE_S + 1]), dm_u2f(e[PV_NEE_S + 2]));
    }
    path_store_cold(cold_line, p);
    path_store_hot(s, p);
    return pool_launch_ray<G, CULL>(fp, cull, s, p.pos, p.d, ts);
}

}  // namespace vrt
#endif
