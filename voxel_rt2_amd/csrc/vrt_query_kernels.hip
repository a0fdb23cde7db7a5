// vrt_query_kernels.hip -- gfx950 kernels of libvrt_hip.so that answer queries against a prepared scene, each with its launcher.
//
//   k_cast_rays                                           vrt_cast_rays: caller-supplied rays through next_hit
//   k_sweep_boxes                                         vrt_sweep_boxes: caller-supplied boxes moved through the pyramid, a wave a box
//   k_trace_radiance                                      vrt_trace_radiance: caller-supplied rays through the path state machine
//   k_gather_irradiance                                   vrt_gather_irradiance: a sun sample and a hemisphere path per (sensor, sample)
//   k_gather_probes                                       vrt_gather_probes: a sun sample and a sphere path per (probe, sample)
//   k_fold_query<Q>                                       the ordered sums of any of the three (vrt_query.h)
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <atomic>
#include "vrt_kernels.h"
#include "vrt_views.h"

namespace vrt {

// ---- the scene queries: what k_cast_rays, k_trace_radiance, k_gather_irradiance and k_gather_probes share -------------------------------------------
// A query kernel's view of the pyramid.  STAGED: the coarse levels in LDS exactly as k_render keeps them for LdsPyramid (at 256^3 the
// 32 KiB l1 level), the fine level through L2, and with MATS the material table beside them as k_render has it; else the launch is small
// and everything is read from global memory.  OOB (STAGED only; GlobalPyramid always can): the instantiation carries the reference's
// reading of cells outside the grid.
template <int G, bool STAGED, bool OOB>
using QueryView = typename std::conditional<STAGED, LdsPyramid<G, OOB>, GlobalPyramid<G>>::type;
// The sizes of the staged levels; the kernel declares the arrays (__shared__ unsigned long long s_l1[STAGED ? N1 : 1] ...: separate
// arrays, not one struct -- as a struct the same bytes cost the 128^3 sampled kernels five registers) and stage_query fills them.
template <int G> struct QueryLds { static constexpr int N1 = GridDim<G>::n1 * GridDim<G>::n1 * GridDim<G>::n1, N2 = GridDim<G>::n2 * GridDim<G>::n2 * GridDim<G>::n2; };
// Called by every thread of the workgroup (it holds the barrier).  Fills the view P, and points scl, the kernel's copy of sc, at what was
// staged.  MATS: the material table too (a cast reads none and hands over a one-element array).  sc by value: through a reference to the
// kernel's argument the unstaged instantiations no longer come out as the code they were with the staging written in the kernel.
template <int G, bool STAGED, bool OOB, bool MATS, int N1, int N2, int NM>
__device__ __forceinline__ void stage_query(const SceneData sc, unsigned long long (&s_l1)[N1], unsigned long long (&s_l2)[N2], float (&s_mats)[NM], float (&s_cull)[8],
                                            QueryView<G, STAGED, OOB>& P, SceneData& scl) {
    if constexpr (STAGED) {
        for (int i = threadIdx.x; i < N1; i += blockDim.x) s_l1[i] = sc.pyr.l1[i];
        if (threadIdx.x < N2) s_l2[threadIdx.x] = sc.pyr.l2[threadIdx.x];
        if (threadIdx.x < 8) s_cull[threadIdx.x] = sc.cull[threadIdx.x];
        if constexpr (MATS) for (int i = threadIdx.x; i < 128 * 14; i += blockDim.x) s_mats[i] = sc.mats[i];
        __syncthreads();
        P.l0 = sc.pyr.l0; P.l1 = s_l1; P.l2 = s_l2;
        P.w3 = (G == 256) ? sc.pyr.l3[0] : 0ULL;
        P.oob = sc.pyr.ref_oob != 0;
        if constexpr (MATS) scl.mats = s_mats;
        scl.cull = s_cull;
    } else {
        P.p = sc.pyr;
    }
}
// A wave's reservation of a sampled query's items, k_render's refill: a wave reserves 64 items at a time from the launch's head word (one
// returning atomic a wave, not one a lane) and hands them to its lanes itself, in lane order.  All three members are wave-uniform.
struct WaveItems {
    bool exhausted = false;         // the launch has no items left
    unsigned next = 0u, end = 0u;   // items [next, end) are reserved for this wave
    // mask: the ballot of the lanes that want an item (need: this lane's bit), not 0, and the launch not exhausted -- the caller tests
    // both (`mask != 0ULL && !items.exhausted && items.take(...)`: with the wave-uniform test in here the compiler lays the loop out
    // differently and k_trace_radiance<256, true, false> takes two more registers).  True on the lanes that got an item: `my` (< total).
    __device__ __forceinline__ bool take(unsigned long long mask, bool need, int lane, unsigned* head, unsigned total, unsigned& my) {
        if (next == end) {
            unsigned base = 0u;
            if (lane == 0) base = atomicAdd(head, 64u);   // (total <= the query's cap of 2^20 items and a grid of a few thousand waves overshoots by 64 each: no wrap)
            base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
            next = base < total ? base : total;
            end = (base + 64u < total) ? base + 64u : total;
            if (base >= total) { exhausted = true; end = next; }
        }
        const unsigned avail = end - next;
        const unsigned n = (unsigned)__popcll(mask);
        const unsigned rank = (unsigned)__popcll(mask & ((1ULL << lane) - 1ULL));
        my = next + rank;
        next += (n < avail) ? n : avail;
        return need && rank < avail;                      // my < end <= total
    }
};

// ---- vrt_cast_rays: caller-supplied rays through next_hit (vrt_cast.h holds the per-ray body) ----------------------------------
// One ray per lane, a grid-stride loop over the batch; the grid is what fits on the chip (plan_cast_blocks), so a workgroup stages
// the pyramid once however many rays it walks (stage_query, without the material table: a cast reads none).
// VRT_RAY_ANY_HIT is a property of a ray, the surface lookup it saves one of the instantiation: a wave whose rays all carry the
// flag runs cast_row<true>; a mixed wave runs cast_row<false> once for all of them and drops the lookup's result on the flagged
// lanes, which is the same record (the walk does not depend on the flag), so no wave walks twice.
template <int G, bool STAGED, bool OOB>
__global__ __launch_bounds__(256) void k_cast_rays(FrameParams fp, SceneData sc, long long n, const vrt_ray* __restrict__ rays, vrt_ray_hit* __restrict__ hits) {
    __shared__ unsigned long long s_l1[STAGED ? QueryLds<G>::N1 : 1];
    __shared__ unsigned long long s_l2[STAGED ? QueryLds<G>::N2 : 1];
    __shared__ float s_mats[1];
    __shared__ float s_cull[8];
    QueryView<G, STAGED, OOB> P;
    SceneData scl = sc;
    stage_query<G, STAGED, OOB, false>(sc, s_l1, s_l2, s_mats, s_cull, P, scl);
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const vrt_ray r = rays[i];
        const bool any = (r.flags & VRT_RAY_ANY_HIT) != 0u;
        vrt_ray_hit h;
        if (__all(any)) {
            cast_row<true>(fp, scl, P, r, h);
        } else {
            cast_row<false>(fp, scl, P, r, h);
            if (any) cast_strip_surface(h);
        }
        hits[i] = h;
    }
}
// ---- vrt_sweep_boxes: caller-supplied boxes moved through the occupancy pyramid (vrt_sweep.h holds everything but the merge) ------------------
// One WAVE per box, four boxes in flight per workgroup, a grid-stride loop over the batch on a grid that fits the chip (plan_sweep_blocks).
// The 64 lanes share the 4x4x4 bricks of the box's candidate region, x fastest, so a wave's l0 loads are neighbours; each lane keeps its
// best candidate as one 64-bit key (sweep_lane), a butterfly of six __shfl_xor steps leaves the smallest on every lane, and lane 0 writes
// the record with ordinary vector stores.  Nothing is staged: a box reads the few l1 words over its region and the l0 words behind their
// set bits once, so there is no reuse for LDS to serve, and no LDS means residency is bounded by registers alone.  The box record is
// read by all 64 lanes from one address (a broadcast load).  Everything a lane branches on outside sweep_lane is wave-uniform.
__global__ __launch_bounds__(256) void k_sweep_boxes(SceneData sc, float floor_height, int G, long long n, const vrt_box_sweep* __restrict__ boxes,
                                                     vrt_sweep_hit* __restrict__ hits) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * VRT_SWEEP_BOXES_PER_BLOCK;
    for (long long i = (long long)blockIdx.x * VRT_SWEEP_BOXES_PER_BLOCK + (threadIdx.x >> 6); i < n; i += stride) {
        const vrt_box_sweep b = boxes[i];
        bool walk;
        SweepKey best = sweep_begin(b, floor_height, walk);
        if (walk) {
            const SweepRegion r = sweep_region(b, G, sc.cull);
            if (!r.empty) best = sweep_lane(b, r, G, sc.pyr.l0, sc.pyr.l1, best, lane, 64, true);
            for (int m = 32; m >= 1; m >>= 1) best = sweep_better(best, __shfl_xor(best, m, 64));
        }
        if (lane == 0) {
            vrt_sweep_hit h;
            sweep_record(best, b, G, h);
            hits[i] = h;
        }
    }
}

// ---- vrt_trace_radiance: caller-supplied rays through the path state machine (vrt_radiance.h holds the per-item body) --------------
// The work item is (ray, sample): item i of a launch is ray i % n_rays, sample s0 + i / n_rays of the block -- a sample's rays side by
// side, so neighbouring lanes start on neighbouring rays, and one ray with 4096 samples fills the chip as 4096 rays with one do.
// A persistent grid (plan_cast_blocks over the items), one Path<false> per lane, k_render's refill (WaveItems): between segments a lane
// whose path ended stores the item's value to plane[i] (every item has exactly one writer: no atomics on results) and takes the next
// item.  Lanes at different depths run side by side.  STAGED / OOB: stage_query's views, with the material table.
// The item of a ray's sample 0 (of the call, not of the chunk) also stores the first hit's distance to out[ray].t; nothing else of `out`
// is written here (rgb carries k_fold_query's running sum).  An invalid ray's items are worth zero and are not traced.
template <int G, bool STAGED, bool OOB>
__global__ __launch_bounds__(256, 2) void k_trace_radiance(FrameParams fp, SceneData sc, unsigned n_rays, unsigned total, unsigned s0, uint32_t first_frame,
                                                           const vrt_path_ray* __restrict__ rays, f3* __restrict__ plane, vrt_radiance* __restrict__ out,
                                                           unsigned* head) {
    __shared__ unsigned long long s_l1[STAGED ? QueryLds<G>::N1 : 1];
    __shared__ unsigned long long s_l2[STAGED ? QueryLds<G>::N2 : 1];
    __shared__ float s_mats[STAGED ? 128 * 14 : 1];
    __shared__ float s_cull[8];
    QueryView<G, STAGED, OOB> P;
    SceneData scl = sc;
    stage_query<G, STAGED, OOB, true>(sc, s_l1, s_l2, s_mats, s_cull, P, scl);
    const int lane = threadIdx.x & 63;
    Path<false> p;
    p.depth = -1;
    unsigned item = 0u;                        // the lane's item while p.depth >= 0
    float t_first = DM_INF;
    TraceStats ts;                             // a sink: a query counts nothing
    stats_zero(ts);
    WaveItems items;
    for (;;) {
        const bool need = p.depth < 0;
        const unsigned long long mask = __ballot(need);
        unsigned my = 0u;
        if (mask != 0ULL && !items.exhausted && items.take(mask, need, lane, head, total, my)) {
            const unsigned ray = my % n_rays, sample = s0 + my / n_rays;
            const vrt_path_ray r = rays[ray];
            if (radiance_ray_valid(r)) {
                item = my;
                radiance_begin(fp, p, r, first_frame + sample);
            } else {
                plane[my] = RadianceQuery::zero();
                if (sample == 0u) out[ray].t = DM_INF;
            }
        }
        if (__ballot(p.depth >= 0) == 0ULL) {
            if (items.exhausted) break;
            continue;
        }
        if (p.depth >= 0) {
            const bool first = p.depth == 0;
            const bool done = radiance_segment(fp, scl, P, p, ts, t_first);
            if (first && item / n_rays + s0 == 0u) out[item % n_rays].t = t_first;
            if (done) {
                plane[item] = radiance_value(p);
                p.depth = -1;
            }
        }
    }
}

// ---- vrt_gather_irradiance: caller-supplied surface points; sun sample and hemisphere path per (sensor, sample) (vrt_sensor.h) ----
// The work item is (sensor, sample): item i of a launch is sensor i % n_sensors, sample s0 + i / n_sensors of the block.  The schedule is
// k_trace_radiance's.  A fresh item has made its four draws (sensor_begin) and waits for its shadow ray; the shadow
// rays of waiting items are walked TOGETHER (sensor_sun) once VRT_SENSOR_SUN_BATCH lanes wait, or when no lane has a path to step, or
// when the launch has no items left -- a refill finds a lane or two a turn, and a walk for them alone would cost the whole wave a
// walk's time.  Waiting lanes sit out the segment step.  The order of walks cannot change a result: an item owns its two random streams.
// Every item has one writer per field of its plane record: the sun terms are stored behind the shadow ray, sky_s at the path's first
// segment, hemi_s at its end; no atomics on results.  An invalid sensor's items, and an item whose derived ray sensor_begin refuses, are
// all zeros and are not traced.
#ifndef VRT_SENSOR_SUN_BATCH
#define VRT_SENSOR_SUN_BATCH 16   // (tools/build_variant.sh NAME -DVRT_SENSOR_SUN_BATCH=1: a shadow walk at every refill; DESIGN.md section 4 says what is known of the choice)
#endif
template <int G, bool STAGED, bool OOB>
__global__ __launch_bounds__(256, 2) void k_gather_irradiance(FrameParams fp, SceneData sc, unsigned n_sensors, unsigned total, unsigned s0, uint32_t first_frame,
                                                              const vrt_sensor* __restrict__ sensors, vrt_irradiance* __restrict__ plane, unsigned* head) {
    __shared__ unsigned long long s_l1[STAGED ? QueryLds<G>::N1 : 1];
    __shared__ unsigned long long s_l2[STAGED ? QueryLds<G>::N2 : 1];
    __shared__ float s_mats[STAGED ? 128 * 14 : 1];
    __shared__ float s_cull[8];
    QueryView<G, STAGED, OOB> P;
    SceneData scl = sc;
    stage_query<G, STAGED, OOB, true>(sc, s_l1, s_l2, s_mats, s_cull, P, scl);
    const int lane = threadIdx.x & 63;
    Path<false> p;
    p.depth = -1;
    unsigned item = 0u;                        // the lane's item while p.depth >= 0
    bool sun_pending = false;                  // the item's shadow ray is still to be walked (then p.depth == 0)
    f3 ldir = mk3(0.0f);                       // ... along ldir, with ndl = dot(ldir, normal)
    float ndl = 0.0f;
    TraceStats ts;                             // a sink: a query counts nothing
    stats_zero(ts);
    WaveItems items;
    for (;;) {
        const bool need = p.depth < 0;
        const unsigned long long mask = __ballot(need);
        unsigned my = 0u;
        if (mask != 0ULL && !items.exhausted && items.take(mask, need, lane, head, total, my)) {
            const unsigned sensor = my % n_sensors, sample = s0 + my / n_sensors;
            const vrt_sensor s = sensors[sensor];
            if (sensor_valid(s) && sensor_begin(fp, p, s, first_frame + sample, ldir, ndl)) {
                item = my;
                sun_pending = true;
            } else {
                plane[my] = SensorQuery::zero();
            }
        }
        const unsigned long long live = __ballot(p.depth >= 0);
        if (live == 0ULL) {
            if (items.exhausted) break;
            continue;
        }
        const unsigned long long waiting = __ballot(sun_pending);   // a subset of `live`
        if (waiting != 0ULL && (__popcll(waiting) >= VRT_SENSOR_SUN_BATCH || waiting == live || items.exhausted)) {
            if (sun_pending) {
                float vis;
                const f3 sun = sensor_sun(fp, scl, P, p.pos, ldir, ndl, ts, vis);
                vrt_irradiance* rec = plane + item;
                rec->sun_rgb[0] = sun.x; rec->sun_rgb[1] = sun.y; rec->sun_rgb[2] = sun.z; rec->sun = vis;
                sun_pending = false;
            }
        }
        if (p.depth >= 0 && !sun_pending) {
            const bool first = p.depth == 0;
            float sky = 0.0f;
            const bool done = sensor_segment(fp, scl, P, p, ts, sky);
            vrt_irradiance* rec = plane + item;
            if (first) rec->sky = sky;
            if (done) {
                const f3 hemi = sensor_value(p);
                rec->sky_rgb[0] = hemi.x; rec->sky_rgb[1] = hemi.y; rec->sky_rgb[2] = hemi.z;
                p.depth = -1;
            }
        }
    }
}

// ---- vrt_gather_probes: caller-supplied points in empty space; sun sample and sphere path per (probe, sample) (vrt_probe_sh.h) ----------
// The work item is (probe, sample): item i of a launch is probe i % n_probes, sample s0 + i / n_probes of the block.  Schedule, refill and
// the shadow rays walked TOGETHER are k_gather_irradiance's (VRT_SENSOR_SUN_BATCH is shared: the same trade); here every item has a shadow
// ray.  The plane holds the compact ProbeItem; the basis and the products are k_fold_query's (probe_fold).  Every item has one writer per
// field of its plane record: w and the pad at the refill, the sun terms behind the shadow ray, sky_s at the path's first segment, L_s at
// its end; no atomics on results.  An invalid probe's items, and an item whose ray probe_begin refuses, are all zeros and are not walked.
template <int G, bool STAGED, bool OOB>
__global__ __launch_bounds__(256, 2) void k_gather_probes(FrameParams fp, SceneData sc, unsigned n_probes, unsigned total, unsigned s0, uint32_t first_frame,
                                                          const vrt_probe* __restrict__ probes, ProbeItem* __restrict__ plane, unsigned* head) {
    __shared__ unsigned long long s_l1[STAGED ? QueryLds<G>::N1 : 1];
    __shared__ unsigned long long s_l2[STAGED ? QueryLds<G>::N2 : 1];
    __shared__ float s_mats[STAGED ? 128 * 14 : 1];
    __shared__ float s_cull[8];
    QueryView<G, STAGED, OOB> P;
    SceneData scl = sc;
    stage_query<G, STAGED, OOB, true>(sc, s_l1, s_l2, s_mats, s_cull, P, scl);
    const int lane = threadIdx.x & 63;
    Path<false> p;
    p.depth = -1;
    unsigned item = 0u;                        // the lane's item while p.depth >= 0 (< total: the plane's bound)
    bool sun_pending = false;                  // the item's shadow ray is still to be walked (then p.depth == 0)
    f3 ldir = mk3(0.0f);                       // ... along ldir
    TraceStats ts;                             // a sink: a query counts nothing
    stats_zero(ts);
    WaveItems items;
    for (;;) {
        const bool need = p.depth < 0;
        const unsigned long long mask = __ballot(need);
        unsigned my = 0u;
        if (mask != 0ULL && !items.exhausted && items.take(mask, need, lane, head, total, my)) {
            const unsigned probe = my % n_probes, sample = s0 + my / n_probes;
            const vrt_probe q = probes[probe];
            f3 w;
            if (probe_valid(q) && probe_begin(fp, p, q, first_frame + sample, ldir, w)) {
                item = my;
                sun_pending = true;
                ProbeItem* rec = plane + my;
                rec->w[0] = w.x; rec->w[1] = w.y; rec->w[2] = w.z; rec->pad = 0.0f;
            } else {
                plane[my] = ProbeQuery::zero();
            }
        }
        const unsigned long long live = __ballot(p.depth >= 0);
        if (live == 0ULL) {
            if (items.exhausted) break;
            continue;
        }
        const unsigned long long waiting = __ballot(sun_pending);   // a subset of `live`
        if (waiting != 0ULL && (__popcll(waiting) >= VRT_SENSOR_SUN_BATCH || waiting == live || items.exhausted)) {
            if (sun_pending) {
                float vis;
                const f3 sun = probe_sun(fp, scl, P, p.pos, ldir, ts, vis);
                ProbeItem* rec = plane + item;
                rec->sun[0] = sun.x; rec->sun[1] = sun.y; rec->sun[2] = sun.z; rec->vis = vis;
                sun_pending = false;
            }
        }
        if (p.depth >= 0 && !sun_pending) {
            const bool first = p.depth == 0;
            float sky = 0.0f;
            const bool done = probe_segment(fp, scl, P, p, ts, sky);
            ProbeItem* rec = plane + item;
            if (first) rec->sky = sky;
            if (done) {
                const f3 L = probe_value(p);
                rec->L[0] = L.x; rec->L[1] = L.y; rec->L[2] = L.z;
                p.depth = -1;
            }
        }
    }
}

// ---- the sampled queries' fold (query_fold, vrt_query.h) -------------------------------------------------------------------------
// One lane per record of the block: the chunk's `count` plane values of the record added in sample order to the sum the chunks before
// left in out[k] (first: to zero), and with the last chunk the division by the call's number of samples.
template <class Q>
__global__ __launch_bounds__(256) void k_fold_query(unsigned n, int count, int first, int last, int n_samples, const typename Q::Item* __restrict__ plane,
                                                    typename Q::Out* __restrict__ out) {
    const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) query_fold<Q>(out[k], plane + k, (long long)n, count, first != 0, last != 0, n_samples);
}

// ---- host-side launchers -----------------------------------------------------------------------
// The ONE place a query launch's (grid_res, staged, oob) becomes an instantiation of its kernel K (CastKernel, ItemKernel<Q>) -- and
// that instantiation's residency, asked once: it depends on nothing a call can change (contexts of one process share the device kind).
template <class K>
static hipError_t query_kernel(int grid_res, bool staged, bool oob, typename K::fn_t* fn, int* per_cu) {
    if (staged) VRT_BY_GRID(grid_res, VRT_BY_2(oob, false, *fn = (K::template get<G, true, A>())));
    else VRT_BY_GRID(grid_res, *fn = (K::template get<G, false, true>()));
    static std::atomic<int> residency[2][3] = {};   // (one table per K)
    std::atomic<int>& cached = residency[grid_res == 256 ? 1 : 0][staged ? (oob ? 2 : 1) : 0];
    *per_cu = cached.load(std::memory_order_relaxed);
    if (*per_cu == 0) {
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, *fn, 256, 0);
        if (e != hipSuccess) return e;
        cached.store(*per_cu, std::memory_order_relaxed);
    }
    return hipSuccess;
}
struct CastKernel {
    typedef void (*fn_t)(FrameParams, SceneData, long long, const vrt_ray*, vrt_ray_hit*);
    template <int G, bool STAGED, bool OOB> static fn_t get() { return k_cast_rays<G, STAGED, OOB>; }
};
template <class Q> struct ItemKernel;   // the kernel that steps Q's items
template <> struct ItemKernel<RadianceQuery> {
    typedef void (*fn_t)(FrameParams, SceneData, unsigned, unsigned, unsigned, uint32_t, const vrt_path_ray*, f3*, vrt_radiance*, unsigned*);
    template <int G, bool STAGED, bool OOB> static fn_t get() { return k_trace_radiance<G, STAGED, OOB>; }
};
template <> struct ItemKernel<SensorQuery> {
    typedef void (*fn_t)(FrameParams, SceneData, unsigned, unsigned, unsigned, uint32_t, const vrt_sensor*, vrt_irradiance*, unsigned*);
    template <int G, bool STAGED, bool OOB> static fn_t get() { return k_gather_irradiance<G, STAGED, OOB>; }
};
template <> struct ItemKernel<ProbeQuery> {
    typedef void (*fn_t)(FrameParams, SceneData, unsigned, unsigned, unsigned, uint32_t, const vrt_probe*, ProbeItem*, unsigned*);
    template <int G, bool STAGED, bool OOB> static fn_t get() { return k_gather_probes<G, STAGED, OOB>; }
};

hipError_t launch_cast_rays(hipStream_t st, int grid_res, bool staged, bool oob, int n_cu, const FrameParams& fp, const SceneData& sc, long long n,
                            const vrt_ray* rays, vrt_ray_hit* hits) {
    CastKernel::fn_t fn = nullptr;
    int per_cu = 0;
    hipError_t e = query_kernel<CastKernel>(grid_res, staged, oob, &fn, &per_cu);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fn, dim3(plan_cast_blocks(n, n_cu, per_cu)), dim3(256), 0, st, fp, sc, n, rays, hits);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
hipError_t launch_sweep_boxes(hipStream_t st, int grid_res, int n_cu, float floor_height, const SceneData& sc, long long n, const vrt_box_sweep* boxes,
                              vrt_sweep_hit* hits) {
    static std::atomic<int> residency{0};   // (asked once: it depends on nothing a call can change)
    int per_cu = residency.load(std::memory_order_relaxed);
    if (per_cu == 0) {
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_sweep_boxes, 256, 0);
        if (e != hipSuccess) return e;
        residency.store(per_cu, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(k_sweep_boxes, dim3(plan_sweep_blocks(n, n_cu, per_cu)), dim3(256), 0, st, sc, floor_height, grid_res, n, boxes, hits);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}

// A sampled query's chunk -- samples [s0, s0 + count) of n records -- worked into `plane` by the query's item kernel and folded into `out`.
// n * count is at most Q::max_items (plan_query_chunk); `head`: the launch's work counter, zeroed here on the stream.
template <class Q>
hipError_t launch_sampled_query(hipStream_t st, int grid_res, bool staged, bool oob, int n_cu, const FrameParams& fp, const SceneData& sc, long long n, int s0,
                                int count, int n_samples, uint32_t first_frame, const typename Q::In* in, typename Q::Item* plane, typename Q::Out* out,
                                unsigned* head) {
    const long long items = n * count;
    if (n < 1 || count < 1 || s0 < 0 || s0 + count > n_samples || items > Q::max_items) return hipErrorInvalidValue;
    typename ItemKernel<Q>::fn_t fn = nullptr;
    int per_cu = 0;
    hipError_t e = query_kernel<ItemKernel<Q>>(grid_res, staged, oob, &fn, &per_cu);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(head, 0, sizeof(unsigned), st);
    if (e != hipSuccess) return e;
    const dim3 grid(plan_cast_blocks(items, n_cu, per_cu));
    if constexpr (std::is_same<Q, RadianceQuery>::value)   // (k_trace_radiance stores the first hit's distance to out[ray].t itself)
        hipLaunchKernelGGL(fn, grid, dim3(256), 0, st, fp, sc, (unsigned)n, (unsigned)items, (unsigned)s0, first_frame, in, plane, out, head);
    else
        hipLaunchKernelGGL(fn, grid, dim3(256), 0, st, fp, sc, (unsigned)n, (unsigned)items, (unsigned)s0, first_frame, in, plane, head);
    VRT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_fold_query<Q>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (unsigned)n, count, s0 == 0 ? 1 : 0,
                       s0 + count == n_samples ? 1 : 0, n_samples, (const typename Q::Item*)plane, out);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
template hipError_t launch_sampled_query<RadianceQuery>(hipStream_t, int, bool, bool, int, const FrameParams&, const SceneData&, long long, int, int, int, uint32_t,
                                                        const vrt_path_ray*, f3*, vrt_radiance*, unsigned*);
template hipError_t launch_sampled_query<SensorQuery>(hipStream_t, int, bool, bool, int, const FrameParams&, const SceneData&, long long, int, int, int, uint32_t,
                                                      const vrt_sensor*, vrt_irradiance*, vrt_irradiance*, unsigned*);
template hipError_t launch_sampled_query<ProbeQuery>(hipStream_t, int, bool, bool, int, const FrameParams&, const SceneData&, long long, int, int, int, uint32_t,
                                                     const vrt_probe*, ProbeItem*, vrt_sh_probe*, unsigned*);

}  // namespace vrt
