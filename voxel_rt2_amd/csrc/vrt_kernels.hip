// vrt_kernels.hip -- gfx950 kernels of libvrt_hip.so: the render launches and the frame passes.  (The scene calls' kernels are in
// vrt_scene_kernels.hip, the queries' in vrt_query_kernels.hip, the test hooks' in vrt_probe_kernels.hip, the sky's in vrt_sky_kernels.hip.)
//
//   k_render_pool / _restir / _dense12                    persistent wave64 path tracer, pooled schedule (vrt_pool.h): a wave owns a
//                                                         pool of path records in LDS and runs them stage by stage (WALK / SHADE /
//                                                         ESCAPE / BEGIN); the default.  Which of them: plan_render_variant, pool_kernel()
//   k_render<RESTIR, INSTR>                               persistent wave64 path tracer, one path per lane (vrt_path.h)
//   k_primary_records / k_primary_vertex / _sun           the camera rays of a pooled launch walked, and its primary vertices shaded, ahead of it
//   k_render_pool_queued                                  the pooled launch behind k_primary_vertex (vrt_primary.h)
//   k_gris_prepare / k_gris                               ReSTIR spatial reuse: per-pixel records (decoded sample, shading
//                                                         basis), then 32 taps x 2 reconnection shifts per pixel
//   k_mat_derived                                         per-material-id part of a shading point (after material uploads)
//   k_temporal                                            fused temporal accumulation -> HDR (sized to run beside
//                                                         the next render launch, see vrt_api.hip)
//   k_temporal_frame_prev                                 the same, moving camera on a row tile with history exchange
//   k_temporal_group                                      the passes of several consecutive launches in one (static camera)
//   k_tonemap                                             LDR presentation
//   k_denoise_prepare / k_denoise_atrous<S>               vrt_denoise: step 1 of every pixel, then an a-trous iteration at stride S
//   k_spoil_primary_records                               -DVRT_DEV_KNOBS builds: camera-ray records made to fail their check (test hook)
//   k_diag_read                                           -DVRT_DIAG_REGIONS builds: this unit's region clocks (g_vrt_region, vrt_types.h)
//
// k_render is a persistent-thread kernel: the grid is sized to the device's residency, each wave
// keeps 64 path records in registers and pulls pixels (8x8 tiles, tile-major order) from a global
// counter.  Between path segments lanes whose path has ended are compacted out with
// __ballot/__popcll and refilled, so the wave's lanes are at different bounce depths but all busy.
// The two coarse brick levels of the pyramid (4 KiB + 64 B) and the material table (7 KiB) are
// staged in LDS once per workgroup; the fine brick level (256 KiB) and the texel grid (8 MiB) stay
// in L2 / Infinity Cache.  Every wave reaches the exit: the loop ends when the counter is exhausted
// and no lane holds a path.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "vrt_kernels.h"
#include "vrt_views.h"

namespace vrt {

// ---- render ----------------------------------------------------------------------------------
// The pooled kernel's view.  128^3: each l1 word beside what the walk needs of its parent l2 word and the l1 cell's fine base
// ({w1, coarse_pack()}[512], vrt_trace.h: one 16-byte LDS read per cell and nothing to evaluate above level 3), and the head of the compacted fine level (Pyramid::l0c) in LDS too -- a sparse scene's fine level is a few
// hundred words, and the fine word is the load every other DDA step depends on (L2: ~700 cycles, LDS: ~130).
// CULL: rays that cannot hit a voxel are not walked (cull_ray, vrt_trace.h).  A launch over a scene whose solids fill the grid
// has nothing to cull and runs the instantiation without the test (its registers cost a dense 4K frame 2.5 %).
template <int G_, bool CULL_, bool SHBR_ = false, bool OOB_ = false>
struct LdsPyramid2 {
    static constexpr int G = G_;
    static constexpr bool cull = CULL_;
    static constexpr bool oob_capable = OOB_;
    bool oob;
    __device__ __forceinline__ bool oob_ref() const { return oob; }
    static constexpr bool flat_descend = true;   // the pooled kernel walks with nearly full waves
    static constexpr bool shadow_branchy = SHBR_;   // ... except SHADE's inline shadow rays in a dense grid (raytrace, vrt_trace.h)
    static constexpr bool mats_packed = true;   // render_pool_body stages packed material rows (pack_material_row, vrt_path.h)
    static constexpr bool coarse_packed = true;   // load_coarse hands out coarse_pack() (vrt_trace.h) and no l2 word
    const unsigned long long* l0;
    const ulonglong2* l1p;             // LDS [512]: {l1 word, coarse_pack() of the l1 cell}
    const unsigned long long* l2;
    const unsigned long long* fine;    // LDS copy of l0c[0 .. n_fine)
    uint32_t n_fine;
    bool all_fine;                     // wave-uniform: n_fine is all the fine words the scene has
    __device__ __forceinline__ unsigned long long load_l0(int i) const { return l0[i]; }
    __device__ __forceinline__ unsigned long long load_l1(int i) const { return l1p[i].x; }
    __device__ __forceinline__ unsigned long long load_l2(int i) const { return l2[i]; }
    __device__ __forceinline__ unsigned long long load_l3() const { return 0ULL; }
    // A scene whose fine words all fit (every sparse one) asks LDS and nothing else.  Otherwise each lane asks the memory
    // its word is in -- as two loads, an LDS and a global one: a single load through a selected generic address is a flat
    // load behind a 64-bit address select.  (The address space is spelled out, or the loads are merged back into that.)
    __device__ __forceinline__ unsigned long long load_fine(int key, uint32_t idx) const {
        const auto staged = (const __attribute__((address_space(3))) unsigned long long*)fine;
        if (all_fine) return staged[idx];
        if (idx < n_fine) return staged[idx];
        return l0[key];
    }
    __device__ __forceinline__ void load_coarse(int i1, int i2, unsigned long long& w1, unsigned long long& w2, uint32_t& packed) const {
        (void)i2; (void)w2;
        const ulonglong2 v = l1p[i1];
        w1 = v.x;
        packed = (uint32_t)v.y;
    }
};
// 256^3: the whole l1 level (16^3 words, 32 KiB) and l2 (4^3 words) resident in LDS -- the brick cache of this grid:
// every coarse query of every DDA step is an LDS read -- the top word in scalar registers, and the fine words (2 MiB:
// they miss LDS by a factor of 13) through L1 / L2 with the current brick's word cached in registers per ray.  A
// workgroup is eight waves (one per CU: eight 13.5 KB path pools + 32.5 KB of pyramid + the material table = 148 KB of
// the CU's 160 KB), so the level is staged once per CU.
template <bool CULL_, bool SHBR_, bool OOB_>
struct LdsPyramid2<256, CULL_, SHBR_, OOB_> {
    static constexpr int G = 256;
    static constexpr bool cull = CULL_;
    static constexpr bool oob_capable = OOB_;
    bool oob;
    __device__ __forceinline__ bool oob_ref() const { return oob; }
    static constexpr bool flat_descend = true;
    static constexpr bool shadow_branchy = SHBR_;
    static constexpr bool mats_packed = true;
    const unsigned long long* l0;
    const unsigned long long* l1;   // LDS [4096]
    const unsigned long long* l2;   // LDS [64]
    unsigned long long w3;
    __device__ __forceinline__ unsigned long long load_l0(int i) const { return l0[i]; }
    __device__ __forceinline__ unsigned long long load_l1(int i) const { return l1[i]; }
    __device__ __forceinline__ unsigned long long load_l2(int i) const { return l2[i]; }
    __device__ __forceinline__ unsigned long long load_l3() const { return w3; }
    __device__ __forceinline__ unsigned long long load_fine(int key, uint32_t idx) const { (void)idx; return l0[key]; }
    __device__ __forceinline__ void load_coarse(int i1, int i2, unsigned long long& w1, unsigned long long& w2, uint32_t& base) const {
        w1 = l1[i1]; w2 = l2[i2];
        base = 0u;
    }
};
#ifndef VRT_POOL_SLOTS_128
#define VRT_POOL_SLOTS_128 VRT_POOL_SLOTS   // (experiments: another pool size at 128^3 only -- the 256^3 workgroup has no LDS to spare)
#endif
// The pooled kernels' two workgroup geometries (render_pool_body): waves (= path pools) per workgroup, slots per pool.
struct PoolShape { int waves, slots; };
template <int G> constexpr PoolShape pool_shape(bool twelve) {
    return twelve ? PoolShape{12, G == 256 ? 88 : 96} : PoolShape{G == 256 ? 8 : VRT_POOL_WAVES, G == 256 ? VRT_POOL_SLOTS : VRT_POOL_SLOTS_128};
}

__device__ __forceinline__ void flush_stats(const TraceStats& ts, Counters* c) {
    // wave-level sum, one atomic per counter per wave
    unsigned v[5] = {ts.rays, ts.iters, ts.queries, ts.closest_hits, ts.sky_lookups};
    unsigned long long* dst[5] = {&c->rays, &c->iters, &c->queries, &c->closest_hits, &c->sky_lookups};
#pragma unroll
    for (int k = 0; k < 5; k++) {
        unsigned long long s = v[k];
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd(dst[k], s);
    }
}

template <int G, bool RESTIR, bool INSTR>
__global__ __launch_bounds__(VRT_RENDER_THREADS, VRT_RENDER_MIN_WAVES) void k_render(FrameParams fp, SceneData sc, PixelBuffers out, unsigned* work_counter, unsigned* next_counter, unsigned chunk, int n_samples) {
    constexpr int N1 = GridDim<G>::n1 * GridDim<G>::n1 * GridDim<G>::n1, N2 = GridDim<G>::n2 * GridDim<G>::n2 * GridDim<G>::n2;
    __shared__ unsigned long long s_l1[N1];
    __shared__ unsigned long long s_l2[N2];
    __shared__ float s_mats[128 * 14];
    __shared__ float s_cull[8];
    for (int i = threadIdx.x; i < N1; i += blockDim.x) s_l1[i] = sc.pyr.l1[i];
    if (threadIdx.x < N2) s_l2[threadIdx.x] = sc.pyr.l2[threadIdx.x];
    if (threadIdx.x < 8) s_cull[threadIdx.x] = sc.cull[threadIdx.x];
    for (int i = threadIdx.x; i < 128 * 14; i += blockDim.x) s_mats[i] = sc.mats[i];
    if (blockIdx.x == 0 && threadIdx.x < VRT_WORK_HEADS) next_counter[threadIdx.x * VRT_WORK_HEAD_STRIDE] = 0u;  // the next launch's heads (idle during this launch)
    if (blockIdx.x == 0 && threadIdx.x == 0) next_counter[1] = 0u;  // and its "drain announced" word
    __syncthreads();
    LdsPyramid<G, INSTR> P;
    P.l0 = sc.pyr.l0; P.l1 = s_l1; P.l2 = s_l2;
    P.w3 = (G == 256) ? sc.pyr.l3[0] : 0ULL;
    P.oob = sc.pyr.ref_oob != 0;
    SceneData scl = sc;
    scl.mats = s_mats;
    scl.cull = s_cull;

    const int lane = threadIdx.x & 63;
    const int tiles_x = (fp.W + 7) >> 3;
    const int tiles_y = launch_tile_rows(fp);
    // work items are (tile, sample, pixel-in-tile), 64 consecutive items = one 8x8 tile of one sample
    const unsigned total = (unsigned)(tiles_x * tiles_y) * 64u * (unsigned)n_samples;

    Path<RESTIR> p;
    p.depth = -1;
    int local_idx = 0;
    TraceStats ts;
    stats_zero(ts);
    bool exhausted = false;               // wave-uniform
    unsigned chunk_next = 0u, chunk_end = 0u;  // wave-uniform: pixels [chunk_next, chunk_end) are reserved for this wave

    for (;;) {
        const bool need = p.depth < 0;
        const unsigned long long mask = __ballot(need);
        if (mask != 0ULL && !exhausted) {
            // One returning atomic on a single word saturates near 88 dequeues/us chip-wide (MI355X_MICROARCH.md,
            // row `dequeue`): a wave therefore reserves `chunk` pixels at a time and hands them to its lanes itself.
            // (Splitting the items over per-XCD heads, which the pooled kernel does, made THIS kernel 3-10 % slower.)
            if (chunk_next == chunk_end) {
                unsigned base = 0u;
                if (lane == 0) base = atomicAdd(work_counter, chunk);
                base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
                chunk_next = base < total ? base : total;
                chunk_end = (base + chunk < total) ? base + chunk : total;
                if (base >= total) { exhausted = true; chunk_end = chunk_next; }
            }
            const unsigned avail = chunk_end - chunk_next;
            const unsigned n = (unsigned)__popcll(mask);
            const unsigned rank = (unsigned)__popcll(mask & ((1ULL << lane) - 1ULL));
            const unsigned my = chunk_next + rank;
            chunk_next += (n < avail) ? n : avail;
            if (need && rank < avail) {
                const unsigned group = my >> 6, in = my & 63u;
                const unsigned tile = group / (unsigned)n_samples;
                const int sample = (int)(group % (unsigned)n_samples);
                const int u = (int)(tile % (unsigned)tiles_x) * 8 + (int)(in & 7u);
                const int v = launch_tile_row(fp, (int)(tile / (unsigned)tiles_x)) + (int)(in >> 3);
                if (u < fp.W && v < fp.row1 && launch_renders_row(fp, v) && !outside_render_area(fp, (float)u, (float)v)) {
                    VRT_REGION(0);
                    path_begin(fp, p, u, v, sample);
                    local_idx = (v - fp.row0) * fp.W + u;
                }
            }
        }
        if (__ballot(p.depth >= 0) == 0ULL) {
            if (exhausted) break;
            continue;
        }
        if (p.depth >= 0) {
            const bool done = path_segment<RESTIR>(fp, scl, P, out, local_idx, p, ts);
            if (done) {
                path_finish<RESTIR>(fp, scl, out, local_idx, p, ts);
                p.depth = -1;
            }
        }
    }
    if (INSTR) flush_stats(ts, sc.counters);
}

// ---- render, pooled schedule (vrt_pool.h) ------------------------------------------------------
// One wave = one pool of VRT_POOL_SLOTS path records in LDS.  Everything below the stage functions is wave-uniform
// bookkeeping: a census of slot states (ballots), a compacted list of the slots the chosen stage will work on, and
// the WALK loop's in-loop refill.  Waves never talk to each other; the only workgroup-level object is the staged
// pyramid / material table.  The wave leaves when the work counter is exhausted and its pool has drained.
#ifndef VRT_POOL_REFILL
#define VRT_POOL_REFILL 16   // WALK: idle lanes that trigger a refill from the pending list
#endif
#ifndef VRT_POOL_PARK
#define VRT_POOL_PARK 16     // WALK: with the list empty, suspend the walks still going once this few are left
#endif
#ifndef VRT_POOL_FINE_WORDS
#define VRT_POOL_FINE_WORDS 1024   // fine brick words of the scene kept in LDS (8 KB): all of a sparse scene's
#endif
// (state words per lane = (SLOTS + 63) / 64; slots past SLOTS are void: state 4)

__device__ __forceinline__ void wave_lds_sync() {  // LDS written by some lanes of this wave, read by others
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int lane_rank(unsigned long long m) {  // set bits of m below this lane
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// WAVES path pools of SLOTS slots per workgroup: 4 x 128 with two workgroups per CU (two waves per SIMD) by default; the whole l1
// level of a 256^3 grid leaves room for one workgroup of 8 x 128 per CU; a DENSE 128^3 grid runs one workgroup of 12 x 96 per CU
// -- three waves per SIMD at 168 registers (k_render_pool_dense12 below).
template <int G, bool RESTIR, bool INSTR, bool BLACK_SUN, bool CULL, bool D12 = false, bool SERVED = false, bool QUEUED = false>   // D12: twelve waves, and SHADE's shadow rays with the branchy descent; SERVED, QUEUED: below
// 208 registers per wave (the attribute counts half of the unified file): two waves per SIMD then leave the 96 that
// k_temporal runs in beside them (see there).  The allocator would take 238; the cap costs 28 bytes of scratch.
// The ReSTIR instantiation (no overlapped launches, so nothing runs beside it) takes the two-wave maximum of 256.
#ifndef VRT_POOL_HALF_VGPRS
#define VRT_POOL_HALF_VGPRS 104
#endif
__device__ __forceinline__ void render_pool_body(const FrameParams& fp, const SceneData& sc, const PixelBuffers& out, unsigned* work_counter, unsigned* next_counter, int n_samples, uint32_t* cold, uint32_t* drain_signal, uint32_t drain_value, PrimaryRecord* prim_cache, const PrimaryQueue& pq = PrimaryQueue{}) {
    constexpr int WAVES = pool_shape<G>(D12).waves, SLOTS = pool_shape<G>(D12).slots;
    constexpr int WORDS = (SLOTS + 63) / 64;
    constexpr bool BIG = (G == 256);   // which coarse levels are staged how: see LdsPyramid2
    __shared__ ulonglong2 s_l1p[BIG ? 1 : 512];
    __shared__ unsigned long long s_l1[BIG ? 4096 : 1];
    __shared__ unsigned long long s_l2[BIG ? 64 : 8];
    __shared__ unsigned long long s_fine[BIG ? 1 : VRT_POOL_FINE_WORDS];
    __shared__ float s_mats[128 * 14];
    __shared__ float s_cull[8];
    __shared__ uint32_t s_pool[WAVES][PF_COUNT * SLOTS];
    __shared__ uint32_t s_state[WAVES][WORDS * 64];
    __shared__ uint32_t s_list[WAVES][SLOTS];
    LdsPyramid2<G, CULL, D12, INSTR> P;
    P.l0 = sc.pyr.l0; P.l2 = s_l2;
    P.oob = sc.pyr.ref_oob != 0;
    if constexpr (BIG) {
        for (int i = threadIdx.x; i < 4096; i += blockDim.x) s_l1[i] = sc.pyr.l1[i];
        if (threadIdx.x < 64) s_l2[threadIdx.x] = sc.pyr.l2[threadIdx.x];
        P.l1 = s_l1;
        P.w3 = sc.pyr.l3[0];
    } else {
        // Packed here, every launch, from the levels as they stand: an edit or a rebuild of the scene needs no table of its own.
        for (int i = threadIdx.x; i < 512; i += blockDim.x) {   // i = the l1 cell (z4, y4, x4), three bits each
            ulonglong2 v;
            v.x = sc.pyr.l1[i];
            const unsigned long long w2 = sc.pyr.l2[(((i >> 8) & 1) << 2) | (((i >> 5) & 1) << 1) | ((i >> 2) & 1)];
            v.y = coarse_pack(w2, i & 7, (i >> 3) & 7, i >> 6, sc.pyr.l0c_base[i]);   // l0c_base <= 32768: below bit VRT_COARSE_BASE_BITS
            s_l1p[i] = v;
        }
        if (threadIdx.x < 8) s_l2[threadIdx.x] = sc.pyr.l2[threadIdx.x];
        const uint32_t n_all = *sc.pyr.l0c_count;  // non-empty fine words of the scene; the first VRT_POOL_FINE_WORDS live in LDS
        const uint32_t n_fine = n_all > VRT_POOL_FINE_WORDS ? VRT_POOL_FINE_WORDS : n_all;
        for (uint32_t i = threadIdx.x; i < n_fine; i += blockDim.x) s_fine[i] = sc.pyr.l0c[i];
        P.l1p = s_l1p; P.fine = s_fine; P.n_fine = n_fine; P.all_fine = n_all <= VRT_POOL_FINE_WORDS;
    }
    if constexpr (decltype(P)::mats_packed) {
        // One packed row per material id: the eight raw columns path_shade() reads and mat_derive() of the row, from the table
        // k_mat_derived refreshed at the last material upload, on the context's stream.  That refresh is ordered before this
        // launch on a render lane the way the upload of `mats` itself is: vrt_upload_materials waits for the context's stream
        // before it returns, and it (like vrt_create, whose refresh nothing waits for) leaves main_dirty set, so the next
        // launch's lanes wait for an event recorded behind it (order_overlapped_launch, vrt_pipeline.hip); a launch that is
        // not overlapped runs on the context's stream itself.  A SceneData without the table: derived here, by the same
        // function.
        for (int id = threadIdx.x; id < 128; id += blockDim.x) {
            const Material m = load_material(sc.mats, id);
            pack_material_row(s_mats + MP_COUNT * id, m, sc.mats_x ? load_mat_derived(sc.mats_x, id) : mat_derive(m));
        }
    } else {
        for (int i = threadIdx.x; i < 128 * 14; i += blockDim.x) s_mats[i] = sc.mats[i];
    }
    if (threadIdx.x < 8) s_cull[threadIdx.x] = sc.cull[threadIdx.x];
    if (blockIdx.x == 0 && threadIdx.x < VRT_WORK_HEADS) next_counter[threadIdx.x * VRT_WORK_HEAD_STRIDE] = 0u;  // the next launch's heads (idle during this launch)
    if (blockIdx.x == 0 && threadIdx.x == 0) next_counter[1] = 0u;  // and its "drain announced" word
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t* const pool = s_pool[wave];
    uint32_t* const state = s_state[wave];
    uint32_t* const list = s_list[wave];
    for (int k = 0; k < WORDS; k++) state[k * 64 + lane] = (k * 64 + lane < SLOTS) ? (uint32_t)SLOT_EMPTY : 4u;
    __syncthreads();
    SceneData scl = sc;
    scl.mats = s_mats;
    scl.cull = s_cull;
    constexpr int COLD = ColdLine<RESTIR>::count;
    uint32_t* const cold_wave = cold + (size_t)(blockIdx.x * WAVES + wave) * SLOTS * COLD;

    const int tiles_x = (fp.W + 7) >> 3;
    const int tiles_y = launch_tile_rows(fp);
    const unsigned total = (unsigned)(tiles_x * tiles_y) * 64u * (unsigned)n_samples;  // (tile, sample, pixel-in-tile) items
    TraceStats ts;
    stats_zero(ts);
    bool exhausted = false;  // wave-uniform
    // items are split into VRT_WORK_HEADS contiguous ranges of whole tiles; this wave starts on its XCD's range
    // a range is a whole number of tiles with all their samples; inside it items run sample-major (all tiles' sample 0,
    // then all tiles' sample 1, ...) so that the camera-ray records of sample 0 are there when the others begin
    const unsigned tiles_per_range = ((unsigned)(tiles_x * tiles_y) + VRT_WORK_HEADS - 1u) / VRT_WORK_HEADS;
    const unsigned range = tiles_per_range * 64u * (unsigned)n_samples;
    const uint32_t prim_tag = drain_value;  // launch_seq + 1: unique per launch, never 0
    unsigned head = blockIdx.x & (VRT_WORK_HEADS - 1u);  // workgroups go round-robin over the 8 XCDs
    int heads_left = VRT_WORK_HEADS;
    // QUEUED: the items of a head are what k_primary_vertex left in its part of the queue -- continuation records first, then leftovers
    unsigned q_cont = 0u, q_left = 0u;   // wave-uniform: of the current head
    if constexpr (QUEUED) {
        q_cont = pq.counts[head * VRT_PV_COUNT_STRIDE]; q_left = pq.counts[head * VRT_PV_COUNT_STRIDE + 1];
        q_cont = q_cont < pq.cap ? q_cont : pq.cap; q_left = q_left < pq.left_cap ? q_left : pq.left_cap;
    }

#if defined(VRT_DIAG_REGIONS)
    unsigned long long t_prev = __builtin_readcyclecounter();
    int prev_stage = 4;  // 4 = start-up
    // summed in registers and flushed once at the end: an atomic per stage switch from 2048 waves saturates the
    // words it lands on and slows every other memory operation (it made the first version of this clock useless)
    unsigned long long t_stage[6] = {0ULL, 0ULL, 0ULL, 0ULL, 0ULL, 0ULL};
    unsigned long long t_sub[4] = {0ULL, 0ULL, 0ULL, 0ULL};   // BEGIN: reservation, record read, set-up from a record, set-up with a ray
#define VRT_SUB_CLOCK(q) do { __asm__ volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); const unsigned long long t_ = __builtin_readcyclecounter(); t_sub[q] += t_ - t_sub_prev; t_sub_prev = t_; } while (0)
#define VRT_SUB_START() do { __asm__ volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); t_sub_prev = __builtin_readcyclecounter(); } while (0)
    unsigned long long t_sub_prev = 0ULL;
#define VRT_POOL_CLOCK(next_stage)                                                                              \
    do {                                                                                                        \
        const unsigned long long t_now = __builtin_readcyclecounter();                                          \
        _Pragma("unroll") for (int q_ = 0; q_ < 6; q_++) if (prev_stage == q_) t_stage[q_] += t_now - t_prev;   \
        t_prev = t_now; prev_stage = (next_stage);                                                              \
    } while (0)
#else
#define VRT_POOL_CLOCK(next_stage) ((void)0)
#define VRT_SUB_CLOCK(q) ((void)0)
#define VRT_SUB_START() ((void)0)
#endif
    for (;;) {
        wave_lds_sync();
        VRT_POOL_CLOCK(5);  // 5 = census + list
        // census
        uint32_t st[WORDS];
        int cnt[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < WORDS; k++) {
            st[k] = state[k * 64 + lane];
#pragma unroll
            for (int q = 0; q < 4; q++) cnt[q] += __popcll(__ballot(st[k] == (uint32_t)q));
        }
        if (exhausted) cnt[SLOT_EMPTY] = 0;
        // the stage with the most slots waiting; ties: SHADE, ESCAPE, WALK, BEGIN.  (Rules that hold WALK back until
        // more rays are pending -- a minimum count, or a lead over the other stages -- measured 0 to -4 %.)
        int stage = SLOT_SHADE, best = cnt[SLOT_SHADE];
        if (cnt[SLOT_ESCAPE] > best) { stage = SLOT_ESCAPE; best = cnt[SLOT_ESCAPE]; }
        if (cnt[SLOT_RAY] > best) { stage = SLOT_RAY; best = cnt[SLOT_RAY]; }
        if (cnt[SLOT_EMPTY] > best) { stage = SLOT_EMPTY; best = cnt[SLOT_EMPTY]; }
        if (best == 0) break;  // nothing pending and no work left
        // compacted list of that stage's slots
        int n = 0;
#pragma unroll
        for (int k = 0; k < WORDS; k++) {
            const bool mine = st[k] == (uint32_t)stage;
            const unsigned long long m = __ballot(mine);
            if (mine) list[n + lane_rank(m)] = (uint32_t)(k * 64 + lane);
            n += __popcll(m);
        }
        wave_lds_sync();
        VRT_POOL_CLOCK(stage);

        if (stage == SLOT_RAY) {
            VRT_REGION(14);
#ifndef VRT_POOL_PARK_MIN
#define VRT_POOL_PARK_MIN 64
#endif
            const int park = (n >= VRT_POOL_PARK_MIN) ? VRT_POOL_PARK : 0;  // suspending only pays when other stages then have work
            int head = 0;
            bool active = false, ended = false;
            RayWalk w;
            BrickCache bc;
            bc.key = -1; bc.word = 0ULL;
            CoarseWords cw;
            cw.w1 = 0ULL; cw.w2 = 0ULL;
            SlotRef s;
            s.base = pool; s.stride = SLOTS;
            int slot = 0, iters0 = 0;
            for (;;) {
                // event: finished walks go to their slots, idle lanes take the next pending rays -- or, with the
                // list empty and few walks left, the rest is suspended
                const unsigned long long idle = __ballot(!active);
                const int n_idle = __popcll(idle);
                if (ended) {
                    VRT_REGION(16);
                    walk_store(s, w);
                    state[slot] = (uint32_t)slot_state_after_walk<G>(w.t, s.f(PF_FLOOR_T));
                    if (prim_cache) {  // the camera ray of a pixel's sample 0: leave its record for the other samples
                        const uint32_t ids = s.u(PF_IDS);
                        if ((ids >> 24) == 0u)  // depth 0, sample 0 (the check word tells a reader whether it saw all of the record)
                            primary_record_store(&prim_cache[((int)((ids >> 12) & 0xfffu) - fp.row0) * fp.W + (int)(ids & 0xfffu)], primary_record(s, prim_tag));
                    }
                    ts.iters += (unsigned)(w.iters - iters0);
                    ended = false;
                }
                if (head >= n) {
                    if (64 - n_idle <= park) {
                        if (active) {  // suspend: the slot stays SLOT_RAY
                            VRT_REGION(17);
                            walk_store(s, w);
                            ts.iters += (unsigned)(w.iters - iters0);
                        }
                        break;
                    }
                } else {
                    const int idx = head + lane_rank(idle);
                    if (!active && idx < n) {
                        VRT_REGION(15);
                        slot = (int)list[idx];
                        s.base = pool + slot;
                        walk_load<G>(s, w);
                        coarse_fetch(P, w.ix, w.iy, w.iz, cw);
                        bc.key = -1;
                        iters0 = w.iters;
                        active = true;
                    }
                    head += (n_idle < n - head) ? n_idle : n - head;
                }
                // the DDA loop proper: nothing but steps until enough lanes have gone idle for the next event
                const int target = (head < n) ? VRT_POOL_REFILL : 64 - park;
                do {
                    if (active) {
                        int nq;
                        if (walk_trip(P, w, bc, cw, nq)) { active = false; ended = true; }
                        ts.queries += (unsigned)nq;
                    }
                } while (__popcll(__ballot(!active)) < target);
            }
        } else {
            const int take = n < 64 ? n : 64;
            unsigned base = 0u, limit = 0u;  // items [base, limit) go to lanes 0.. of this BEGIN
            unsigned range0 = 0u, per_sample = 1u;  // first item of the range they belong to, items per sample in it
            unsigned q_head = 0u, q_n_cont = 0u;    // QUEUED: the head [base, limit) belongs to, and its continuation records
            if constexpr (QUEUED) {
              if (stage == SLOT_EMPTY) {
                VRT_SUB_START();
                unsigned got = 0u;
                if (lane == 0) got = atomicAdd(work_counter + head * VRT_WORK_HEAD_STRIDE, (unsigned)take);
                got = (unsigned)__builtin_amdgcn_readfirstlane((int)got);
                const unsigned cnt = q_cont + q_left;
                q_head = head; q_n_cont = q_cont;
                base = got;
                limit = (got + (unsigned)take < cnt) ? got + (unsigned)take : cnt;
                if (got + (unsigned)take >= cnt) {
                    heads_left -= 1;
                    head = (head + 1u) & (VRT_WORK_HEADS - 1u);
                    q_cont = pq.counts[head * VRT_PV_COUNT_STRIDE]; q_left = pq.counts[head * VRT_PV_COUNT_STRIDE + 1];
                    q_cont = q_cont < pq.cap ? q_cont : pq.cap; q_left = q_left < pq.left_cap ? q_left : pq.left_cap;
                    if (heads_left == 0) {
                        exhausted = true;
                        if (drain_signal && lane == 0 && atomicExch(work_counter + 1, 1u) == 0u)
                            __hip_atomic_fetch_max(drain_signal, drain_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    }
                }
                if (base > limit) base = limit;
                VRT_SUB_CLOCK(0);   // (the sub-clocks of the plain BEGIN below, at the same points: reservation, read, set-up)
              }
            } else
            if (stage == SLOT_EMPTY) {
                VRT_SUB_START();
                // pull from the current head; a used-up range sends the wave on to the next head (and this BEGIN
                // hands out nothing: the census runs again)
                unsigned got = 0u;
                if (lane == 0) got = atomicAdd(work_counter + head * VRT_WORK_HEAD_STRIDE, (unsigned)take);
                got = (unsigned)__builtin_amdgcn_readfirstlane((int)got);
                const unsigned r0 = head * range, r1 = (r0 + range < total) ? r0 + range : total;
                base = r0 + got;
                limit = (base + (unsigned)take < r1) ? base + (unsigned)take : r1;
                range0 = r0;
                per_sample = (r1 > r0) ? (r1 - r0) / (unsigned)n_samples : 1u;
                if (r0 >= total || base + (unsigned)take >= r1) {
                    heads_left -= 1;
                    head = (head + 1u) & (VRT_WORK_HEADS - 1u);
                    if (heads_left == 0) {
                        exhausted = true;
                        // the launch starts to drain: tell the stream holding the NEXT launch back until now (vrt_api.hip)
                        // (the first wave to get here does; word 1 of this launch's head line says whether one has)
                        if (drain_signal && lane == 0 && atomicExch(work_counter + 1, 1u) == 0u)
                            __hip_atomic_fetch_max(drain_signal, drain_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    }
                }
                if (base > limit) base = limit;
                VRT_SUB_CLOCK(0);
            }
            if (lane < take) {
                SlotRef s;
                s.stride = SLOTS;
                if (stage == SLOT_SHADE) {
                    VRT_REGION(11);
                    const int slot = (int)list[lane];
                    s.base = pool + slot;
                    state[slot] = (uint32_t)pool_shade<HIT_SOMETHING, BLACK_SUN, RESTIR>(fp, scl, P, out, s, cold_wave + slot * COLD, ts);
                } else if (stage == SLOT_ESCAPE) {
                    VRT_REGION(12);
                    const int slot = (int)list[lane];
                    s.base = pool + slot;
                    state[slot] = (uint32_t)pool_shade<HIT_NOTHING, false, RESTIR>(fp, scl, P, out, s, cold_wave + slot * COLD, ts);
                } else {
                    VRT_REGION(13);
                    const unsigned my = base + (unsigned)lane;
                    if constexpr (QUEUED) {
                        if (my < limit) {
                            const int slot = (int)list[lane];
                            s.base = pool + slot;
                            if (my < q_n_cont) {
                                constexpr int PW = PrimaryContWords<BLACK_SUN>::count;
                                const uint32_t* const at = pq.entries + ((size_t)q_head * pq.cap + my) * PW;
                                uint32_t e[PW];
#pragma unroll
                                for (int k = 0; k < PW; k++) e[k] = at[k];
                                VRT_SUB_CLOCK(1);
                                state[slot] = (uint32_t)pool_begin_queued<G, CULL, BLACK_SUN>(fp, scl.cull, s, cold_wave + slot * COLD, e, ts);
                                VRT_SUB_CLOCK(3);   // a set-up with a ray: the bounce ray's
                            } else {
                                // a depth-0 item k_primary_vertex left to the pool: as a launch without the queue begins it
                                const uint32_t item = pq.leftovers[(size_t)q_head * pq.left_cap + (my - q_n_cont)];
                                const int u = (int)(item & 0xfffu), v = (int)((item >> 12) & 0xfffu), sample = (int)(item >> 28);
                                const PrimaryRecord rec = primary_record_load(&prim_cache[(v - fp.row0) * fp.W + u]);
                                const bool known = primary_record_valid(rec, prim_tag);
                                VRT_SUB_CLOCK(1);
                                int st;
                                if (known) st = pool_begin_known<G>(fp, s, u, v, sample, rec);
                                else {
                                    st = pool_begin<G, CULL>(fp, scl.cull, s, u, v, sample, ts);
                                    if (sample == 0 && st != SLOT_RAY) primary_record_store(&prim_cache[(v - fp.row0) * fp.W + u], primary_record(s, prim_tag));
                                }
                                state[slot] = (uint32_t)st;
                                VRT_SUB_CLOCK(known ? 2 : 3);
                            }
                        }
                    } else
                    if (my < limit) {
                        const int slot = (int)list[lane];
                        s.base = pool + slot;
                        const unsigned j = my - range0;  // sample-major inside the range (n_samples <= 4)
                        const int sample = (int)(j >= per_sample) + (int)(j >= 2u * per_sample) + (int)(j >= 3u * per_sample);
                        const unsigned rem = j - (unsigned)sample * per_sample;
                        const unsigned tile = range0 / (64u * (unsigned)n_samples) + (rem >> 6), in = rem & 63u;
                        const int u = (int)(tile % (unsigned)tiles_x) * 8 + (int)(in & 7u);
                        const int v = launch_tile_row(fp, (int)(tile / (unsigned)tiles_x)) + (int)(in >> 3);
                        if (u < fp.W && v < fp.row1 && launch_renders_row(fp, v) && !outside_render_area(fp, (float)u, (float)v)) {
                            bool known = false;
                            PrimaryRecord rec;
                            rec.x = rec.y = rec.z = rec.dx = rec.dy = rec.dz = rec.ft = rec.w = 0u;
                            // (SERVED: k_primary_records has run for this launch, so sample 0 may find its record too; one that is
                            // missing or does not check out is set up and walked below, and leaves its record, as ever)
                            if (prim_cache && (SERVED || sample > 0)) {
                                rec = primary_record_load(&prim_cache[(v - fp.row0) * fp.W + u]);
                                known = primary_record_valid(rec, prim_tag);
                            }
                            VRT_SUB_CLOCK(1);
                            int st;
                            if (known) st = pool_begin_known<G>(fp, s, u, v, sample, rec);
                            else {
                                st = pool_begin<G, CULL>(fp, scl.cull, s, u, v, sample, ts);
                                // a camera ray with nothing to walk (it misses the grid or every solid voxel) is finished here: its
                                // record is left here too
                                if (prim_cache && sample == 0 && st != SLOT_RAY) primary_record_store(&prim_cache[(v - fp.row0) * fp.W + u], primary_record(s, prim_tag));
                            }
                            state[slot] = (uint32_t)st;
                            VRT_SUB_CLOCK(known ? 2 : 3);
                        }
                    }
                }
            }
        }
    }
    VRT_POOL_CLOCK(4);
#if defined(VRT_DIAG_REGIONS)
    if (lane == 0)
        for (int q = 0; q < 6; q++) atomicAdd(&g_vrt_region[2 * (20 + q)], t_stage[q]);
    if (lane == 0)
        for (int q = 0; q < 4; q++) atomicAdd(&g_vrt_region[52 + q], t_sub[q]);
#endif
    if (INSTR) flush_stats(ts, sc.counters);
}
// (the register attribute takes a literal, hence one kernel per budget around the shared body)
// SERVED: the instantiation for launches with a pre-pass (k_primary_records, below).  A template parameter, not a kernel argument: as
// an argument the test reached the code of every launch, and the one-sample calls, which have no pre-pass, ran 1.0 % slower
// (DESIGN.md section 7); this way a launch without a pre-pass runs the machine code it ran before there was one.
template <int G, bool INSTR, bool BLACK_SUN, bool CULL, bool SERVED = false>
__global__ __launch_bounds__(64 * pool_shape<G>(false).waves, VRT_POOL_MIN_WAVES) __attribute__((amdgpu_num_vgpr(VRT_POOL_HALF_VGPRS))) void k_render_pool(FrameParams fp, SceneData sc, PixelBuffers out, unsigned* work_counter, unsigned* next_counter, int n_samples, uint32_t* cold, uint32_t* drain_signal, uint32_t drain_value, PrimaryRecord* prim_cache) {
    render_pool_body<G, false, INSTR, BLACK_SUN, CULL, false, SERVED>(fp, sc, out, work_counter, next_counter, n_samples, cold, drain_signal, drain_value, prim_cache);
}
// A DENSE grid under an emitting sun: the shadow rays of SHADE with the branchy descent (shadow_branchy_of, vrt_trace.h), and
// THREE waves per SIMD: one workgroup of twelve waves per CU, 96 slots per pool (12 x 10.4 KB of pools
// + 25 KB of pyramid and materials = 148 KB of LDS), 168 registers (21-36 spilled).  A dense grid's rays end after a step or two, so
// its waves spend their time in SHADE waiting on texel and shadow-ray loads, which a third wave covers: the dense 4K frame
// 2 673 -> 2 953 Mpath-samples/s.  A sparse scene loses as much with it (config 2 -3.6 %, sun-lit -6 %: fewer slots per pool
// thin the WALK stage out, and the spills cost), so only launches over a dense grid under an emitting sun use it.
// At 256^3 the staged l1 level (32 KB) leaves the twelve pools 88 slots each (153 KB of LDS in all).
template <int G, bool INSTR, bool CULL>
__global__ __launch_bounds__(64 * pool_shape<G>(true).waves, 3) __attribute__((amdgpu_num_vgpr(84))) void k_render_pool_dense12(FrameParams fp, SceneData sc, PixelBuffers out, unsigned* work_counter, unsigned* next_counter, int n_samples, uint32_t* cold, uint32_t* drain_signal, uint32_t drain_value, PrimaryRecord* prim_cache) {
    render_pool_body<G, false, INSTR, false, CULL, true>(fp, sc, out, work_counter, next_counter, n_samples, cold, drain_signal, drain_value, prim_cache);
}
template <int G, bool INSTR, bool CULL>
__global__ __launch_bounds__(64 * pool_shape<G>(false).waves, VRT_POOL_MIN_WAVES) __attribute__((amdgpu_num_vgpr(128))) void k_render_pool_restir(FrameParams fp, SceneData sc, PixelBuffers out, unsigned* work_counter, unsigned* next_counter, int n_samples, uint32_t* cold, uint32_t* drain_signal, uint32_t drain_value, PrimaryRecord* prim_cache) {
    render_pool_body<G, true, INSTR, false, CULL>(fp, sc, out, work_counter, next_counter, n_samples, cold, drain_signal, drain_value, prim_cache);
}

// The camera-ray records of a launch, made AHEAD of it (primary_record_walk, vrt_pool.h) by a kernel small enough to run beside two
// pooled workgroups per CU: one wave a workgroup, one workgroup an 8x8 tile of the rows the launch renders (BEGIN's own gating), no
// LDS -- the pyramid is read through global memory, 260 KiB that stay in cache -- and at most the 96 registers that two pooled waves
// of 208 leave free on a SIMD (the attribute counts half of the unified file, as VRT_TEMPORAL_HALF_VGPRS does).  Queued on the
// launch's own lane behind that lane's previous launch, it runs while the launches of the other lanes hold the heavy slots, in issue
// slots their waves leave idle; the launch then begins sample 0 from the record (the SERVED instantiation) instead of setting the ray up and
// walking it between bounce rays.  Nothing waits for it but stream order, and a record that is not there is walked as ever.
#ifndef VRT_PRIMARY_HALF_VGPRS
#define VRT_PRIMARY_HALF_VGPRS 48
#endif
template <int G, bool CULL>
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(VRT_PRIMARY_HALF_VGPRS))) void k_primary_records(FrameParams fp, SceneData sc, PrimaryRecord* prim_cache, uint32_t tag) {
    const int tiles_x = (fp.W + 7) >> 3;
    const unsigned tile = blockIdx.x, in = threadIdx.x;
    const int u = (int)(tile % (unsigned)tiles_x) * 8 + (int)(in & 7u);
    const int v = launch_tile_row(fp, (int)(tile / (unsigned)tiles_x)) + (int)(in >> 3);
    if (!(u < fp.W && v < fp.row1 && launch_renders_row(fp, v) && !outside_render_area(fp, (float)u, (float)v))) return;
    GlobalPyramid<G> P;
    P.p = sc.pyr;
    primary_record_store(&prim_cache[(v - fp.row0) * fp.W + u], primary_record_walk<G, CULL>(fp, P, sc.cull, u, v, tag));
}

// The primary vertex of every path of a launch, AHEAD of it (vrt_primary.h): one wave a workgroup, one workgroup an 8x8 tile, a lane
// a pixel, gated as k_primary_records is, whose records it reads; no LDS, the pyramid (walked by the emitting sun's shadow rays only)
// and the material table through global memory.  NOT the pre-pass's register budget: at 96 registers it spills 52-97 of them and
// measures slower than at 160, where it no longer fits beside two pooled waves of a SIMD, only beside one (below).  The g-buffer and
// the shading point of the primary vertex (primary_vertex_surf: material row, mat_derive, basis) are made once a pixel, ahead of the
// sample loop; paths that go on are compacted per sample with a ballot and one atomic a wave onto the queue of head (tile % 8).
// Two budgets, so two kernels around one body (the register attribute takes a literal).  What decides is how many of its waves fit
// beside ONE pooled wave of a SIMD (208 registers: 304 are left), the slots a draining launch frees: two of up to 152 registers, one of
// 160 or 168.  Under a black sun the kernel took 139 registers before the shading point was shared -- allocated as 144, two such waves --
// and asks for 165 with it live across the sample loop; capped at 144 it spills ONE register and keeps the second wave.  Measured in one
// session, headline: 144: +2.7 % over the parent, 152: +2.5 %, 160: +2.1 %, 168: -0.6 %.  Under an emitting sun it took
// 157 already (one wave beside a pooled one); at 168 no instantiation spills, at 160 eleven registers do, at 144 fourteen, and the
// sun-lit scene orders them 168 > 160 > 152 = 144, all above the parent.
#ifndef VRT_PRIMARY_VERTEX_HALF_VGPRS
#define VRT_PRIMARY_VERTEX_HALF_VGPRS 72       // black sun: 144 registers
#endif
#ifndef VRT_PRIMARY_VERTEX_SUN_HALF_VGPRS
#define VRT_PRIMARY_VERTEX_SUN_HALF_VGPRS 84   // emitting sun: 168 registers (allocated like 160: three waves a SIMD where no pooled wave is)
#endif
#if 2 * VRT_PRIMARY_VERTEX_HALF_VGPRS + 2 * VRT_POOL_HALF_VGPRS > 512 || 2 * VRT_PRIMARY_VERTEX_SUN_HALF_VGPRS + 2 * VRT_POOL_HALF_VGPRS > 512
#error "k_primary_vertex must fit beside one pooled wave of a SIMD at least"   // (or it only runs where the chip is empty)
#endif
#ifndef VRT_PRIMARY_SHARED_SURF
#define VRT_PRIMARY_SHARED_SURF 1   // 0 (A/B and region-clock variants only): the shading point per sample inside path_shade, as before it was shared
#endif
template <int G, bool BLACK_SUN, bool CULL>
static __device__ __forceinline__ void primary_vertex_body(const FrameParams& fp, const SceneData& sc, const PixelBuffers& out, const PrimaryRecord* prim_cache, uint32_t tag, int n_samples, const PrimaryQueue& pq) {
    const int tiles_x = (fp.W + 7) >> 3;
    const unsigned tile = blockIdx.x, in = threadIdx.x;
    const int u = (int)(tile % (unsigned)tiles_x) * 8 + (int)(in & 7u);
    const int v = launch_tile_row(fp, (int)(tile / (unsigned)tiles_x)) + (int)(in >> 3);
    const bool live = u < fp.W && v < fp.row1 && launch_renders_row(fp, v) && !outside_render_area(fp, (float)u, (float)v);
    const unsigned head = tile & (VRT_PV_HEADS - 1u);
    constexpr int PW = PrimaryContWords<BLACK_SUN>::count;
    GlobalPyramid<G> P;
    P.p = sc.pyr;
    TraceStats ts;
    stats_zero(ts);
    PrimaryRecord rec;
    rec.x = rec.y = rec.z = rec.dx = rec.dy = rec.dz = rec.ft = rec.w = 0u;
    bool known = false;
    Hit h;
    hit_init(h);
    int state = SLOT_ESCAPE;
    constexpr bool SHARED_SURF = VRT_PRIMARY_SHARED_SURF != 0;
    Surf surf;   // the pixel's shading point, built once ahead of the sample loop (primary_vertex_surf)
#if defined(VRT_DIAG_REGIONS)
    __shared__ unsigned long long pv_clock[PVR_COUNT + 1];   // the wave's region clocks (VRT_PV_CLOCK, vrt_trace.h)
    if (in <= (unsigned)PVR_COUNT) pv_clock[in] = 0ULL;
    ts.pv = pv_clock;
    ts.pv[PVR_COUNT] = __builtin_readcyclecounter();
#endif
    if (live) {
        rec = primary_record_load(&prim_cache[(v - fp.row0) * fp.W + u]);
        known = primary_record_valid(rec, tag);
    }
    VRT_PV_CLOCK(ts, PVR_RECORD);
    if (known) {
        state = primary_vertex_hit<G>(fp, sc, rec, h, ts);
        primary_vertex_gbuffer(fp, out, u, v, rec, h);
        VRT_PV_CLOCK(ts, PVR_HIT);
        if constexpr (SHARED_SURF) (void)primary_vertex_surf<GlobalPyramid<G>>(sc, rec, h, state, surf);
        VRT_PV_CLOCK(ts, PVR_SURF);
    }
    unsigned n_done = 0u, n_on = 0u;
    for (int sample = 0; sample < n_samples; sample++) {
        Path<false> p;
        bool on = false;
        if (known) on = primary_vertex_sample<G, BLACK_SUN, CULL, SHARED_SURF>(fp, sc, P, out, u, v, sample, rec, h, state, p, ts, &surf);
        // continuations: one atomic a wave on the head's record count; a record that does not fit is a leftover
        const unsigned long long m_on = __ballot(on);
        bool left = live && !known;
        if (m_on != 0ULL) {
            unsigned at = 0u;
            if (in == (unsigned)__builtin_ctzll(m_on)) at = atomicAdd(&pq.counts[head * VRT_PV_COUNT_STRIDE], (unsigned)__popcll(m_on));
            at = (unsigned)__shfl((int)at, __builtin_ctzll(m_on), 64) + (unsigned)__popcll(m_on & ((1ULL << in) - 1ULL));
            if (on) {
                if (at < pq.cap) primary_cont_pack<BLACK_SUN>(pq.entries + ((size_t)head * pq.cap + at) * PW, p);
                else left = true;
            }
        }
        const unsigned long long m_left = __ballot(left);
        if (m_left != 0ULL) {
            unsigned at = 0u;
            if (in == (unsigned)__builtin_ctzll(m_left)) at = atomicAdd(&pq.counts[head * VRT_PV_COUNT_STRIDE + 1], (unsigned)__popcll(m_left));
            at = (unsigned)__shfl((int)at, __builtin_ctzll(m_left), 64) + (unsigned)__popcll(m_left & ((1ULL << in) - 1ULL));
            if (left && at < pq.left_cap) pq.leftovers[(size_t)head * pq.left_cap + at] = primary_leftover_item(u, v, sample);
        }
        if (known && !left) { if (on) n_on++; else n_done++; }
        VRT_PV_CLOCK(ts, PVR_APPEND);
    }
#if defined(VRT_DIAG_REGIONS)
    if (in < (unsigned)PVR_COUNT) atomicAdd(&g_vrt_region[56 + in], pv_clock[in]);   // [56..63]: tools/diag_regions.py
    static_assert(56 + PVR_COUNT <= 64, "the region counters' last eight words");
#endif
    if (pq.report) {   // development builds: the counts the tests read
        unsigned long long a = n_done, b = n_on;
        for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); }
        if (in == 0u) { atomicAdd(&pq.report[0], a); atomicAdd(&pq.report[1], b); }
    }
}
template <int G, bool CULL>   // black sun
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(VRT_PRIMARY_VERTEX_HALF_VGPRS))) void k_primary_vertex(FrameParams fp, SceneData sc, PixelBuffers out, const PrimaryRecord* prim_cache, uint32_t tag, int n_samples, PrimaryQueue pq) {
    primary_vertex_body<G, true, CULL>(fp, sc, out, prim_cache, tag, n_samples, pq);
}
template <int G, bool CULL>   // emitting sun
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(VRT_PRIMARY_VERTEX_SUN_HALF_VGPRS))) void k_primary_vertex_sun(FrameParams fp, SceneData sc, PixelBuffers out, const PrimaryRecord* prim_cache, uint32_t tag, int n_samples, PrimaryQueue pq) {
    primary_vertex_body<G, false, CULL>(fp, sc, out, prim_cache, tag, n_samples, pq);
}
// QUEUED: the instantiation for launches behind k_primary_vertex (plan_primary, vrt_plan.h): BEGIN resumes the queue's paths at depth 1
// and takes its leftovers as depth-0 items.  A kernel of its own, so that every other launch runs the machine code it ran before.
template <int G, bool BLACK_SUN, bool CULL>
__global__ __launch_bounds__(64 * pool_shape<G>(false).waves, VRT_POOL_MIN_WAVES) __attribute__((amdgpu_num_vgpr(VRT_POOL_HALF_VGPRS))) void k_render_pool_queued(FrameParams fp, SceneData sc, PixelBuffers out, unsigned* work_counter, unsigned* next_counter, int n_samples, uint32_t* cold, uint32_t* drain_signal, uint32_t drain_value, PrimaryRecord* prim_cache, PrimaryQueue pq) {
    render_pool_body<G, false, false, BLACK_SUN, CULL, false, true, true>(fp, sc, out, work_counter, next_counter, n_samples, cold, drain_signal, drain_value, prim_cache, pq);
}

// ---- spatial reuse ---------------------------------------------------------------------------
#ifndef VRT_GRIS_SPLIT
#define VRT_GRIS_SPLIT 1   // the pass as two kernels of three waves per SIMD each (gris_pixel, vrt_restir.h); 0: one kernel of two
                           // (config 3: 358 against 317 Mpath-samples/s; the first half alone at three waves: 335)
#endif
#ifndef VRT_GRIS_MIN_WAVES
#define VRT_GRIS_MIN_WAVES 2   // whole pass: 256 registers, no spills; one wave per SIMD left the VALU idle a third of the time (6.6 vs 10.2 ms)
#endif
#ifndef VRT_GRIS_MIN_WAVES_A
#define VRT_GRIS_MIN_WAVES_A 3 // first half: 168 registers, no spills
#endif
#ifndef VRT_GRIS_MIN_WAVES_B
#define VRT_GRIS_MIN_WAVES_B 3 // second half: 168 registers hold it once the output reservoir carries the chosen TAP instead of its sample
#endif
template <int G, bool INSTR, int PHASE = 0>
__global__ __launch_bounds__(256, (PHASE == 1 ? VRT_GRIS_MIN_WAVES_A : PHASE == 2 ? VRT_GRIS_MIN_WAVES_B : VRT_GRIS_MIN_WAVES)) void k_gris(FrameParams fp, SceneData sc, GrisBuffers gb, int r0, int r_first, int r1, int tiles_x, int band_w) {
    constexpr int N1 = GridDim<G>::n1 * GridDim<G>::n1 * GridDim<G>::n1, N2 = GridDim<G>::n2 * GridDim<G>::n2 * GridDim<G>::n2;
    __shared__ unsigned long long s_l1[N1];
    __shared__ unsigned long long s_l2[N2];
    __shared__ float s_mats[128 * 14];
    __shared__ float s_mats_x[128 * 8];
    __shared__ float s_cs[4][64];          // per wave (= 8x8 pixel tile): cos / sin of the 32 tap angles
    __shared__ uint16_t s_off[32][256];    // per tap, per thread: the tap's pixel offset
    for (int i = threadIdx.x; i < N1; i += blockDim.x) s_l1[i] = sc.pyr.l1[i];
    if (threadIdx.x < N2) s_l2[threadIdx.x] = sc.pyr.l2[threadIdx.x];
    for (int i = threadIdx.x; i < 128 * 14; i += blockDim.x) s_mats[i] = sc.mats[i];
    for (int i = threadIdx.x; i < 128 * 8; i += blockDim.x) s_mats_x[i] = gb.mats_x[i];
    __shared__ float s_cull[8];
    if (threadIdx.x < 8) s_cull[threadIdx.x] = sc.cull[threadIdx.x];
    LdsPyramid<G, INSTR> P;
    P.l0 = sc.pyr.l0; P.l1 = s_l1; P.l2 = s_l2;
    P.w3 = (G == 256) ? sc.pyr.l3[0] : 0ULL;
    P.oob = sc.pyr.ref_oob != 0;
    SceneData scl = sc;
    scl.mats = s_mats;
    scl.cull = s_cull;
    GrisBuffers gbl = gb;
    gbl.mats_x = s_mats_x;
    // 16x16 pixel tile per workgroup = four 8x8 wave tiles.  Workgroups go to the 8 XCDs round robin: XCD k takes the
    // k-th vertical band of tiles, row by row, so that the tiles resident on one XCD at a time are neighbours and their
    // 64x64-pixel tap windows overlap in that XCD's L2.
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int bx = xcd * band_w + slot % band_w, by = slot / band_w;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int u = bx * 16 + (wave & 1) * 8 + (lane & 7);
    // r0 is a multiple of 8: a wave's 8x8 pixels are then one tile of the tap-angle hash (u >> 3, v >> 3), whatever row the
    // shard starts at; rows [r0, r_first) are not this launch's
    const int v = r0 + by * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (lane < 32) gris_tap_cs(u, v, 0, lane, s_cs[wave]);
    __syncthreads();
    GrisTaps taps;
    taps.cs = s_cs[wave]; taps.off = &s_off[0][threadIdx.x]; taps.off_stride = 256;
    TraceStats ts;
    stats_zero(ts);
    if (bx < tiles_x && u < fp.W && v >= r_first && v < r1) gris_pixel<PHASE>(fp, scl, P, gbl, taps, u, v, 0, 24.0f, 32, 1, ts);
    if (INSTR) flush_stats(ts, sc.counters);
}

// The first kernel of the split pass (pathtracer.py:917-931: the centre's sample shifted into every accepted neighbour's domain; the
// sum of the terms is the canonical MIS weight), on a WAVE-LEVEL schedule.  Whether a pixel's shifts need evaluating is a
// property of ITS sample (gris_classify_pixel: a dead sample makes every one of them a constant), so the counts are bimodal
// -- 0 or ~25 taps per pixel, 7.8 on average in a scene open to the sky -- and a loop per lane runs as long as the wave's busiest
// pixel (measured: 16.6 trips at 30 of 64 lanes).  Here the wave's 8x8 pixels pool their taps: every lane lists its live taps in
// LDS, the wave evaluates the list 64 at a time (a lane loads the sample of whichever pixel its item belongs to: 224 bytes from
// L2 instead of registers kept across a loop) and leaves each term where the item was; then every lane sums ITS pixel's terms in
// tap order, constants included -- the float sum of gris_pixel<1>, term for term (gris_first_term is the loop's body).
#ifndef VRT_GRIS_FIRST_ROUNDS
#define VRT_GRIS_FIRST_ROUNDS 1
#endif
template <int G, bool INSTR>
__global__ __launch_bounds__(256, VRT_GRIS_MIN_WAVES_A) void k_gris_first(FrameParams fp, SceneData sc, GrisBuffers gb, int r0, int r_first, int r1, int tiles_x, int band_w) {
    __shared__ float s_mats[128 * 14];
    __shared__ float s_mats_x[128 * 8];
    __shared__ float s_cs[4][64];          // per wave (= 8x8 pixel tile): cos / sin of the 32 tap angles
    __shared__ uint32_t s_item[4][64 * 32 / VRT_GRIS_FIRST_ROUNDS];  // per wave: (lane << 8 | tap) of every tap to evaluate, then the tap's term in its place
    __shared__ float s_radius[4][64];      // per wave: each pixel's radius_shift
    for (int i = threadIdx.x; i < 128 * 14; i += blockDim.x) s_mats[i] = sc.mats[i];
    for (int i = threadIdx.x; i < 128 * 8; i += blockDim.x) s_mats_x[i] = gb.mats_x[i];
    SceneData scl = sc;
    scl.mats = s_mats;
    GrisBuffers gbl = gb;
    gbl.mats_x = s_mats_x;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int bx = xcd * band_w + slot % band_w, by = slot / band_w;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int u0 = bx * 16 + (wave & 1) * 8, v0 = r0 + by * 16 + (wave >> 1) * 8;   // the wave's 8x8 tile (one tile of the tap-angle hash)
    const int u = u0 + (lane & 7), v = v0 + (lane >> 3);
    if (lane < 32) gris_tap_cs(u, v, 0, lane, s_cs[wave]);
    __syncthreads();
    GrisTaps taps;
    taps.cs = s_cs[wave]; taps.off = nullptr; taps.off_stride = 0;
    TraceStats ts;
    stats_zero(ts);
    const int max_taps = 32;
    const float max_radius = 24.0f;
    uint32_t* const item = s_item[wave];

    // this lane's own pixel: gris_pixel<1>'s early outs, its masks and the constant term
    const int idx = (v - fp.row0) * fp.W + u;
    bool mine = bx < tiles_x && u < fp.W && v >= r_first && v < r1 && !outside_render_area(fp, (float)u, (float)v);
    unsigned accepted = 0u, walk = 0u;
    float const_term = 0.0f;
    if (mine) {
        const GrisGeo* cg = &gb.geo[idx];
        if (near_zero3(cg->x1)) mine = false;
        else {
            dm_rng rng = dm_rng_init(fp.seed, fp.frame, (uint32_t)(v * fp.W + u), 1u);
            (void)dm_rng_f32(&rng);  // start_index draw (:827), value unused
            s_radius[wave][lane] = dm_rng_f32(&rng);
            accepted = cg->pad;
            walk = accepted & gb.src[idx].pad2;
            Reservoir c;
            c.z.F = gb.src[idx].F; c.M = gb.src[idx].M;
            const_term = gris_first_const_term(c, max_taps);
        }
    }
    // Two rounds, the pixels of lanes 0-31 and then of lanes 32-63 (VRT_GRIS_FIRST_ROUNDS = 2: a list of 32 x 32 entries per wave
    // -- 16 KB per workgroup instead of 32 -- so that LDS leaves room for more waves per SIMD; 1: the whole wave's pixels at once).
    float canonical_mis = 1.0f;
    constexpr int ROUNDS = VRT_GRIS_FIRST_ROUNDS, PER = 64 / ROUNDS;
    for (int round = 0; round < ROUNDS; round++) {
        const bool in_round = lane / PER == round;
        // where this lane's items start in the wave's list: exclusive prefix sum of the counts
        const int cnt = in_round ? __builtin_popcount(walk) : 0;
        int incl = cnt;
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        const int base = incl - cnt;
        const int total = __shfl(incl, 63, 64);
        if (in_round) {
            int k = base;
            for (unsigned m = walk; m != 0u; m &= m - 1u) item[k++] = ((uint32_t)lane << 8) | (uint32_t)__builtin_ctz(m);
        }
        wave_lds_sync();
        for (int k0 = 0; k0 < total; k0 += 64) {
            const int k = k0 + lane;
            if (k < total) {
                const uint32_t e = item[k];
                const int q = (int)(e >> 8), i = (int)(e & 31u);
                const int uq = u0 + (q & 7), vq = v0 + (q >> 3);
                int tx, ty;
                (void)gris_tap(fp, taps, uq, vq, i, s_radius[wave][q], max_radius, max_taps, tx, ty);
                Reservoir center;
                f3 center_rc_ty, center_sky_t;
                RcPre center_pre;
                gris_load_src(center, center_rc_ty, center_sky_t, center_pre, gb.src[(vq - fp.row0) * fp.W + uq]);
                item[k] = dm_f2u(gris_first_term(fp, scl, gbl, center, center_rc_ty, center_sky_t, center_pre, tx, ty, max_taps, ts));
            }
        }
        wave_lds_sync();
        if (mine && in_round) {
            int k = base;
            for (unsigned m = accepted; m != 0u; m &= m - 1u) {
                const int i = __builtin_ctz(m);
                canonical_mis += ((walk >> i) & 1u) ? dm_u2f(item[k++]) : const_term;
            }
            gb.geo[idx].pad3 = dm_f2u(canonical_mis);
        }
        wave_lds_sync();   // (the list is written again by the next round)
    }
    if (INSTR) flush_stats(ts, sc.counters);
}

// split pass, before its two kernels: masks of accepted and of live taps per pixel (gris_classify_pixel).  Same tiling as k_gris:
// a wave is one 8x8 tile of the tap-angle hash.
#ifndef VRT_CLASSIFY_MIN_WAVES
#define VRT_CLASSIFY_MIN_WAVES 4
#endif
template <bool INSTR>
__global__ __launch_bounds__(256, VRT_CLASSIFY_MIN_WAVES) void k_gris_classify(FrameParams fp, SceneData sc, GrisBuffers gb, int r0, int r_first, int r1, int tiles_x, int band_w) {
    __shared__ float s_cs[4][64];
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int bx = xcd * band_w + slot % band_w, by = slot / band_w;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int u = bx * 16 + (wave & 1) * 8 + (lane & 7);
    const int v = r0 + by * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (lane < 32) gris_tap_cs(u, v, 0, lane, s_cs[wave]);
    __syncthreads();
    GrisTaps taps;
    taps.cs = s_cs[wave]; taps.off = nullptr; taps.off_stride = 0;
    TraceStats ts;
    stats_zero(ts);
    if (bx < tiles_x && u < fp.W && v >= r_first && v < r1) gris_classify_pixel(fp, gb, taps, u, v, 24.0f, 32, ts);
    if (INSTR) flush_stats(ts, sc.counters);
}

// once per pixel of every row the launch holds: the records k_gris reads ~32 times per pixel (vrt_restir.h)
__global__ __launch_bounds__(256) void k_gris_prepare(FrameParams fp, SceneData sc, GrisBuffers gb) {
    const int u = blockIdx.x * 64 + (threadIdx.x & 63);
    const int v = fp.row0 + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (u < fp.W && v < fp.row1) gris_prepare_pixel(fp, sc, gb, u, v);
}
__global__ void k_mat_derived(const float* mats, float* mats_x) {
    const int id = threadIdx.x;
    if (id < 128) { const Material m = load_material(mats, id); store_mat_derived(mats_x, id, mat_derive(m), material_unit_range(m)); }
}

// ---- temporal accumulation + presentation ------------------------------------------------------
// Register budgets chosen together (overlapped launches, vrt_api.hip): two pooled render waves at 208 registers leave
// 96 of a SIMD's 512, which is what this kernel is held to, so that a temporal pass runs on the same CUs BESIDE the next
// render launch instead of waiting for its persistent workgroups to retire.  (A 48-register build beside 232-register
// render waves was the first version: its spills made it 1.2 ms long beside a launch; this one measured 4 % faster.
// Raising its waves' priority with s_setprio measured 2.5 % slower.)
#ifndef VRT_TEMPORAL_HALF_VGPRS
#define VRT_TEMPORAL_HALF_VGPRS 48   // the attribute counts half of the unified register file
#endif
// Workgroups of VRT_TEMPORAL_ROWS waves (one image row each).  One: beside a render launch a SIMD has room for one wave of this
// kernel, and a workgroup of four waits until all four SIMDs of a CU have theirs free at once (one-wave workgroups: the frame's
// upper rows as a rank's tile +4 %, one-sample calls +2 %, the whole frame unchanged; profiles/r04_zj_*).
#ifndef VRT_TEMPORAL_ROWS
#define VRT_TEMPORAL_ROWS 1
#endif
__global__ __launch_bounds__(64 * VRT_TEMPORAL_ROWS) __attribute__((amdgpu_num_vgpr(VRT_TEMPORAL_HALF_VGPRS))) void k_temporal(FrameParams fp, TemporalBuffers tb, int r0, int r1, int n_samples) {
    const int u = blockIdx.x * 64 + (threadIdx.x & 63);
    const int v = r0 + blockIdx.y * VRT_TEMPORAL_ROWS + (threadIdx.x >> 6);
    if (u < fp.W && v < r1) temporal_pixel(fp, tb, u, v, n_samples);
}
// the same pass over a striped context's OWN rows (vrt_set_row_stripes): n_own of them, stripe after stripe, in ONE launch (a launch
// per stripe put 17 dispatches on the context's stream per step of an eighth of 1080p in 8-row stripes: 0.66 ms a step for 0.19)
__global__ __launch_bounds__(64 * VRT_TEMPORAL_ROWS) __attribute__((amdgpu_num_vgpr(VRT_TEMPORAL_HALF_VGPRS))) void k_temporal_stripes(FrameParams fp, TemporalBuffers tb, int n_own, int n_samples) {
    const int u = blockIdx.x * 64 + (threadIdx.x & 63);
    const int k = blockIdx.y * VRT_TEMPORAL_ROWS + (threadIdx.x >> 6);
    if (k >= n_own) return;
    const int v = (k / fp.stripe_rows) * fp.stripe_period + fp.stripe_first + k % fp.stripe_rows;
    if (u < fp.W && v < fp.H) temporal_pixel<true>(fp, tb, u, v, n_samples);
}
// the moving-camera pass of a row tile with history exchange (vrt_set_history_exchange): the previous frame's histories and
// g-buffer come from whole-frame planes (the reprojected taps land on any row), the rest from the tile's own + halo rows
__global__ __launch_bounds__(64 * VRT_TEMPORAL_ROWS) __attribute__((amdgpu_num_vgpr(VRT_TEMPORAL_HALF_VGPRS))) void k_temporal_frame_prev(FrameParams fp, TemporalBuffers tb, int r0, int r1, int n_samples) {
    const int u = blockIdx.x * 64 + (threadIdx.x & 63);
    const int v = r0 + blockIdx.y * VRT_TEMPORAL_ROWS + (threadIdx.x >> 6);
    if (u < fp.W && v < r1) temporal_pixel<false, true>(fp, tb, u, v, n_samples);
}
// the passes of up to VRT_MAX_GROUP consecutive render launches as one (static camera at render scale 1; the slices are kernel
// arguments: nothing is copied to the device for them).  Same register budget and workgroup shape as k_temporal: it runs in the
// same place, beside two render waves.
__global__ __launch_bounds__(64 * VRT_TEMPORAL_ROWS) __attribute__((amdgpu_num_vgpr(VRT_TEMPORAL_HALF_VGPRS))) void k_temporal_group(TemporalGroup tg, int r0, int r1) {
    const int u = blockIdx.x * 64 + (threadIdx.x & 63);
    const int v = r0 + blockIdx.y * VRT_TEMPORAL_ROWS + (threadIdx.x >> 6);
    if (u < tg.W && v < r1) temporal_group_pixel(tg, u, v);
}
__global__ __launch_bounds__(256) void k_tonemap(FrameParams fp, const f3* hdr, f4* ldr, int r0, int r1) {
    const int u = blockIdx.x * 64 + (threadIdx.x & 63);
    const int v = r0 + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (u < fp.W && v < r1) ldr[(v - fp.row0) * fp.W + u] = tonemap_pixel(fp, hdr, u, v);
}
// the same image as 8-bit rgba for a display or a PNG: u8(clamp(c, 0, 1) * 255 + 0.5), the conversion scene.py's image writer does
__global__ __launch_bounds__(256) void k_tonemap8(FrameParams fp, const f3* hdr, uint32_t* ldr8, int r0, int r1) {
    const int u = blockIdx.x * 64 + (threadIdx.x & 63);
    const int v = r0 + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (u < fp.W && v < r1) {
        const f4 c = tonemap_pixel(fp, hdr, u, v);
        ldr8[(v - fp.row0) * fp.W + u] = dm_f2u32(dm_saturate(c.x) * 255.0f + 0.5f) | (dm_f2u32(dm_saturate(c.y) * 255.0f + 0.5f) << 8) |
                                         (dm_f2u32(dm_saturate(c.z) * 255.0f + 0.5f) << 16) | (dm_f2u32(dm_saturate(c.w) * 255.0f + 0.5f) << 24);
    }
}
// ---- vrt_denoise (vrt_denoise.h) ---------------------------------------------------------------------------------------------------
// Step 1 of every pixel, and the ONLY kernel of the pass that reads planes the render launches and their passes write: the guide record,
// the material word and the two signals go to the pass's own scratch, and a pixel that is no surface pixel gets its HDR value here.
__global__ __launch_bounds__(256) void k_denoise_prepare(int W, int H, int moving, DenoiseSource src, DenoiseGuide* __restrict__ guide, uint32_t* __restrict__ mat,
                                                         f4* __restrict__ d, f4* __restrict__ s, f3* __restrict__ out) {
    const int u = blockIdx.x * 64 + (threadIdx.x & 63);
    const int v = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (u >= W || v >= H) return;
    const int idx = v * W + u;
    const uint32_t M = src.gb_mat[idx];
    DenoiseGuide g;
    f4 xd, xs;
    const bool surface = denoise_prepare(src.gb_pos[idx], src.gb_normal[idx], M, src.hist_d[idx], src.hist_s[idx], moving, g, xd, xs);
    guide[idx] = g;
    mat[idx] = M;
    d[idx] = xd;
    s[idx] = xs;
    if (!surface) out[idx] = src.hdr[idx];
}
// One iteration at stride S: a 32 x 8 pixel tile per workgroup, a pixel a lane, the 25 taps gathered from global memory (DESIGN.md
// section 4 says why not through LDS).  The last iteration (out != nullptr) goes on to step 3 and writes the surface pixels of the
// result instead of the signals; u_d / u_s: step 1's values.
template <int S>
__global__ __launch_bounds__(256) void k_denoise_atrous(DenoiseIn in, DenoiseSettings st, int use_lum, f4* __restrict__ d_out, f4* __restrict__ s_out,
                                                        const f4* __restrict__ u_d, const f4* __restrict__ u_s, f3* __restrict__ out) {
    const int u = blockIdx.x * 32 + (threadIdx.x & 31);
    const int v = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (u >= in.W || v >= in.H) return;
    const int idx = v * in.W + u;
    f4 xd, xs;
    const bool surface = denoise_iteration(in, u, v, S, use_lum != 0, st.sigma_l, st.tol, xd, xs);
    if (out) {
        if (surface) out[idx] = denoise_finish(xd, xs, u_d[idx], u_s[idx], in.mat[idx], st.moving, st.full_at);
    } else {
        d_out[idx] = xd;
        s_out[idx] = xs;
    }
}
#if defined(VRT_DIAG_REGIONS)
__global__ void k_diag_read(unsigned long long* out, int reset) {
    int i = threadIdx.x;
    if (i < 64) { out[i] = g_vrt_region[i]; if (reset) g_vrt_region[i] = 0ULL; }
}
#endif
hipError_t launch_diag_read(hipStream_t st, unsigned long long* out, int reset) {
#if defined(VRT_DIAG_REGIONS)
    hipLaunchKernelGGL(k_diag_read, dim3(1), dim3(64), 0, st, out, reset);
    return hipGetLastError();
#else
    (void)st; (void)out; (void)reset;
    return hipErrorNotSupported;
#endif
}

// ---- host-side launchers -----------------------------------------------------------------------
hipError_t query_render_residency(int grid_res, bool restir, bool instr, int* blocks_per_cu) {
    hipError_t e = hipSuccess;
    VRT_BY_GRID(grid_res, VRT_BY_2(restir, instr, e = hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_render<G, A, B>, VRT_RENDER_THREADS, 0)));
    return e;
}

hipError_t launch_render(hipStream_t st, int grid_res, bool restir, bool instr, int n_blocks, const FrameParams& fp, const SceneData& sc,
                         const PixelBuffers& out, unsigned* work_counters, unsigned launch_seq, int n_samples, int chunk_override) {
    // sixteen sets of heads rotate: launch k counts on set k % 16 and zeroes set (k + 8) % 16 -- up to four launches are in
    // flight together (vrt_accumulate) and none of their sets may be touched; launch k + 8 runs on launch k's stream (the
    // pipeline is 2 or 4 streams deep), so its set is clean before it starts whatever the other streams do
    unsigned* work_counter = work_counters + (launch_seq & 15u) * (VRT_WORK_HEADS * VRT_WORK_HEAD_STRIDE);  // the fused kernel uses head 0 only
    unsigned* next_counter = work_counters + ((launch_seq + 8u) & 15u) * (VRT_WORK_HEADS * VRT_WORK_HEAD_STRIDE);
    dim3 g(n_blocks), b(VRT_RENDER_THREADS);
    // pixels a wave reserves per atomic: whole 8x8 tiles.  One tile keeps the tail short (measured: 192-pixel chunks
    // cost 13 % at 1080p on the sparse scene) and still cuts the atomic rate ~3x against per-refill atomics, which
    // is what the dense 4K frame needed (67 -> 22 dequeues/us, 5.9 -> 4.8 ms).  chunk_override: development builds (VRT_CHUNK).
    const unsigned chunk = chunk_override > 0 ? (unsigned)chunk_override : 64u;
    VRT_BY_GRID(grid_res, VRT_BY_2(restir, instr, hipLaunchKernelGGL((k_render<G, A, B>), g, b, 0, st, fp, sc, out, work_counter, next_counter, chunk, n_samples)));
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
// The ONE place a pooled launch's variant (plan_render_variant, vrt_plan.h) becomes a kernel and its geometry: block size, residency,
// scratch size.  (restir: the reservoir needs the light sample whatever the sun's colour.)
typedef void (*pool_kernel_fn)(FrameParams, SceneData, PixelBuffers, unsigned*, unsigned*, int, uint32_t*, uint32_t*, uint32_t, PrimaryRecord*);
struct PoolKernel { pool_kernel_fn fn; PoolShape shape; };
static PoolKernel pool_kernel(int grid_res, const RenderVariant& v, bool served = false) {
    PoolKernel k{nullptr, {0, 0}};
    if (served && !v.instr && !v.restir && !v.dense12) {   // (plan_prepass names no other launch; same geometry and residency as the plain instantiation)
        VRT_BY_GRID(grid_res, VRT_BY_2(v.black_sun, v.cull, k = (PoolKernel{k_render_pool<G, false, A, B, true>, pool_shape<G>(false)})));
        return k;
    }
    VRT_BY_GRID(grid_res, VRT_BY_2(v.instr, v.cull,
        k = (v.restir ? PoolKernel{k_render_pool_restir<G, A, B>, pool_shape<G>(false)}
           : v.dense12 ? PoolKernel{k_render_pool_dense12<G, A, B>, pool_shape<G>(true)}
           : v.black_sun ? PoolKernel{k_render_pool<G, A, true, B>, pool_shape<G>(false)}
                         : PoolKernel{k_render_pool<G, A, false, B>, pool_shape<G>(false)})));
    return k;
}
hipError_t query_render_pool(int grid_res, const RenderVariant& v, int* blocks_per_cu, size_t* scratch_per_block) {
    const PoolKernel k = pool_kernel(grid_res, v);
    *scratch_per_block = (size_t)k.shape.waves * k.shape.slots * (v.restir ? ColdLine<true>::count : ColdLine<false>::count) * sizeof(uint32_t);
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k.fn, 64 * k.shape.waves, 0);
}
hipError_t launch_render_pool(hipStream_t st, int grid_res, const RenderVariant& v, int n_blocks, const FrameParams& fp, const SceneData& sc,
                              const PixelBuffers& out, unsigned* work_counters, unsigned launch_seq, int n_samples, uint32_t* cold,
                              uint32_t* drain_signal, PrimaryRecord* prim_cache, bool prim_served) {
    unsigned* work_counter = work_counters + (launch_seq & 15u) * (VRT_WORK_HEADS * VRT_WORK_HEAD_STRIDE);
    unsigned* next_counter = work_counters + ((launch_seq + 8u) & 15u) * (VRT_WORK_HEADS * VRT_WORK_HEAD_STRIDE);
    const PoolKernel k = pool_kernel(grid_res, v, prim_served);
    // the signal carries launch_seq + 1 of the latest launch that has begun to drain
    hipLaunchKernelGGL(k.fn, dim3(n_blocks), dim3(64 * k.shape.waves), 0, st, fp, sc, out, work_counter, next_counter, n_samples, cold, drain_signal, launch_seq + 1u, prim_cache);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
hipError_t launch_primary_records(hipStream_t st, int grid_res, const RenderVariant& v, const FrameParams& fp, const SceneData& sc, PrimaryRecord* prim_cache,
                                  unsigned launch_seq) {
    const int tiles = ((fp.W + 7) >> 3) * launch_tile_rows(fp);
    if (tiles <= 0) return hipSuccess;
    // the tag the launch itself will look for (launch_render_pool): launch_seq + 1
    VRT_BY_GRID(grid_res, VRT_BY_2(v.cull, false, hipLaunchKernelGGL((k_primary_records<G, A>), dim3(tiles), dim3(64), 0, st, fp, sc, prim_cache, launch_seq + 1u)));
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
hipError_t launch_primary_vertex(hipStream_t st, int grid_res, const RenderVariant& v, const FrameParams& fp, const SceneData& sc, const PixelBuffers& out,
                                 const PrimaryRecord* prim_cache, unsigned launch_seq, int n_samples, const PrimaryQueue& pq) {
    const int tiles = ((fp.W + 7) >> 3) * launch_tile_rows(fp);
    if (tiles <= 0) return hipSuccess;
    if (v.black_sun) VRT_BY_GRID(grid_res, VRT_BY_2(v.cull, false, hipLaunchKernelGGL((k_primary_vertex<G, A>), dim3(tiles), dim3(64), 0, st, fp, sc, out, prim_cache, launch_seq + 1u, n_samples, pq)));
    else VRT_BY_GRID(grid_res, VRT_BY_2(v.cull, false, hipLaunchKernelGGL((k_primary_vertex_sun<G, A>), dim3(tiles), dim3(64), 0, st, fp, sc, out, prim_cache, launch_seq + 1u, n_samples, pq)));
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
hipError_t launch_render_pool_queued(hipStream_t st, int grid_res, const RenderVariant& v, int n_blocks, const FrameParams& fp, const SceneData& sc,
                                     const PixelBuffers& out, unsigned* work_counters, unsigned launch_seq, int n_samples, uint32_t* cold,
                                     uint32_t* drain_signal, PrimaryRecord* prim_cache, const PrimaryQueue& pq) {
    unsigned* work_counter = work_counters + (launch_seq & 15u) * (VRT_WORK_HEADS * VRT_WORK_HEAD_STRIDE);
    unsigned* next_counter = work_counters + ((launch_seq + 8u) & 15u) * (VRT_WORK_HEADS * VRT_WORK_HEAD_STRIDE);
    VRT_BY_GRID(grid_res, VRT_BY_2(v.black_sun, v.cull, hipLaunchKernelGGL((k_render_pool_queued<G, A, B>), dim3(n_blocks), dim3(64 * pool_shape<G>(false).waves), 0, st, fp, sc, out,
                                                                         work_counter, next_counter, n_samples, cold, drain_signal, launch_seq + 1u, prim_cache, pq)));
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
#if defined(VRT_DEV_KNOBS)
// Test hook of the development build (VRT_TEST_SPOIL_RECORDS=N, vrt_plan.h; tests/test_gpu_primary_routes.py): behind a launch's pre-pass,
// ahead of everything that reads its records, the records of the live pixels -- k_primary_records' own gating -- whose index in the
// table is launch_number mod N (mod N) have bit 0 of their check word inverted, so that they fail primary_record_valid under every tag
// that the payload passed with.  What the design says of a missing, stale or torn record (vrt_pool.h) then has to hold: k_primary_vertex
// makes every sample of such a pixel a leftover, and the pool begins it from depth 0, g-buffer and record included.  N = 1: every record.
__global__ __launch_bounds__(64) void k_spoil_primary_records(FrameParams fp, PrimaryRecord* prim_cache, uint32_t n, uint32_t launch_number) {
    const int tiles_x = (fp.W + 7) >> 3;
    const unsigned tile = blockIdx.x, in = threadIdx.x;
    const int u = (int)(tile % (unsigned)tiles_x) * 8 + (int)(in & 7u);
    const int v = launch_tile_row(fp, (int)(tile / (unsigned)tiles_x)) + (int)(in >> 3);
    if (!(u < fp.W && v < fp.row1 && launch_renders_row(fp, v) && !outside_render_area(fp, (float)u, (float)v))) return;
    const uint32_t i = (uint32_t)((v - fp.row0) * fp.W + u);
    if (i % n != launch_number % n) return;
    prim_cache[i].w ^= 1u;
}
hipError_t launch_spoil_primary_records(hipStream_t st, const FrameParams& fp, PrimaryRecord* prim_cache, unsigned n, unsigned launch_number) {
    const int tiles = ((fp.W + 7) >> 3) * launch_tile_rows(fp);
    if (tiles <= 0 || n == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_spoil_primary_records, dim3(tiles), dim3(64), 0, st, fp, prim_cache, (uint32_t)n, (uint32_t)launch_number);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
#endif
hipError_t launch_mat_derived(hipStream_t st, const float* mats, float* mats_x) {
    hipLaunchKernelGGL(k_mat_derived, dim3(1), dim3(128), 0, st, mats, mats_x);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
hipError_t launch_gris(hipStream_t st, int grid_res, bool instr, const FrameParams& fp, const SceneData& sc, const GrisBuffers& gb, int r0, int r1) {
    hipLaunchKernelGGL(k_gris_prepare, dim3((fp.W + 63) / 64, (fp.row1 - fp.row0 + 3) / 4), dim3(256), 0, st, fp, sc, gb);
    // the tap angles of a pixel are hashed from its 8x8 tile in FRAME coordinates (pathtracer.py:834-836) and worked out once
    // per wave: the wave tiles have to sit on that grid, so the launch starts at the multiple of 8 at or below r0
    const int ra = r0 & ~7;
    const int tiles_x = (fp.W + 15) / 16, tiles_y = (r1 - ra + 15) / 16, band_w = (tiles_x + 7) / 8;
    dim3 g(8 * band_w * tiles_y), b(256);
#if VRT_GRIS_SPLIT
    if (instr) hipLaunchKernelGGL((k_gris_classify<true>), g, b, 0, st, fp, sc, gb, ra, r0, r1, tiles_x, band_w);
    else hipLaunchKernelGGL((k_gris_classify<false>), g, b, 0, st, fp, sc, gb, ra, r0, r1, tiles_x, band_w);
    VRT_BY_GRID(grid_res, VRT_BY_2(instr, false, hipLaunchKernelGGL((k_gris_first<G, A>), g, b, 0, st, fp, sc, gb, ra, r0, r1, tiles_x, band_w)));
    VRT_BY_GRID(grid_res, VRT_BY_2(instr, false, hipLaunchKernelGGL((k_gris<G, A, 2>), g, b, 0, st, fp, sc, gb, ra, r0, r1, tiles_x, band_w)));
#else
    VRT_BY_GRID(grid_res, VRT_BY_2(instr, false, hipLaunchKernelGGL((k_gris<G, A>), g, b, 0, st, fp, sc, gb, ra, r0, r1, tiles_x, band_w)));
#endif
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
hipError_t launch_temporal(hipStream_t st, const FrameParams& fp, const TemporalBuffers& tb, int r0, int r1, int n_samples, bool frame_prev) {
    dim3 g((fp.W + 63) / 64, (r1 - r0 + VRT_TEMPORAL_ROWS - 1) / VRT_TEMPORAL_ROWS), b(64 * VRT_TEMPORAL_ROWS);
    if (frame_prev) hipLaunchKernelGGL(k_temporal_frame_prev, g, b, 0, st, fp, tb, r0, r1, n_samples);
    else if (fp.stripe_period) hipLaunchKernelGGL(k_temporal_stripes, g, b, 0, st, fp, tb, r1 - r0, n_samples);   // (r0 = 0, r1 = the context's own rows)
    else hipLaunchKernelGGL(k_temporal, g, b, 0, st, fp, tb, r0, r1, n_samples);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
hipError_t launch_temporal_group(hipStream_t st, const TemporalGroup& tg, int r0, int r1) {
    if (tg.n_slices < 1 || tg.n_slices > VRT_MAX_GROUP || r0 < tg.row0 || r1 > tg.row1) return hipErrorInvalidValue;
    dim3 g((tg.W + 63) / 64, (r1 - r0 + VRT_TEMPORAL_ROWS - 1) / VRT_TEMPORAL_ROWS), b(64 * VRT_TEMPORAL_ROWS);
    hipLaunchKernelGGL(k_temporal_group, g, b, 0, st, tg, r0, r1);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
hipError_t launch_tonemap(hipStream_t st, const FrameParams& fp, const f3* hdr, f4* ldr, int r0, int r1) {
    dim3 g((fp.W + 63) / 64, (r1 - r0 + 3) / 4), b(256);
    hipLaunchKernelGGL(k_tonemap, g, b, 0, st, fp, hdr, ldr, r0, r1);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
hipError_t launch_tonemap8(hipStream_t st, const FrameParams& fp, const f3* hdr, uint32_t* ldr8, int r0, int r1) {
    dim3 g((fp.W + 63) / 64, (r1 - r0 + 3) / 4), b(256);
    hipLaunchKernelGGL(k_tonemap8, g, b, 0, st, fp, hdr, ldr8, r0, r1);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
hipError_t launch_denoise_prepare(hipStream_t st, int W, int H, int moving, const DenoiseSource& src, const DenoiseScratch& scr, f3* out) {
    dim3 g((W + 63) / 64, (H + 3) / 4), b(256);
    hipLaunchKernelGGL(k_denoise_prepare, g, b, 0, st, W, H, moving, src, scr.guide, scr.mat, scr.d[0], scr.s[0], out);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
hipError_t launch_denoise_filter(hipStream_t st, int W, int H, const DenoiseSettings& set, const DenoiseScratch& scr, f3* out) {
    dim3 g((W + 31) / 32, (H + 7) / 8), b(256);
    int from = 0;   // the copy iteration i reads: step 1's, then the two others in turn
    for (int i = 0; i < set.iterations; i++) {
        const int to = from == 1 ? 2 : 1;
        const DenoiseIn in{scr.guide, scr.mat, scr.d[from], scr.s[from], W, H};
        const int use_lum = i >= 1 && set.sigma_l > 0.0f;
        f3* const last = i == set.iterations - 1 ? out : nullptr;
#define VRT_DENOISE_AT(S_) hipLaunchKernelGGL(k_denoise_atrous<S_>, g, b, 0, st, in, set, use_lum, scr.d[to], scr.s[to], scr.d[0], scr.s[0], last)
        switch (i) {
            case 0: VRT_DENOISE_AT(1); break;
            case 1: VRT_DENOISE_AT(2); break;
            case 2: VRT_DENOISE_AT(4); break;
            case 3: VRT_DENOISE_AT(8); break;
            case 4: VRT_DENOISE_AT(16); break;
            case 5: VRT_DENOISE_AT(32); break;
            default: return hipErrorInvalidValue;
        }
#undef VRT_DENOISE_AT
        VRT_LAUNCH_CHECK();
        from = to;
    }
    return hipSuccess;
}

}  // namespace vrt
