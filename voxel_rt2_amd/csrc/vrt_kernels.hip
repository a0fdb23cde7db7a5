// vrt_kernels.hip -- gfx950 kernels of libvrt_hip.so.
//
//   k_pack_grid / k_build_l0 / k_build_coarse / k_build_l0c   prepare_data: packed voxel texels, the bit-brick
//                                                         occupancy pyramid and its compacted fine level
//   k_render_pool / _restir / _dense12                    persistent wave64 path tracer, pooled schedule (vrt_pool.h): a wave owns a
//                                                         pool of path records in LDS and runs them stage by stage (WALK / SHADE /
//                                                         ESCAPE / BEGIN); the default.  Which of them: plan_render_variant, pool_kernel()
//   k_render<RESTIR, INSTR>                               persistent wave64 path tracer, one path per lane (vrt_path.h)
//   k_gris_prepare / k_gris                               ReSTIR spatial reuse: per-pixel records (decoded sample, shading
//                                                         basis), then 32 taps x 2 reconnection shifts per pixel
//   k_mat_derived                                         per-material-id part of a shading point (after material uploads)
//   k_temporal                                            fused temporal accumulation -> HDR (sized to run beside
//                                                         the next render launch, see vrt_api.hip)
//   k_temporal_frame_prev                                 the same, moving camera on a row tile with history exchange
//   k_temporal_group                                      the passes of several consecutive launches in one (static camera)
//   k_tonemap                                             LDR presentation
//   k_cast_rays / k_fetch_voxels                          vrt_cast_rays: caller-supplied rays through next_hit; vrt_fetch_voxels
//   k_sweep_boxes                                         vrt_sweep_boxes: caller-supplied boxes moved through the pyramid, a wave a box
//   k_trace_radiance                                      vrt_trace_radiance: caller-supplied rays through the path state machine
//   k_gather_irradiance                                   vrt_gather_irradiance: a sun sample and a hemisphere path per (sensor, sample)
//   k_gather_probes                                       vrt_gather_probes: a sun sample and a sphere path per (probe, sample)
//   k_fold_query<Q>                                       the ordered sums of any of the three (vrt_query.h)
//   k_dist_z / k_dist_y / k_dist_x                        vrt_distance_field: the three line passes of the exact distance transform
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
#include <atomic>
#include "vrt_kernels.h"
#include "vrt_probe.h"
#include "vrt_shade_probe.h"

namespace vrt {

// ---- prepare_data ----------------------------------------------------------------------------
// voxel_world.py:69-87: rgba8 texel per voxel; a negative material byte stores 0 (unorm clamp)
template <int G>
__global__ void k_pack_grid(const int8_t* __restrict__ mat, const uint8_t* __restrict__ rgb, uint32_t* __restrict__ grid) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;  // [x][y][z], the order of the uploaded arrays
    if (i >= G * G * G) return;
    int m = mat[i];
    uint32_t a = (m < 0) ? 0u : (uint32_t)m;
    const int z = i & (G - 1), y = (i / G) & (G - 1), x = i / (G * G);
    grid[texel_index<G>(x, y, z)] = (uint32_t)rgb[3 * i] | ((uint32_t)rgb[3 * i + 1] << 8) | ((uint32_t)rgb[3 * i + 2] << 16) | (a << 24);
}
// raytracer.py:46-53: LOD-0 bit = voxel_material > 0 (signed), gathered into one 4x4x4 brick word per thread
__global__ void k_build_l0(const int8_t* __restrict__ mat, unsigned long long* __restrict__ l0, int G) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int n0 = G >> 2;
    if (b >= n0 * n0 * n0) return;
    int bx = b % n0, by = (b / n0) % n0, bz = b / (n0 * n0);
    unsigned long long w = 0ULL;
    for (int z = 0; z < 4; z++)
        for (int y = 0; y < 4; y++)
            for (int x = 0; x < 4; x++) {
                int vx = bx * 4 + x, vy = by * 4 + y, vz = bz * 4 + z;
                if (mat[(vx * G + vy) * G + vz] > 0) w |= 1ULL << (z * 16 + y * 4 + x);
            }
    l0[b] = w;
}
// raytracer.py:54-70: a coarser cell is occupied if any child is; here one bit per non-zero child word
__global__ void k_build_coarse(const unsigned long long* __restrict__ fine, unsigned long long* __restrict__ coarse, int n_coarse) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    int total = n_coarse * n_coarse * n_coarse;
    if (b >= total) return;
    int n_fine = n_coarse * 4;
    int bx = b % n_coarse, by = (b / n_coarse) % n_coarse, bz = b / (n_coarse * n_coarse);
    unsigned long long w = 0ULL;
    for (int z = 0; z < 4; z++)
        for (int y = 0; y < 4; y++)
            for (int x = 0; x < 4; x++) {
                int fx = bx * 4 + x, fy = by * 4 + y, fz = bz * 4 + z;
                if (fine[(fz * n_fine + fy) * n_fine + fx] != 0ULL) w |= 1ULL << (z * 16 + y * 4 + x);
            }
    coarse[b] = w;
}

// Bounding box of the solid voxels (brick granular) grown by VRT_CULL_MARGIN: what cull_ray() (vrt_trace.h) tests rays against.
// One block; an empty grid gives lo > hi.
__global__ void k_cull_box(const unsigned long long* __restrict__ l0, int n0, float* __restrict__ out) {
    __shared__ int s_lo[3][256], s_hi[3][256];
    __shared__ int s_cnt[256];
    int cnt = 0;   // non-empty bricks
    int lo[3] = {1 << 20, 1 << 20, 1 << 20}, hi[3] = {-(1 << 20), -(1 << 20), -(1 << 20)};
    for (int b = threadIdx.x; b < n0 * n0 * n0; b += blockDim.x) {
        if (l0[b] == 0ULL) continue;
        cnt++;
        const int c[3] = {b % n0, (b / n0) % n0, b / (n0 * n0)};
        for (int a = 0; a < 3; a++) { lo[a] = min(lo[a], c[a] * 4); hi[a] = max(hi[a], c[a] * 4 + 4); }
    }
    for (int a = 0; a < 3; a++) { s_lo[a][threadIdx.x] = lo[a]; s_hi[a][threadIdx.x] = hi[a]; }
    s_cnt[threadIdx.x] = cnt;
    __syncthreads();
    if (threadIdx.x < 3) {
        int l = 1 << 20, h = -(1 << 20);
        for (int i = 0; i < 256; i++) { l = min(l, s_lo[threadIdx.x][i]); h = max(h, s_hi[threadIdx.x][i]); }
        out[threadIdx.x] = (float)l - VRT_CULL_MARGIN;
        out[3 + threadIdx.x] = (float)h + VRT_CULL_MARGIN;
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // is there anything to cull: does the grown box leave part of the grid out
        const float G = (float)(n0 * 4);
        bool some = false;
        for (int a = 0; a < 3; a++) some = some || out[a] > 0.0f || out[3 + a] < G;
        out[6] = some ? 1.0f : 0.0f;
        int total = 0;
        for (int i = 0; i < 256; i++) total += s_cnt[i];
        out[7] = (float)total / (float)(n0 * n0 * n0);   // share of non-empty 4x4x4 bricks (read by the host: which SHADE variant; cull_ray does not look at it)
    }
}

// The fine level without its empty words (Pyramid::l0c, vrt_types.h).  One block of 512 threads, thread i = l1 brick i:
// exclusive prefix sum of the popcounts, then each thread copies the words behind its set bits in bit order.
__global__ void k_build_l0c(const unsigned long long* __restrict__ l0, const unsigned long long* __restrict__ l1,
                            unsigned long long* __restrict__ l0c, uint32_t* __restrict__ base) {
    __shared__ uint32_t s_scan[512];
    const int i = threadIdx.x;
    const unsigned long long w = l1[i];
    const uint32_t cnt = (uint32_t)__popcll(w);
    s_scan[i] = cnt;
    __syncthreads();
    for (int off = 1; off < 512; off <<= 1) {  // Hillis-Steele inclusive scan
        const uint32_t v = (i >= off) ? s_scan[i - off] : 0u;
        __syncthreads();
        s_scan[i] += v;
        __syncthreads();
    }
    const uint32_t first = s_scan[i] - cnt;
    base[i] = first;
    if (i == 511) base[512] = s_scan[511];
    const int bx1 = i & 7, by1 = (i >> 3) & 7, bz1 = i >> 6;
    uint32_t k = first;
    for (int b = 0; b < 64; b++) {
        if ((w >> b) & 1ULL) {
            const int bx = bx1 * 4 + (b & 3), by = by1 * 4 + ((b >> 2) & 3), bz = bz1 * 4 + (b >> 4);
            l0c[k++] = l0[(bz * 32 + by) * 32 + bx];
        }
    }
}

// ---- vrt_update_voxels: the same data for a box of voxels (vrt_edit.h holds the arithmetic) -----
// One thread per voxel of the box, z fastest: a wave reads runs of the box arrays and writes runs of hz voxels of the grid's.
template <int G>
__global__ void k_edit_store(EditBox box, const int8_t* __restrict__ box_mat, const uint8_t* __restrict__ box_rgb, int8_t* __restrict__ mat,
                             uint8_t* __restrict__ rgb, uint32_t* __restrict__ grid) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < edit_box_voxels(box)) edit_store_voxel<G>(box, i, box_mat, box_rgb, mat, rgb, grid);
}
// One thread per 4x4x4 brick the box touches.
__global__ void k_edit_fine(EditBox box, const int8_t* __restrict__ mat, unsigned long long* __restrict__ l0, int G) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < edit_cell_count(edit_cells(box, 2))) edit_rebuild_fine(box, i, mat, l0, G);
}
// One thread per word the box touches of the level with cells of (1 << shift) voxels.
__global__ void k_edit_coarse(EditBox box, int shift, const unsigned long long* __restrict__ fine, unsigned long long* __restrict__ coarse, int G) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < edit_cell_count(edit_cells(box, shift))) edit_rebuild_coarse(box, shift, i, fine, coarse, G);
}

// ---- render ----------------------------------------------------------------------------------
// OOB: the instantiation can read cells outside the grid the reference's way (oob_capable_of, vrt_trace.h).  It is the INSTRUMENTED
// instantiations that can (a context with vrt_set_reference_indexing launches those): the timed kernels carry no test for it.
template <int G_, bool OOB_ = false>
struct LdsPyramid {  // coarse levels in LDS, fine level through L2
    static constexpr int G = G_;
    static constexpr bool flat_descend = false;  // its kernels walk with few active lanes: descend()'s early outs win
    static constexpr bool cull = true;
    static constexpr bool oob_capable = OOB_;
    bool oob;   // wave-uniform: Pyramid::ref_oob
    __device__ __forceinline__ bool oob_ref() const { return oob; }
    const unsigned long long* l0;
    const unsigned long long* l1;
    const unsigned long long* l2;
    unsigned long long w3;   // the top word (G = 256), wave-uniform
    __device__ __forceinline__ unsigned long long load_l0(int i) const { return l0[i]; }
    __device__ __forceinline__ unsigned long long load_l1(int i) const { return l1[i]; }
    __device__ __forceinline__ unsigned long long load_l2(int i) const { return l2[i]; }
    __device__ __forceinline__ unsigned long long load_l3() const { return w3; }
};
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
__global__ void k_detmath_probe(int op, int n, const float* a, const float* b, float* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float r = 0.0f;
    switch (op) {
        case 0: r = dm_sin(a[i]); break;
        case 1: r = dm_cos(a[i]); break;
        case 2: r = dm_exp(a[i]); break;
        case 3: r = dm_log(a[i]); break;
        case 4: r = dm_pow(a[i], b[i]); break;
        case 5: r = dm_acos(a[i]); break;
        case 6: r = dm_atan2(a[i], b[i]); break;
        case 7: r = dm_min(a[i], b[i]); break;
        case 8: r = dm_max(a[i], b[i]); break;
        case 9: r = dm_round_f16(a[i]); break;
        case 10: r = a[i] / b[i]; break;
        case 11: r = dm_sqrt(a[i]); break;
        case 12: r = a[i] * b[i] + a[i]; break;  // must NOT contract
        case 13: r = (float)dm_f2i(a[i]); break;
        case 14: r = dm_u2f((uint32_t)dm_f32_to_f16(a[i])); break;             // the half code, as the low bits of the output word
        case 15: r = dm_f16_to_f32((uint16_t)(dm_f2u(a[i]) & 0xffffu)); break;  // input word's low bits = half code
    }
    out[i] = r;
}

// Test hook (vrt_trace_probe): one ray per lane through the closest-hit walk of the pyramid in global memory (vrt_probe.h).
template <int G, int WALK>
__global__ __launch_bounds__(64) void k_trace_probe(Pyramid pyr, const float* cull, int n, const float* rays, ProbeOut* out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    GlobalPyramid<G> P;
    P.p = pyr;
    const float* a = rays + (size_t)i * 6;
    ProbeOut r;
    probe_ray<G, WALK>(P, mk3(a[0], a[1], a[2]), mk3(a[3], a[4], a[5]), cull, r);
    out[i] = r;
}

// Test hook (vrt_shade_probe): one row of arguments per lane through one shading function (vrt_shade_probe.h).
__global__ __launch_bounds__(64) void k_shade_probe(FrameParams fp, SceneData sc, const float* mats_x, int op, int n, const float* in, int in_stride,
                                                    float* out, int out_stride, float* lane_tables) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    shade_probe_row(fp, sc, mats_x, op, in + (size_t)i * in_stride, out + (size_t)i * out_stride, out_stride,
                    lane_tables ? lane_tables + (size_t)i * VRT_SHADE_LANE_TABLE : nullptr);
}

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
// vrt_fetch_voxels: one thread per voxel of the box, z fastest (k_edit_store the other way round)
__global__ void k_fetch_voxels(EditBox box, int G, const int8_t* __restrict__ mat, const uint8_t* __restrict__ rgb, int8_t* __restrict__ box_mat,
                               uint8_t* __restrict__ box_rgb) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < edit_box_voxels(box)) fetch_box_voxel(box, G, i, mat, rgb, box_mat, box_rgb);
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
#define VRT_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; } while (0)

hipError_t launch_prepare(hipStream_t st, int G, const int8_t* mat, const uint8_t* rgb, uint32_t* grid, unsigned long long* l0,
                          unsigned long long* l1, unsigned long long* l2, unsigned long long* l3, unsigned long long* l0c, uint32_t* l0c_base,
                          float* cull) {
    const int n = G * G * G, n0 = G / 4, n1 = G / 16, n2 = G / 64;
    if (G == 256) hipLaunchKernelGGL(k_pack_grid<256>, dim3((n + 255) / 256), dim3(256), 0, st, mat, rgb, grid);
    else hipLaunchKernelGGL(k_pack_grid<128>, dim3((n + 255) / 256), dim3(256), 0, st, mat, rgb, grid);
    VRT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_build_l0, dim3((n0 * n0 * n0 + 255) / 256), dim3(256), 0, st, mat, l0, G);
    VRT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cull_box, dim3(1), dim3(256), 0, st, (const unsigned long long*)l0, n0, cull);
    VRT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_build_coarse, dim3((n1 * n1 * n1 + 255) / 256), dim3(256), 0, st, (const unsigned long long*)l0, l1, n1);
    VRT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_build_coarse, dim3(1), dim3(64), 0, st, (const unsigned long long*)l1, l2, n2);
    VRT_LAUNCH_CHECK();
    if (G == 256) {  // the top word: bit = l2 word non-zero
        hipLaunchKernelGGL(k_build_coarse, dim3(1), dim3(64), 0, st, (const unsigned long long*)l2, l3, 1);
    } else {         // the compacted fine level of the pooled kernel's LDS copy (128^3 only)
        if (n0 * n0 * n0 >= (1 << (VRT_COARSE_BASE_BITS - 4))) return hipErrorInvalidValue;   // l0c_base counts fine words: coarse_pack (vrt_trace.h) keeps it below its level bits
        hipLaunchKernelGGL(k_build_l0c, dim3(1), dim3(512), 0, st, (const unsigned long long*)l0, (const unsigned long long*)l1, l0c, l0c_base);
    }
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}

// What launch_prepare leaves, for a grid that differs from the prepared one inside `box` (valid and not empty: the caller checks).
// Box-sized: store and pack, the fine words, the l1 and l2 words the box touches, each level after the one below it.  Whole-level,
// as in launch_prepare: the l3 word or the compacted fine level (one new brick moves every later word of it), and the culling box --
// they cost bricks, not voxels.
hipError_t launch_edit(hipStream_t st, int G, const EditBox& box, const int8_t* box_mat, const uint8_t* box_rgb, int8_t* mat, uint8_t* rgb,
                       uint32_t* grid, unsigned long long* l0, unsigned long long* l1, unsigned long long* l2, unsigned long long* l3,
                       unsigned long long* l0c, uint32_t* l0c_base, float* cull) {
    const int n = edit_box_voxels(box);
    if (G == 256) hipLaunchKernelGGL(k_edit_store<256>, dim3((n + 255) / 256), dim3(256), 0, st, box, box_mat, box_rgb, mat, rgb, grid);
    else hipLaunchKernelGGL(k_edit_store<128>, dim3((n + 255) / 256), dim3(256), 0, st, box, box_mat, box_rgb, mat, rgb, grid);
    VRT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_edit_fine, dim3((edit_cell_count(edit_cells(box, 2)) + 63) / 64), dim3(64), 0, st, box, (const int8_t*)mat, l0, G);
    VRT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_edit_coarse, dim3((edit_cell_count(edit_cells(box, 4)) + 63) / 64), dim3(64), 0, st, box, 4, (const unsigned long long*)l0, l1, G);
    VRT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_edit_coarse, dim3((edit_cell_count(edit_cells(box, 6)) + 63) / 64), dim3(64), 0, st, box, 6, (const unsigned long long*)l1, l2, G);
    VRT_LAUNCH_CHECK();
    if (G == 256) hipLaunchKernelGGL(k_edit_coarse, dim3(1), dim3(64), 0, st, box, 8, (const unsigned long long*)l2, l3, G);
    else hipLaunchKernelGGL(k_build_l0c, dim3(1), dim3(512), 0, st, (const unsigned long long*)l0, (const unsigned long long*)l1, l0c, l0c_base);
    VRT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cull_box, dim3(1), dim3(256), 0, st, (const unsigned long long*)l0, G / 4, cull);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}

// Kernel variants are picked by four switches; these macros spell the dispatch once.
#define VRT_BY_GRID(G_, CALL) do { if ((G_) == 256) { constexpr int G = 256; CALL; } else { constexpr int G = 128; CALL; } } while (0)
#define VRT_BY_2(A_, B_, CALL) do { if (A_) { constexpr bool A = true; if (B_) { constexpr bool B = true; CALL; } else { constexpr bool B = false; CALL; } } \
                                    else { constexpr bool A = false; if (B_) { constexpr bool B = true; CALL; } else { constexpr bool B = false; CALL; } } } while (0)

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
hipError_t launch_detmath_probe(hipStream_t st, int op, int n, const float* a, const float* b, float* out) {
    hipLaunchKernelGGL(k_detmath_probe, dim3((n + 255) / 256), dim3(256), 0, st, op, n, a, b, out);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
hipError_t launch_shade_probe(hipStream_t st, const FrameParams& fp, const SceneData& sc, const float* mats_x, int op, int n, const float* in, int in_stride,
                              float* out, int out_stride, float* lane_tables) {
    if (op == SHADE_SHIFT && !lane_tables) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_shade_probe, dim3((n + 63) / 64), dim3(64), 0, st, fp, sc, mats_x, op, n, in, in_stride, out, out_stride, lane_tables);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
hipError_t launch_trace_probe(hipStream_t st, int grid_res, int walk, const Pyramid& pyr, const float* cull, int n, const float* rays, ProbeOut* out) {
    const dim3 g((n + 63) / 64), b(64);
    if (walk == PROBE_WALK_BRANCHY) VRT_BY_GRID(grid_res, hipLaunchKernelGGL((k_trace_probe<G, PROBE_WALK_BRANCHY>), g, b, 0, st, pyr, cull, n, rays, out));
    else if (walk == PROBE_WALK_FLAT) VRT_BY_GRID(grid_res, hipLaunchKernelGGL((k_trace_probe<G, PROBE_WALK_FLAT>), g, b, 0, st, pyr, cull, n, rays, out));
    else if (walk == PROBE_WALK_RECORD) VRT_BY_GRID(grid_res, hipLaunchKernelGGL((k_trace_probe<G, PROBE_WALK_RECORD>), g, b, 0, st, pyr, cull, n, rays, out));
    else return hipErrorInvalidValue;
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}

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
hipError_t launch_fetch_voxels(hipStream_t st, int grid_res, const EditBox& box, const int8_t* mat, const uint8_t* rgb, int8_t* box_mat, uint8_t* box_rgb) {
    hipLaunchKernelGGL(k_fetch_voxels, dim3((edit_box_voxels(box) + 255) / 256), dim3(256), 0, st, box, grid_res, mat, rgb, box_mat, box_rgb);
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

// ---- vrt_voxelize_triangles: caller-supplied triangles voxelised into a box (vrt_voxelize.h holds the arithmetic) -----------------------
// Three kernels around an ownership buffer of one word per voxel of the clip box; launch_edit then does what it does for any box.
//   k_vox_setup    a LANE a triangle: the gate, the snap, the 16^3 cells its clipped bounds touch = its work items.  A wave sums its
//                  lanes' counts with a shuffle scan and takes entries and item numbers for all of them with ONE 64-bit atomic
//                  (entries << 40 | items), so entries come out ordered by their first item; lane 0 also counts the invalid ones.
//   k_vox_raster   a WAVE an item.  Waves reserve VRT_VOX_ITEMS_PER_GRAB consecutive items from a work head until it is exhausted, find
//                  the first one's triangle by binary search and walk on from there; the set-up (thirteen axes) is redone only when
//                  the triangle changes.  An item: the 16^3 cell is tested whole (wave-uniform), its 64 bricks by the 64 lanes, one
//                  each, and for every brick of the ballot the 64 lanes test its 64 voxels, one each; a covered voxel's word is
//                  raised to the triangle's global number + 1 with atomicMax, which is what makes the outcome independent of any of
//                  this.  A triangle spanning the grid is 4096 items in 1024 grabs: no wave walks it alone.
//   k_vox_resolve  a lane a few voxels of the box, z fastest like k_edit_store: the owner's payload, or the grid's stored voxel, into the
//                  box arrays; the last batch's also counts the written voxels and bounds them, reduced over the workgroup first.
// Plain C++ and vector memory operations throughout; the indices a wave branches on are made wave-uniform with readfirstlane so
// that triangle and entry loads are scalar loads.
#define VRT_VOX_ITEM_MASK ((1ULL << 40) - 1ULL)
__global__ __launch_bounds__(256) void k_vox_begin(VoxResult* res) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        for (int a = 0; a < 3; a++) { res->lo[a] = 0x7fffffff; res->hi[a] = (int32_t)0x80000000; }
        res->voxels = 0ULL; res->invalid = 0ULL;
    }
}
// The set-up pass of both triangle edits: tri_items is the call's item count of one triangle (vox_tri_items, fill_tri_items).
template <uint32_t (*tri_items)(const vrt_triangle&, int, const EditBox&, bool&)>
static __device__ __forceinline__ void tri_setup(int G, const EditBox& clip, long long m, const vrt_triangle* __restrict__ tris,
                                                 unsigned long long* __restrict__ heads, VoxEntry* __restrict__ entries, VoxResult* __restrict__ res) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool valid = true;
    uint32_t items = 0u;
    if (i < m) items = tri_items(tris[i], G, clip, valid);
    const unsigned long long has = __ballot(items != 0u), bad = __ballot(!valid);
    unsigned long long incl = items;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    const unsigned long long total = __shfl(incl, 63, 64);
    unsigned long long old = 0ULL;
    if (lane == 0) {
        if (has) old = atomicAdd(&heads[0], ((unsigned long long)__popcll(has) << 40) + total);
        if (bad) atomicAdd(&res->invalid, (unsigned long long)__popcll(bad));
    }
    old = __shfl(old, 0, 64);
    if (items != 0u) {   // (slot < m: a batch has no more entries than triangles)
        VoxEntry e;
        e.first = (old & VRT_VOX_ITEM_MASK) + incl - items;
        e.tri = (uint32_t)i;
        e.items = items;
        entries[(old >> 40) + (unsigned long long)__popcll(has & ((1ULL << lane) - 1ULL))] = e;
    }
}
__global__ __launch_bounds__(256) void k_vox_setup(int G, EditBox clip, long long m, const vrt_triangle* __restrict__ tris, unsigned long long* __restrict__ heads,
                                                   VoxEntry* __restrict__ entries, VoxResult* __restrict__ res) {
    tri_setup<vox_tri_items>(G, clip, m, tris, heads, entries, res);
}
__global__ __launch_bounds__(256) void k_vox_raster(int G, EditBox clip, unsigned long long base, const vrt_triangle* __restrict__ tris,
                                                    unsigned long long* __restrict__ heads, const VoxEntry* __restrict__ entries, uint32_t* __restrict__ owner) {
    const int lane = threadIdx.x & 63;
    const unsigned long long h = heads[0], total = h & VRT_VOX_ITEM_MASK;
    const long long n_entries = (long long)(h >> 40);
    for (;;) {
        unsigned long long g = 0ULL;
        if (lane == 0) g = atomicAdd(&heads[1], (unsigned long long)VRT_VOX_ITEMS_PER_GRAB);
        g = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(g >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)g);
        if (g >= total) return;
        const unsigned long long g1 = g + VRT_VOX_ITEMS_PER_GRAB < total ? g + VRT_VOX_ITEMS_PER_GRAB : total;
        long long e = vox_find_entry(entries, n_entries, g);
        while (g < g1 && e < n_entries) {   // (e < n_entries always: every item below `total` belongs to an entry)
            const VoxEntry en = entries[e++];
            VoxTri s;
            vox_setup(tris[en.tri], G, s);
            const EditCells cells = vox_cells(s, clip, 4), bricks = vox_cells(s, clip, 2);
            const uint32_t mine = (uint32_t)(base + en.tri + 1ULL);
            const unsigned long long end = en.first + en.items < g1 ? en.first + en.items : g1;
            for (; g < end; g++) {
                int cx, cy, cz;
                edit_cell(cells, (int)(g - en.first), cx, cy, cz);
                if (!vox_cube(s, cx, cy, cz, 4)) continue;
                unsigned long long todo = __ballot(vox_lane_brick(s, bricks, cx, cy, cz, lane));
                while (todo) {
                    const int brick = __ffsll((long long)todo) - 1;
                    todo &= todo - 1ULL;
                    const int at = vox_lane_voxel(s, clip, cx, cy, cz, brick, lane);   // (-1, or inside the box: vox_in_box)
                    if (at >= 0) atomicMax(&owner[at], mine);
                }
            }
        }
    }
}
// VRT_VOX_RESOLVE_PER_THREAD voxels a thread, a workgroup's 256 x that many consecutive voxels taken 256 apart so that a wave's loads and
// stores stay neighbours.  Count and bounds are summed per thread, then by tri_tally -- which both resolves end on -- over the wave with
// shuffles, then over the workgroup's four waves through LDS, and one thread a workgroup issues the atomics -- the bounds' only where they
// would move the record (a plain load first): one atomic per wave on seven words that every wave shares made the written voxels, not the
// box, set this kernel's time.  Every thread of the workgroup calls tri_tally (a barrier inside); `final`, the same for all of them: the
// surface pass's resolves before the last tally nothing (tested in here, where it leaves k_vox_resolve's machine code what it was).
#define VRT_VOX_RESOLVE_PER_THREAD 8
static __device__ __forceinline__ void tri_tally(bool final, int count, int lo[3], int hi[3], VoxResult* res) {
    __shared__ int part[4][7];
    if (!final) return;
    for (int d = 32; d >= 1; d >>= 1) {
        count += __shfl_xor(count, d, 64);
        for (int a = 0; a < 3; a++) {
            const int l = __shfl_xor(lo[a], d, 64), u = __shfl_xor(hi[a], d, 64);
            lo[a] = l < lo[a] ? l : lo[a];
            hi[a] = u > hi[a] ? u : hi[a];
        }
    }
    if ((threadIdx.x & 63) == 0) {
        int* p = part[threadIdx.x >> 6];
        p[0] = count;
        for (int a = 0; a < 3; a++) { p[1 + a] = lo[a]; p[4 + a] = hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) {
            count += part[w][0];
            for (int a = 0; a < 3; a++) { lo[a] = part[w][1 + a] < lo[a] ? part[w][1 + a] : lo[a]; hi[a] = part[w][4 + a] > hi[a] ? part[w][4 + a] : hi[a]; }
        }
        if (count) {
            atomicAdd(&res->voxels, (unsigned long long)count);
            for (int a = 0; a < 3; a++) {   // (a stale load only costs an atomic that changes nothing)
                if (lo[a] < *(volatile int32_t*)&res->lo[a]) atomicMin(&res->lo[a], lo[a]);
                if (hi[a] > *(volatile int32_t*)&res->hi[a]) atomicMax(&res->hi[a], hi[a]);
            }
        }
    }
}
__global__ __launch_bounds__(256) void k_vox_resolve(int G, EditBox clip, const uint32_t* __restrict__ owner, unsigned long long base,
                                                     const vrt_triangle* __restrict__ tris, int final, const int8_t* __restrict__ mat,
                                                     const uint8_t* __restrict__ rgb, int8_t* __restrict__ box_mat, uint8_t* __restrict__ box_rgb,
                                                     VoxResult* res) {
    const int nv = edit_box_voxels(clip), first = blockIdx.x * (256 * VRT_VOX_RESOLVE_PER_THREAD) + threadIdx.x;
    int count = 0, lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {(int32_t)0x80000000, (int32_t)0x80000000, (int32_t)0x80000000};
    for (int k = 0; k < VRT_VOX_RESOLVE_PER_THREAD; k++) {
        const int i = first + k * 256;
        if (i < nv && vox_resolve_voxel(clip, G, i, owner, base, tris, final != 0, mat, rgb, box_mat, box_rgb) && final) {
            int c[3];
            edit_box_voxel(clip, i, c[0], c[1], c[2]);
            count++;
            for (int a = 0; a < 3; a++) { lo[a] = c[a] < lo[a] ? c[a] : lo[a]; hi[a] = c[a] > hi[a] ? c[a] : hi[a]; }
        }
    }
    tri_tally(final != 0, count, lo, hi, res);
}

hipError_t launch_tri_begin(hipStream_t st, size_t head_bytes, const TriScratch& s) {
    hipError_t e = hipMemsetAsync(s.words, 0, head_bytes, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_vox_begin, dim3(1), dim3(64), 0, st, s.res);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
// What a batch of either call begins with: the two heads zeroed and the call's set-up kernel over the batch's m triangles.
template <class Setup>
static hipError_t launch_tri_setup(hipStream_t st, Setup k_setup, int grid_res, const EditBox& clip, long long m, const vrt_triangle* tris, const TriScratch& s) {
    hipError_t e = hipMemsetAsync(s.heads, 0, 16, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_setup, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, grid_res, clip, m, tris, s.heads, s.entries, s.res);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
hipError_t launch_voxelize_batch(hipStream_t st, int grid_res, int n_cu, const EditBox& clip, unsigned long long base, long long m, const vrt_triangle* tris,
                                 const TriScratch& s) {
    hipError_t e = launch_tri_setup(st, k_vox_setup, grid_res, clip, m, tris, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_vox_raster, dim3(plan_voxelize_blocks(n_cu)), dim3(256), 0, st, grid_res, clip, base, tris, s.heads, (const VoxEntry*)s.entries, s.words);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
hipError_t launch_voxelize_resolve(hipStream_t st, int grid_res, const EditBox& clip, unsigned long long base, const vrt_triangle* tris, bool final,
                                   const int8_t* mat, const uint8_t* rgb, const TriScratch& s) {
    hipLaunchKernelGGL(k_vox_resolve, dim3((edit_box_voxels(clip) + 256 * VRT_VOX_RESOLVE_PER_THREAD - 1) / (256 * VRT_VOX_RESOLVE_PER_THREAD)), dim3(256), 0, st, grid_res, clip, (const uint32_t*)s.words, base, tris,
                       final ? 1 : 0, mat, rgb, s.box_mat, s.box_rgb, s.res);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}

// ---- vrt_fill_triangles: the inside of a closed mesh filled with voxels (vrt_fill.h holds the arithmetic) ---------------------------------
// Three kernels around a toggle bitmap of one bit per voxel of the clip box, bits along z; launch_edit then does what it does for any box.
//   k_fill_setup    k_vox_setup's body (tri_setup) over this call's item count: a LANE a triangle, the gate, the snap, sign(n_z), the
//                   aligned tiles of 16 x 16 columns its clipped xy bounds touch = its work items; entries and item numbers for a
//                   wave's 64 triangles with ONE 64-bit atomic, in the same layout (VoxEntry, entries << 40 | items).
//   k_fill_raster   a WAVE an item, VRT_FILL_ITEMS_PER_GRAB consecutive items a grab from the work head, the triangle found by binary
//                   search and its set-up redone only when it changes, as in k_vox_raster.  An item: each lane tests four columns of
//                   the tile (three edge functions, the bracket in int32) and, for a column the triangle owns, finds the first cell
//                   above the triangle with one 64-bit division and flips that cell's bit with ONE atomicXor -- a triangle costs an
//                   atomic per column, not per covered voxel.  XOR commutes, so nothing here depends on order: batches and the host
//                   path's chunks toggle into the same bitmap and no resolve runs between them.
//   k_fill_resolve  a lane a few voxels of the box, z fastest: the prefix-XOR of the column's words up to the voxel's own says inside;
//                   the payload or the grid's stored voxel into the box arrays; count and tight box reduced over the workgroup first.
// Plain C++ and vector memory operations throughout; the item number is made wave-uniform with readfirstlane as in k_vox_raster.
__global__ __launch_bounds__(256) void k_fill_setup(int G, EditBox clip, long long m, const vrt_triangle* __restrict__ tris, unsigned long long* __restrict__ heads,
                                                    VoxEntry* __restrict__ entries, VoxResult* __restrict__ res) {
    tri_setup<fill_tri_items>(G, clip, m, tris, heads, entries, res);
}
__global__ __launch_bounds__(256) void k_fill_raster(int G, EditBox clip, const vrt_triangle* __restrict__ tris, unsigned long long* __restrict__ heads,
                                                     const VoxEntry* __restrict__ entries, uint32_t* __restrict__ toggles) {
    const int lane = threadIdx.x & 63;
    const unsigned long long h = heads[0], total = h & VRT_VOX_ITEM_MASK;
    const long long n_entries = (long long)(h >> 40);
    for (;;) {
        unsigned long long g = 0ULL;
        if (lane == 0) g = atomicAdd(&heads[1], (unsigned long long)VRT_FILL_ITEMS_PER_GRAB);
        g = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(g >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)g);
        if (g >= total) return;
        const unsigned long long g1 = g + VRT_FILL_ITEMS_PER_GRAB < total ? g + VRT_FILL_ITEMS_PER_GRAB : total;
        long long e = vox_find_entry(entries, n_entries, g);
        while (g < g1 && e < n_entries) {   // (e < n_entries always: every item below `total` belongs to an entry)
            const VoxEntry en = entries[e++];
            FillTri s;
            fill_setup(tris[en.tri], G, s);
            const EditCells cells = fill_cells(s, clip), tiles = fill_tiles(cells);
            const unsigned long long end = en.first + en.items < g1 ? en.first + en.items : g1;
            for (; g < end; g++) {
                int tx, ty, tz;
                edit_cell(tiles, (int)(g - en.first), tx, ty, tz);
                for (int k = 0; k < 4; k++) {
                    int cx, cy;
                    if (!fill_lane_column(s, cells, tx, ty, lane, k, cx, cy)) continue;
                    uint32_t bit;
                    const int at = fill_toggle_at(clip, cx, cy, fill_first_cell(s, cx, cy), bit);   // (-1, or below fill_words(clip): the column is in the box)
                    if (at >= 0) atomicXor(&toggles[at], bit);
                }
            }
        }
    }
}
// k_vox_resolve's shape: VRT_VOX_RESOLVE_PER_THREAD voxels a thread taken 256 apart, count and bounds summed per thread, then tri_tally.
__global__ __launch_bounds__(256) void k_fill_resolve(int G, EditBox clip, const uint32_t* __restrict__ toggles, uint32_t voxel, const int8_t* __restrict__ mat,
                                                      const uint8_t* __restrict__ rgb, int8_t* __restrict__ box_mat, uint8_t* __restrict__ box_rgb, VoxResult* res) {
    const int nv = edit_box_voxels(clip), first = blockIdx.x * (256 * VRT_VOX_RESOLVE_PER_THREAD) + threadIdx.x;
    int count = 0, lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {(int32_t)0x80000000, (int32_t)0x80000000, (int32_t)0x80000000};
    for (int k = 0; k < VRT_VOX_RESOLVE_PER_THREAD; k++) {
        const int i = first + k * 256;
        if (i < nv && fill_resolve_voxel(clip, G, i, toggles, voxel, mat, rgb, box_mat, box_rgb)) {
            int c[3];
            edit_box_voxel(clip, i, c[0], c[1], c[2]);
            count++;
            for (int a = 0; a < 3; a++) { lo[a] = c[a] < lo[a] ? c[a] : lo[a]; hi[a] = c[a] > hi[a] ? c[a] : hi[a]; }
        }
    }
    tri_tally(true, count, lo, hi, res);
}

hipError_t launch_fill_batch(hipStream_t st, int grid_res, int n_cu, const EditBox& clip, long long m, const vrt_triangle* tris, const TriScratch& s) {
    hipError_t e = launch_tri_setup(st, k_fill_setup, grid_res, clip, m, tris, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fill_raster, dim3(plan_voxelize_blocks(n_cu)), dim3(256), 0, st, grid_res, clip, tris, s.heads, (const VoxEntry*)s.entries, s.words);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
hipError_t launch_fill_resolve(hipStream_t st, int grid_res, const EditBox& clip, uint32_t voxel, const int8_t* mat, const uint8_t* rgb, const TriScratch& s) {
    hipLaunchKernelGGL(k_fill_resolve, dim3((edit_box_voxels(clip) + 256 * VRT_VOX_RESOLVE_PER_THREAD - 1) / (256 * VRT_VOX_RESOLVE_PER_THREAD)), dim3(256), 0, st, grid_res, clip,
                       (const uint32_t*)s.words, voxel, mat, rgb, s.box_mat, s.box_rgb, s.res);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}

// ---- vrt_distance_field: three separable line passes through LDS (vrt_distance.h holds the arithmetic, vrt_plan.h the tile shapes) ----------
// Memory is z-fastest everywhere, so every pass puts adjacent lanes on adjacent z (pass x: on adjacent cells of the (y, z) plane, which
// is contiguous) and every global access is a coalesced segment.  A line is staged once and read by every output element of it.
//   k_dist_z   VRT_DIST_Z_LINES consecutive lines (x, y) of the grown box a workgroup: their material bytes, read straight from d_mat,
//              become 0 (target) or cap in LDS, one line after the other; a thread works elements 256 apart, so a wave's lanes sit on
//              consecutive z of one line (or of neighbouring lines where the box is narrow) and read consecutive LDS words.
//   k_dist_y   a tile of VRT_DIST_LANES adjacent z at one x a workgroup, staged as [y][lane]: a lane walks its own line with stride
//              VRT_DIST_LANES words, so the 32 lanes of a group read 32 consecutive words -- no bank conflict inside a group.
//   k_dist_x   the same over adjacent cells of the (y, z) plane, lines along x; writes d2 (dist_final) and, with NEAR, assembles `nearest`.
// NEAR = false compiles the coordinates out: no cz / cy store, no load, and the scan stops one step earlier (dist_line_element).
// Lanes of a wave scan as long as their slowest neighbour; neighbours see nearly the same distances, so little is lost.
template <bool NEAR>
__global__ __launch_bounds__(256) void k_dist_z(DistBox p, int G, const int8_t* __restrict__ mat, int* __restrict__ A, uint8_t* __restrict__ cz) {
    __shared__ int f[VRT_DIST_Z_LINES * VRT_DIST_Z_PITCH];
    const int gyn = dist_len(p.grown, 1), gzn = dist_len(p.grown, 2), bzn = dist_len(p.box, 2);
    const int lines = dist_len(p.grown, 0) * gyn;
    const int L0 = blockIdx.x * VRT_DIST_Z_LINES;
    const int nl = min(VRT_DIST_Z_LINES, lines - L0);
    for (int idx = threadIdx.x; idx < nl * gzn; idx += 256) {
        const int l = idx / gzn, k = idx - l * gzn, L = L0 + l;
        const int x = p.grown.lo[0] + L / gyn, y = p.grown.lo[1] + L % gyn;
        f[l * VRT_DIST_Z_PITCH + k] = dist_seed(mat[edit_grid_index(G, x, y, p.grown.lo[2] + k)], p);
    }
    __syncthreads();
    const int off = p.box.lo[2] - p.grown.lo[2];
    for (int idx = threadIdx.x; idx < nl * bzn; idx += 256) {
        const int l = idx / bzn, zi = idx - l * bzn;
        const DistPick b = dist_line_element<NEAR>(f + l * VRT_DIST_Z_PITCH, 1, gzn, off + zi, p.grown.lo[2]);
        const size_t o = (size_t)L0 * bzn + idx;   // dist_a_index: lines are consecutive in A
        A[o] = b.v;
        if (NEAR) cz[o] = (uint8_t)b.c;
    }
}
template <bool NEAR>
__global__ __launch_bounds__(256) void k_dist_y(DistBox p, const int* __restrict__ A, int* __restrict__ B, uint8_t* __restrict__ cy) {
    extern __shared__ int f[];   // [gyn][VRT_DIST_LANES]
    const int lane = threadIdx.x % VRT_DIST_LANES, grp = threadIdx.x / VRT_DIST_LANES;
    const int gyn = dist_len(p.grown, 1), byn = dist_len(p.box, 1), bzn = dist_len(p.box, 2);
    const int xi = blockIdx.y, zi = blockIdx.x * VRT_DIST_LANES + lane;
    const bool ok = zi < bzn;
    for (int j = grp; j < gyn; j += VRT_DIST_GROUPS) f[j * VRT_DIST_LANES + lane] = ok ? A[dist_a_index(p, xi, j, zi)] : p.cap;
    __syncthreads();
    if (!ok) return;
    const int off = p.box.lo[1] - p.grown.lo[1];
    for (int yo = grp; yo < byn; yo += VRT_DIST_GROUPS) {
        const DistPick b = dist_line_element<NEAR>(f + lane, VRT_DIST_LANES, gyn, off + yo, p.grown.lo[1]);
        const size_t o = dist_b_index(p, xi, yo, zi);
        B[o] = b.v;
        if (NEAR) cy[o] = (uint8_t)b.c;
    }
}
template <bool NEAR>
__global__ __launch_bounds__(256) void k_dist_x(DistBox p, int G, const int* __restrict__ B, const uint8_t* __restrict__ cz, const uint8_t* __restrict__ cy,
                                                int* __restrict__ d2, int* __restrict__ nearest) {
    extern __shared__ int f[];   // [gxn][VRT_DIST_LANES]
    const int lane = threadIdx.x % VRT_DIST_LANES, grp = threadIdx.x / VRT_DIST_LANES;
    const int gxn = dist_len(p.grown, 0), bxn = dist_len(p.box, 0), bzn = dist_len(p.box, 2);
    const int plane = dist_len(p.box, 1) * bzn;
    const int pi = blockIdx.x * VRT_DIST_LANES + lane;
    const bool ok = pi < plane;
    for (int j = grp; j < gxn; j += VRT_DIST_GROUPS) f[j * VRT_DIST_LANES + lane] = ok ? B[(size_t)j * plane + pi] : p.cap;
    __syncthreads();
    if (!ok) return;
    const int off = p.box.lo[0] - p.grown.lo[0];
    const int yo = pi / bzn, zi = pi - yo * bzn;
    for (int xo = grp; xo < bxn; xo += VRT_DIST_GROUPS) {
        const DistPick b = dist_line_element<NEAR>(f + lane, VRT_DIST_LANES, gxn, off + xo, p.grown.lo[0]);
        const size_t o = (size_t)xo * plane + pi;
        const int v = dist_final(b.v, p.max_d2);
        d2[o] = v;
        if (NEAR) nearest[o] = v == VRT_DIST_FAR_VALUE ? -1 : dist_assemble(p, G, b.c, yo, zi, cy, cz);
    }
}
template <bool NEAR>
static hipError_t launch_distance_passes(hipStream_t st, int grid_res, const DistBox& p, const int8_t* mat, const DistScratch& s, int* d2, int* nearest) {
    const int gxn = dist_len(p.grown, 0), gyn = dist_len(p.grown, 1), byn = dist_len(p.box, 1), bzn = dist_len(p.box, 2);
    hipLaunchKernelGGL(k_dist_z<NEAR>, dim3((gxn * gyn + VRT_DIST_Z_LINES - 1) / VRT_DIST_Z_LINES), dim3(256), 0, st, p, grid_res, mat, s.a, s.cz);
    VRT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_dist_y<NEAR>, dim3((bzn + VRT_DIST_LANES - 1) / VRT_DIST_LANES, gxn), dim3(256), (size_t)gyn * VRT_DIST_LANES * sizeof(int), st, p,
                       (const int*)s.a, s.b, s.cy);
    VRT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_dist_x<NEAR>, dim3((byn * bzn + VRT_DIST_LANES - 1) / VRT_DIST_LANES), dim3(256), (size_t)gxn * VRT_DIST_LANES * sizeof(int), st, p,
                       grid_res, (const int*)s.b, (const uint8_t*)s.cz, (const uint8_t*)s.cy, d2, nearest);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
hipError_t launch_distance_field(hipStream_t st, int grid_res, const DistBox& p, const int8_t* mat, const DistScratch& s, int* d2, int* nearest) {
    if (edit_box_voxels(p.box) == 0 || grid_res > VRT_DIST_LINE) return hipErrorInvalidValue;
    return nearest ? launch_distance_passes<true>(st, grid_res, p, mat, s, d2, nearest) : launch_distance_passes<false>(st, grid_res, p, mat, s, d2, nullptr);
}

// ---- vrt_label_components: a union-find in the output array (vrt_label.h holds the arithmetic and the proof, vrt_plan.h the tile shape) --------
// Three launches; the kernel boundary is the only barrier between workgroups, and no thread ever waits for another: every loop is
// label_find's or label_union's, bounded by vrt_label.h's first sentence.
//   k_label_tile    a workgroup a tile: material bytes straight from d_mat (a wave's lanes on 64 consecutive z: one segment), members
//                   seeded with their tile-local name in LDS, united with their forward neighbours inside the tile by LDS atomics, and
//                   every cell's word stored -- the grid index of its tile root, or VRT_LABEL_NONE.
//   k_label_seams   a workgroup a tile again: a thread a slot on a tile face, united with the forward neighbours that lie in another tile.
//                   The label array is touched through agent-scope relaxed atomic loads and atomic min only (LabelWords): a plain load
//                   could be served by an L1 or by another XCD's L2 that nobody refreshes.  Even so nothing here NEEDS a fresh
//                   value -- a stale one is an earlier parent, and vrt_label.h's second sentence covers it.
//   k_label_finish  a thread a cell: walks to its root and stores it in place (one more parent to whoever still reads the word);
//                   members and roots counted by ballot per wave, summed over the workgroup's four waves in LDS, one atomic per
//                   counter word and workgroup.
struct LabelLds {   // names: tile-local slots
    int* s;
    VRT_DEV int load(int i) const { return __hip_atomic_load(s + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    VRT_DEV int atomic_min(int i, int v) const { return __hip_atomic_fetch_min(s + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};
struct LabelWords {   // names: grid indices; the words sit box-locally
    int* L;
    const LabelBox& p;
    VRT_DEV int load(int g) const { return __hip_atomic_load(L + label_box_of_grid(p, g), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    VRT_DEV int atomic_min(int g, int v) const { return __hip_atomic_fetch_min(L + label_box_of_grid(p, g), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    VRT_DEV void store(int g, int v) const { __hip_atomic_store(L + label_box_of_grid(p, g), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
__global__ __launch_bounds__(256) void k_label_tile(LabelBox p, const int8_t* __restrict__ mat, int* __restrict__ L) {
    __shared__ int s[VRT_LABEL_TILE];
    const LabelTile r = label_tile(p, blockIdx.x);
    LabelLds m{s};
    for (int t = threadIdx.x; t < VRT_LABEL_TILE; t += 256) s[t] = label_tile_seed(p, r, mat, t);
    __syncthreads();
    for (int t = threadIdx.x; t < VRT_LABEL_TILE; t += 256) {
        if (m.load(t) < 0) continue;
        for (int k = 0; k < p.forward; k++) label_tile_link(m, r, t, k);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < VRT_LABEL_TILE; t += 256) {
        int lx, ly, lz;
        label_tile_cell(t, lx, ly, lz);
        if (label_in_tile(r, lx, ly, lz)) L[label_box_index(p, r.o[0] + lx, r.o[1] + ly, r.o[2] + lz)] = label_tile_result(m, p, r, t);
    }
}
__global__ __launch_bounds__(256) void k_label_seams(LabelBox p, int* L) {
    const LabelTile r = label_tile(p, blockIdx.x);
    LabelWords m{L, p};
    for (int t = threadIdx.x; t < VRT_LABEL_TILE; t += 256) {
        int lx, ly, lz;
        label_tile_cell(t, lx, ly, lz);
        if (!label_in_tile(r, lx, ly, lz) || !label_on_seam(p, r, lx, ly, lz)) continue;
        if (m.load(label_grid_index(p, r.o[0] + lx, r.o[1] + ly, r.o[2] + lz)) < 0) continue;
        for (int k = 0; k < p.forward; k++) label_seam_link(m, p, r, t, k);
    }
}
__global__ __launch_bounds__(256) void k_label_finish(LabelBox p, int* L, vrt_label_result* counters) {
    __shared__ int part[4][2];
    const int nv = p.n[0] * p.n[1] * p.n[2], i = blockIdx.x * 256 + threadIdx.x;
    LabelWords m{L, p};
    bool member = false, root = false;
    if (i < nv) label_finish_cell(m, p, i / (p.n[2] * p.n[1]), i / p.n[2] % p.n[1], i % p.n[2], member, root);
    const int members = __popcll(__ballot(member)), roots = __popcll(__ballot(root));
    if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6][0] = members; part[threadIdx.x >> 6][1] = roots; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int cells = part[0][0] + part[1][0] + part[2][0] + part[3][0], comps = part[0][1] + part[1][1] + part[2][1] + part[3][1];
        if (cells) atomicAdd((unsigned long long*)&counters->cells, (unsigned long long)cells);
        if (comps) atomicAdd(&counters->components, comps);
    }
}
hipError_t launch_label_components(hipStream_t st, const LabelBox& p, const int8_t* mat, int* labels, vrt_label_result* counters) {
    const int nv = edit_box_voxels(p.box);
    if (nv == 0) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(counters, 0, sizeof(vrt_label_result), st);
    if (e != hipSuccess) return e;
    const int tiles = label_tile_count(p);
    hipLaunchKernelGGL(k_label_tile, dim3(tiles), dim3(256), 0, st, p, mat, labels);
    VRT_LAUNCH_CHECK();
    if (tiles > 1) {   // (a lone tile has no seam)
        hipLaunchKernelGGL(k_label_seams, dim3(tiles), dim3(256), 0, st, p, labels);
        VRT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_label_finish, dim3((nv + 255) / 256), dim3(256), 0, st, p, labels, counters);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}

// ---- vrt_move_voxels: voxels of a box moved or copied under an integer affine map (vrt_move.h holds the arithmetic and the passes' order) ----
//   k_move_snapshot  a thread a cell of the source box, z fastest: the cell's word (move_snap_cell) stored; the piece cells the call
//                    vacates counted into `erased`.
//   k_move_dst       a workgroup a tile of VRT_MOVE_TX x TY x TZ cells of the destination box, a thread a run of VRT_MOVE_RUN cells along z: the
//                    map once, then the z step.  A tile's source cells are a slab a few cells thick whatever the map turns it to, one
//                    4-byte word a cell.  <false> is the count pass, <true> writes the destination box's arrays, a wave's lanes on 64
//                    consecutive z of one line; it reads the count pass's `blocked` for VRT_MOVE_IF_FREE.
//   k_move_src       a thread a cell of the source box: the source box's arrays.
// The record: the two counting kernels run at most VRT_MOVE_COUNT_BLOCKS workgroups, each striding over cells or tiles with its tallies in
// registers; at the end a wave folds them by shuffles, the workgroup's four waves meet in LDS and ONE thread adds to the record's words.
// (One atomic a wave and tile was measured first: on a half-full 128^3 grid the 260 000 atomics on the record's one cache line were
// 0.7 of the count pass's 0.8 ms.)  Plain C++ and vector memory operations throughout.
#define VRT_MOVE_COUNT_BLOCKS 2048
__global__ __launch_bounds__(64) void k_move_begin(MoveRecord* rec) {
    if (threadIdx.x == 0 && blockIdx.x == 0) move_record_begin(*rec);
}
static __device__ __forceinline__ void move_tally_fold(MoveTally& t) {   // over the wave; every lane ends with the wave's
    for (int d = 32; d > 0; d >>= 1) {
        t.written += __shfl_xor(t.written, d, 64);
        t.blocked += __shfl_xor(t.blocked, d, 64);
        for (int a = 0; a < 3; a++) { t.lo[a] = min(t.lo[a], __shfl_xor(t.lo[a], d, 64)); t.hi[a] = max(t.hi[a], __shfl_xor(t.hi[a], d, 64)); }
    }
}
__global__ __launch_bounds__(256) void k_move_snapshot(MovePlan p, int n, const int8_t* __restrict__ mat, const uint8_t* __restrict__ rgb, const int* __restrict__ select,
                                                       uint32_t* __restrict__ snap, MoveRecord* rec) {
    __shared__ unsigned part[4];
    unsigned pieces = 0u;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {   // (n <= 2^24, the stride <= 2^19: no overflow)
        const uint32_t w = move_snap_cell(p, i, mat, rgb, select);
        snap[i] = w;
        pieces += move_vacated(p.flags, w) ? 1u : 0u;
    }
    for (int d = 32; d > 0; d >>= 1) pieces += __shfl_xor(pieces, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = pieces;
    __syncthreads();
    if (threadIdx.x == 0 && part[0] + part[1] + part[2] + part[3]) atomicAdd(&rec->erased, (unsigned long long)(part[0] + part[1] + part[2] + part[3]));
}
template <bool BUILD>
__global__ __launch_bounds__(256) void k_move_dst(MovePlan p, int tiles, const int8_t* __restrict__ mat, const uint8_t* __restrict__ rgb, const uint32_t* __restrict__ snap,
                                                  int8_t* __restrict__ box_mat, uint8_t* __restrict__ box_rgb, MoveRecord* rec) {
    __shared__ MoveTally part[4];
    MoveTally t = move_tally_none();
    const bool go = BUILD ? move_go(p.flags, rec->blocked) : true;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        int x, y, z;
        const int n = move_tile_run(p, tile, threadIdx.x, x, y, z);
        if (n > 0) move_dst_run<BUILD>(p, go, x, y, z, n, mat, rgb, snap, box_mat, box_rgb, t);
    }
    if (!BUILD) {
        move_tally_fold(t);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = t;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < 4; w++) {
                t.written += part[w].written; t.blocked += part[w].blocked;
                for (int a = 0; a < 3; a++) { t.lo[a] = min(t.lo[a], part[w].lo[a]); t.hi[a] = max(t.hi[a], part[w].hi[a]); }
            }
            if (t.blocked) atomicAdd(&rec->blocked, (unsigned long long)t.blocked);
            if (t.written) {
                atomicAdd(&rec->written, (unsigned long long)t.written);
                for (int a = 0; a < 3; a++) { atomicMin(&rec->lo[a], t.lo[a]); atomicMax(&rec->hi[a], t.hi[a]); }
            }
        }
    }
}
__global__ __launch_bounds__(256) void k_move_src(MovePlan p, int n, const int8_t* __restrict__ mat, const uint8_t* __restrict__ rgb, const uint32_t* __restrict__ snap,
                                                  int8_t* __restrict__ box_mat, uint8_t* __restrict__ box_rgb, const MoveRecord* rec) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) move_src_build(p, move_go(p.flags, rec->blocked), i, mat, rgb, snap, box_mat, box_rgb);
}
hipError_t launch_move_count(hipStream_t st, const MovePlan& p, const int8_t* mat, const uint8_t* rgb, const int* select, uint32_t* snap, MoveRecord* rec) {
    const int n_src = edit_box_voxels(p.src);
    if (n_src == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_move_begin, dim3(1), dim3(64), 0, st, rec);
    VRT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_move_snapshot, dim3(std::min((n_src + 255) / 256, VRT_MOVE_COUNT_BLOCKS)), dim3(256), 0, st, p, n_src, mat, rgb, select, snap, rec);
    VRT_LAUNCH_CHECK();
    if (edit_box_voxels(p.dst) != 0) {
        const int tiles = move_tile_count(p);
        hipLaunchKernelGGL(k_move_dst<false>, dim3(std::min(tiles, VRT_MOVE_COUNT_BLOCKS)), dim3(256), 0, st, p, tiles, mat, rgb, (const uint32_t*)snap, (int8_t*)nullptr,
                           (uint8_t*)nullptr, rec);
        VRT_LAUNCH_CHECK();
    }
    return hipSuccess;
}
hipError_t launch_move_src_arrays(hipStream_t st, const MovePlan& p, const int8_t* mat, const uint8_t* rgb, const uint32_t* snap, int8_t* box_mat, uint8_t* box_rgb,
                                  const MoveRecord* rec) {
    const int n_src = edit_box_voxels(p.src);
    if (n_src == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_move_src, dim3((n_src + 255) / 256), dim3(256), 0, st, p, n_src, mat, rgb, snap, box_mat, box_rgb, rec);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
hipError_t launch_move_dst_arrays(hipStream_t st, const MovePlan& p, const int8_t* mat, const uint8_t* rgb, const uint32_t* snap, int8_t* box_mat, uint8_t* box_rgb,
                                  MoveRecord* rec) {
    if (edit_box_voxels(p.dst) == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_move_dst<true>, dim3(move_tile_count(p)), dim3(256), 0, st, p, move_tile_count(p), mat, rgb, snap, box_mat, box_rgb, rec);
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
