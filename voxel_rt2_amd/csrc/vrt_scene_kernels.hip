// vrt_scene_kernels.hip -- gfx950 kernels of libvrt_hip.so that build or edit a scene, each with its launcher.
//
//   k_pack_grid / k_build_l0 / k_build_coarse / k_build_l0c   prepare_data: packed voxel texels, the bit-brick
//                                                         occupancy pyramid and its compacted fine level
//   k_cull_box                                            the culling box of the solids (cull_ray, vrt_trace.h)
//   k_edit_store / k_edit_fine / k_edit_coarse            vrt_update_voxels: the same data for a box of voxels (vrt_edit.h)
//   k_fetch_voxels                                        vrt_fetch_voxels: the stored voxels of a box
//   k_vox_begin / k_vox_setup / k_vox_raster / k_vox_resolve   vrt_voxelize_triangles (vrt_voxelize.h): ownership words, a wave an item
//   k_fill_setup / k_fill_raster / k_fill_resolve         vrt_fill_triangles (vrt_fill.h): one toggle bit per voxel, a wave an item
//   k_dist_z / k_dist_y / k_dist_x                        vrt_distance_field: the three line passes of the exact distance transform
//   k_label_tile / k_label_seams / k_label_finish         vrt_label_components (vrt_label.h): a union-find in the output array
//   k_move_begin / k_move_snapshot / k_move_dst / k_move_src   vrt_move_voxels (vrt_move.h): snapshot, count pass, the two boxes' arrays
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "vrt_kernels.h"

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

// vrt_fetch_voxels: one thread per voxel of the box, z fastest (k_edit_store the other way round)
__global__ void k_fetch_voxels(EditBox box, int G, const int8_t* __restrict__ mat, const uint8_t* __restrict__ rgb, int8_t* __restrict__ box_mat,
                               uint8_t* __restrict__ box_rgb) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < edit_box_voxels(box)) fetch_box_voxel(box, G, i, mat, rgb, box_mat, box_rgb);
}

// ---- host-side launchers of the above (each section below has its own beside its kernels) --------
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

hipError_t launch_fetch_voxels(hipStream_t st, int grid_res, const EditBox& box, const int8_t* mat, const uint8_t* rgb, int8_t* box_mat, uint8_t* box_rgb) {
    hipLaunchKernelGGL(k_fetch_voxels, dim3((edit_box_voxels(box) + 255) / 256), dim3(256), 0, st, box, grid_res, mat, rgb, box_mat, box_rgb);
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

}  // namespace vrt
