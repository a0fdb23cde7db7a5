// vrt_kernels.h -- launcher declarations of vrt_kernels.hip, vrt_scene_kernels.hip, vrt_query_kernels.hip, vrt_probe_kernels.hip and vrt_sky_kernels.hip, for them and the host units.
#ifndef VRT_KERNELS_H
#define VRT_KERNELS_H

#include <hip/hip_runtime.h>
#include "vrt_types.h"
#include "vrt_trace.h"
#include "vrt_bsdf.h"
#include "vrt_sky.h"
#include "vrt_path.h"
#include "vrt_pool.h"
#include "vrt_primary.h"
#include "vrt_restir.h"
#include "vrt_temporal.h"
#include "vrt_plan.h"
#include "vrt_edit.h"
#include "vrt_cast.h"
#include "vrt_sweep.h"
#include "vrt_voxelize.h"
#include "vrt_fill.h"
#include "vrt_distance.h"
#include "vrt_label.h"
#include "vrt_move.h"
#include "vrt_query.h"
#include "vrt_denoise.h"

#define VRT_RENDER_THREADS 256
#ifndef VRT_RENDER_MIN_WAVES
#define VRT_RENDER_MIN_WAVES 2   // waves per SIMD the register allocator must leave room for (tuned on MI355X)
#endif

// Work distribution: the render kernels pull (tile, sample, pixel) items from head words with returning atomics.
// One word saturates near 88 pulls/us chip-wide and answers in ~3 us with 256 CUs pulling (MI355X_MICROARCH.md, row
// `dequeue`), so the pooled kernel splits the items into VRT_WORK_HEADS contiguous ranges, one head per XCD on a
// 128-byte line of its own; a wave pulls from the head of its XCD and moves on to the next head when that range is
// used up.  Sixteen sets of heads rotate with the launch number (a launch zeroes the set eight launches ahead: vrt_kernels.hip).
#define VRT_WORK_HEADS 8
#define VRT_WORK_HEAD_STRIDE 32    // uints between heads
#ifndef VRT_POOL_WAVES
#define VRT_POOL_WAVES 4           // waves (= path pools) per workgroup of the pooled render kernel
#endif
#ifndef VRT_POOL_MIN_WAVES
#define VRT_POOL_MIN_WAVES 2
#endif

static_assert(VRT_PV_HEADS == VRT_WORK_HEADS, "the queue of vrt_primary.h has a part per work head");

// What the launchers of every kernel unit are written with.
#define VRT_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; } while (0)
// Kernel variants are picked by four switches; these macros spell the dispatch once.
#define VRT_BY_GRID(G_, CALL) do { if ((G_) == 256) { constexpr int G = 256; CALL; } else { constexpr int G = 128; CALL; } } while (0)
#define VRT_BY_2(A_, B_, CALL) do { if (A_) { constexpr bool A = true; if (B_) { constexpr bool B = true; CALL; } else { constexpr bool B = false; CALL; } } \
                                    else { constexpr bool A = false; if (B_) { constexpr bool B = true; CALL; } else { constexpr bool B = false; CALL; } } } while (0)

namespace vrt {

struct ProbeOut;   // vrt_probe.h (test hook; vrt_probe_kernels.hip and vrt_api.hip include it)

// grid_res (128 or 256) selects the kernel instantiation everywhere below (GridDim, vrt_types.h)
// ---- vrt_kernels.hip: the render launches and the frame passes
hipError_t query_render_residency(int grid_res, bool restir, bool instr, int* blocks_per_cu);
hipError_t launch_render(hipStream_t st, int grid_res, bool restir, bool instr, int n_blocks, const FrameParams& fp, const SceneData& sc,
                         const PixelBuffers& out, unsigned* work_counters, unsigned launch_seq, int n_samples, int chunk_override);
// pooled schedule (vrt_pool.h).  `v` (plan_render_variant, vrt_plan.h) picks the kernel and with it the workgroup geometry: the query
// answers for the kernel a launch with the same `v` runs.  `cold` holds n_blocks x scratch_per_block bytes at least.
hipError_t query_render_pool(int grid_res, const RenderVariant& v, int* blocks_per_cu, size_t* scratch_per_block);
hipError_t launch_render_pool(hipStream_t st, int grid_res, const RenderVariant& v, int n_blocks, const FrameParams& fp, const SceneData& sc,
                              const PixelBuffers& out, unsigned* work_counters, unsigned launch_seq, int n_samples, uint32_t* cold,
                              uint32_t* drain_signal,   // signal memory (or null): receives launch_seq + 1 when the launch starts to drain
                              PrimaryRecord* prim_cache,        // per-pixel camera-ray records shared by the fused samples (or null), npix entries
                              bool prim_served = false);        // launch_primary_records has been queued ahead of this launch, with its number
// The pre-pass of pooled launch number launch_seq (plan_prepass, vrt_plan.h): k_primary_records fills prim_cache with the records of the
// launch's camera rays under the launch's tag.  fp, sc, v: the launch's own.
hipError_t launch_primary_records(hipStream_t st, int grid_res, const RenderVariant& v, const FrameParams& fp, const SceneData& sc, PrimaryRecord* prim_cache,
                                  unsigned launch_seq);
// The primary vertices of pooled launch number launch_seq (plan_primary, vrt_plan.h), behind its pre-pass on the same stream: k_primary_vertex
// finishes the paths that end at or right behind the primary vertex and leaves the others in pq, whose counts the caller has zeroed in
// stream order.  launch_render_pool_queued is that launch: the same geometry, residency and scratch as launch_render_pool's.
hipError_t launch_primary_vertex(hipStream_t st, int grid_res, const RenderVariant& v, const FrameParams& fp, const SceneData& sc, const PixelBuffers& out,
                                 const PrimaryRecord* prim_cache, unsigned launch_seq, int n_samples, const PrimaryQueue& pq);
hipError_t launch_render_pool_queued(hipStream_t st, int grid_res, const RenderVariant& v, int n_blocks, const FrameParams& fp, const SceneData& sc,
                                     const PixelBuffers& out, unsigned* work_counters, unsigned launch_seq, int n_samples, uint32_t* cold,
                                     uint32_t* drain_signal, PrimaryRecord* prim_cache, const PrimaryQueue& pq);
#if defined(VRT_DEV_KNOBS)
// Test hook (VRT_TEST_SPOIL_RECORDS, vrt_plan.h): behind launch_primary_records on the same stream, the records of the launch's live pixels
// whose table index is launch_number mod n (mod n) fail their check from here on.  fp: the launch's own.
hipError_t launch_spoil_primary_records(hipStream_t st, const FrameParams& fp, PrimaryRecord* prim_cache, unsigned n, unsigned launch_number);
#endif
hipError_t launch_mat_derived(hipStream_t st, const float* mats, float* mats_x /*[128][8]*/);  // after every material upload
// spatial reuse over rows [r0, r1); first a per-pixel prepare pass over all rows the launch holds (fp.row0..fp.row1) into gb.geo / gb.src
hipError_t launch_gris(hipStream_t st, int grid_res, bool instr, const FrameParams& fp, const SceneData& sc, const GrisBuffers& gb, int r0, int r1);
// frame_prev: k_temporal_frame_prev (moving camera on a row tile with history exchange: hist_*_in / prev_* are whole-frame planes)
hipError_t launch_temporal(hipStream_t st, const FrameParams& fp, const TemporalBuffers& tb, int r0, int r1, int n_samples, bool frame_prev = false);
// the accumulation passes of tg.n_slices consecutive render launches over rows [r0, r1) in one kernel (vrt_temporal.h: temporal_group_pixel)
hipError_t launch_temporal_group(hipStream_t st, const TemporalGroup& tg, int r0, int r1);
hipError_t launch_tonemap(hipStream_t st, const FrameParams& fp, const f3* hdr, f4* ldr, int r0, int r1);
hipError_t launch_tonemap8(hipStream_t st, const FrameParams& fp, const f3* hdr, uint32_t* ldr8 /* rgba, 8 bits each */, int r0, int r1);
// vrt_denoise (vrt_denoise.h), whole frames of W x H.  The planes the pass reads of the context -- the last launch's g-buffer, the
// histories, the HDR frame -- and its own scratch: d[0] / s[0] hold step 1's signals, the iterations alternate between the other two.
struct DenoiseSource { const f3* gb_pos; const uint32_t* gb_normal; const uint32_t* gb_mat; const f4* hist_d; const f4* hist_s; const f3* hdr; };
struct DenoiseScratch { DenoiseGuide* guide; uint32_t* mat; f4* d[3]; f4* s[3]; };
// step 1 into the scratch; out (f32[H][W][3], device memory) receives the pixels that are no surface pixels.  Reads `src` and nothing else does
hipError_t launch_denoise_prepare(hipStream_t st, int W, int H, int moving, const DenoiseSource& src, const DenoiseScratch& scr, f3* out);
// set.iterations a-trous kernels at strides 1, 2, 4, ..; the last one fades, recomposes and writes the surface pixels of `out`
hipError_t launch_denoise_filter(hipStream_t st, int W, int H, const DenoiseSettings& set, const DenoiseScratch& scr, f3* out);
hipError_t launch_diag_read(hipStream_t st, unsigned long long* out, int reset);  // -DVRT_DIAG_REGIONS builds only
// ---- vrt_scene_kernels.hip: the calls that build or edit a scene
hipError_t launch_prepare(hipStream_t st, int grid_res, const int8_t* mat, const uint8_t* rgb, uint32_t* grid, unsigned long long* l0,
                          unsigned long long* l1, unsigned long long* l2, unsigned long long* l3, unsigned long long* l0c, uint32_t* l0c_base,
                          float* cull /*[6]: cull_ray()'s box, vrt_trace.h*/);
// vrt_update_voxels: the voxels of `box` (valid, not empty) replaced by box_mat / box_rgb (device memory, [hx][hy][hz] and [hx][hy][hz][3]),
// and everything launch_prepare derives from them brought up to date -- the levels' words the box touches, l0c and the culling box whole
hipError_t launch_edit(hipStream_t st, int grid_res, const EditBox& box, const int8_t* box_mat, const uint8_t* box_rgb, int8_t* mat, uint8_t* rgb,
                       uint32_t* grid, unsigned long long* l0, unsigned long long* l1, unsigned long long* l2, unsigned long long* l3,
                       unsigned long long* l0c, uint32_t* l0c_base, float* cull);
// vrt_fetch_voxels: the stored voxels of `box` (valid, not empty) gathered into box_mat / box_rgb (device memory)
hipError_t launch_fetch_voxels(hipStream_t st, int grid_res, const EditBox& box, const int8_t* mat, const uint8_t* rgb, int8_t* box_mat, uint8_t* box_rgb);
// vrt_voxelize_triangles (vrt_voxelize.h) and vrt_fill_triangles (vrt_fill.h).  The context's scratch, cut up by plan_tri_layout: `words`,
// the head region the raster kernel writes -- one ownership word per voxel of the clip box, or one toggle bit per voxel (fill_words
// words) -- the box arrays launch_edit takes, the item-list entries of a batch, heads[0] the set-up pass's counter (entries << 40 | items),
// heads[1] the rasterise pass's work head, and the result record (lo = INT32_MAX / hi = INT32_MIN while nothing is written; hi INCLUSIVE).
struct VoxResult { int32_t lo[3], hi[3]; unsigned long long voxels, invalid; };
struct TriScratch { uint32_t* words; int8_t* box_mat; uint8_t* box_rgb; VoxEntry* entries; unsigned long long* heads; VoxResult* res; };
// the head region's head_bytes zeroed, the result record opened
hipError_t launch_tri_begin(hipStream_t st, size_t head_bytes, const TriScratch& s);
// one batch of m <= plan_voxelize_batch() triangles (device memory), global numbers base .. base + m - 1: k_vox_setup, a lane a triangle,
// counts the items and writes the entries; k_vox_raster, a wave an item, raises the ownership words
hipError_t launch_voxelize_batch(hipStream_t st, int grid_res, int n_cu, const EditBox& clip, unsigned long long base, long long m, const vrt_triangle* tris,
                                 const TriScratch& s);
// k_vox_resolve, a lane a few voxels of the box: payloads of the owners among tris (global numbers from base), and with `final` the grid's
// stored voxels where nobody owns one, the count and the tight box
hipError_t launch_voxelize_resolve(hipStream_t st, int grid_res, const EditBox& clip, unsigned long long base, const vrt_triangle* tris, bool final,
                                   const int8_t* mat, const uint8_t* rgb, const TriScratch& s);
// one batch of m <= plan_voxelize_batch() triangles (device memory): k_fill_setup, a lane a triangle, counts the items and writes the
// entries; k_fill_raster, a wave an item, toggles one bit per owned column.  Batches need no order and no resolve between them.
hipError_t launch_fill_batch(hipStream_t st, int grid_res, int n_cu, const EditBox& clip, long long m, const vrt_triangle* tris, const TriScratch& s);
// k_fill_resolve, a lane a few voxels of the box, once after every batch: `voxel` where the prefix-XOR of the column says inside, the
// grid's stored voxel elsewhere; the count and the tight box of the inside cells
hipError_t launch_fill_resolve(hipStream_t st, int grid_res, const EditBox& clip, uint32_t voxel, const int8_t* mat, const uint8_t* rgb, const TriScratch& s);
// vrt_distance_field (vrt_distance.h).  The call's scratch cut up by plan_distance_layout: pass z's and pass y's values and, where
// `nearest` is asked for, the coordinates they chose (cz, cy: not touched otherwise).
struct DistScratch { int* a; int* b; uint8_t* cz; uint8_t* cy; };
// k_dist_z, k_dist_y, k_dist_x, one after the other on `st`: d2 (and nearest, unless NULL) of the cells of p.box (not empty), device memory
hipError_t launch_distance_field(hipStream_t st, int grid_res, const DistBox& p, const int8_t* mat, const DistScratch& s, int* d2, int* nearest);
// vrt_label_components (vrt_label.h): k_label_tile, k_label_seams (where the box has more than one tile) and k_label_finish, one after the
// other on `st`, behind a memset of `counters` (the 16-byte record k_label_finish adds members and roots to).  labels: int32 per cell of
// p.box (not empty), device memory, every word written; the union-find works in it.
hipError_t launch_label_components(hipStream_t st, const LabelBox& p, const int8_t* mat, int* labels, vrt_label_result* counters);
// vrt_move_voxels (vrt_move.h), p.src not empty; mat, rgb: the grid's arrays; snap: one word per cell of p.src; rec: the device's record.
// launch_move_count: k_move_begin, k_move_snapshot (select: int32 per cell of p.src in device memory, or null) and, where p.dst is not
// empty, the count pass k_move_dst<false>; the record is gathered per workgroup, one atomic a word.  The two array launches write box arrays for launch_edit -- the source box's (k_move_src), and
// behind the source box's edit the destination box's (k_move_dst<true>, p.dst not empty); both read rec->blocked.
hipError_t launch_move_count(hipStream_t st, const MovePlan& p, const int8_t* mat, const uint8_t* rgb, const int* select, uint32_t* snap, MoveRecord* rec);
hipError_t launch_move_src_arrays(hipStream_t st, const MovePlan& p, const int8_t* mat, const uint8_t* rgb, const uint32_t* snap, int8_t* box_mat, uint8_t* box_rgb,
                                  const MoveRecord* rec);
hipError_t launch_move_dst_arrays(hipStream_t st, const MovePlan& p, const int8_t* mat, const uint8_t* rgb, const uint32_t* snap, int8_t* box_mat, uint8_t* box_rgb,
                                  MoveRecord* rec);
// ---- vrt_query_kernels.hip: the queries against a prepared scene
// vrt_cast_rays: n rays (device memory) through cast_row (vrt_cast.h).  staged: the coarse pyramid levels in LDS, as k_render stages them;
// else everything through global memory.  oob: the instantiation that can read outside the grid the reference's way (sc.pyr.ref_oob).
// The grid is n_cu x the kernel's residency at most (plan_cast_blocks).
hipError_t launch_cast_rays(hipStream_t st, int grid_res, bool staged, bool oob, int n_cu, const FrameParams& fp, const SceneData& sc, long long n,
                            const vrt_ray* rays, vrt_ray_hit* hits);
// vrt_sweep_boxes: n boxes (device memory) through k_sweep_boxes, a wave a box (vrt_sweep.h); four boxes a workgroup per turn of its loop,
// the grid n_cu x the kernel's residency at most (plan_sweep_blocks).  Of sc the two finest pyramid levels and the culling box are read.
hipError_t launch_sweep_boxes(hipStream_t st, int grid_res, int n_cu, float floor_height, const SceneData& sc, long long n, const vrt_box_sweep* boxes,
                              vrt_sweep_hit* hits);
// A sampled query Q (vrt_query.h:RadianceQuery, SensorQuery, ProbeQuery): samples [s0, s0 + count) of n records (device memory) worked into
// plane[n * count] by the query's item kernel (k_trace_radiance, k_gather_irradiance, k_gather_probes) and folded into out[n] (k_fold_query).
// n * count <= Q::max_items; staged / oob as for launch_cast_rays; head: one word of device memory, the launch's work counter.
template <class Q>
hipError_t launch_sampled_query(hipStream_t st, int grid_res, bool staged, bool oob, int n_cu, const FrameParams& fp, const SceneData& sc, long long n, int s0,
                                int count, int n_samples, uint32_t first_frame, const typename Q::In* in, typename Q::Item* plane, typename Q::Out* out,
                                unsigned* head);
// ---- vrt_probe_kernels.hip: test hooks
hipError_t launch_detmath_probe(hipStream_t st, int op, int n, const float* a, const float* b, float* out);
// n rays (origin, direction: 6 floats each, voxel units) through walk PROBE_WALK_* against `cull`'s box (vrt_probe.h)
hipError_t launch_trace_probe(hipStream_t st, int grid_res, int walk, const Pyramid& pyr, const float* cull, int n, const float* rays, ProbeOut* out);
// n rows of in_stride floats through shading function `op` (vrt_shade_probe.h); lane_tables: n x VRT_SHADE_LANE_TABLE floats for SHADE_SHIFT, else null
hipError_t launch_shade_probe(hipStream_t st, const FrameParams& fp, const SceneData& sc, const float* mats_x, int op, int n, const float* in, int in_stride,
                              float* out, int out_stride, float* lane_tables);

// sky precompute (vrt_sky_kernels.hip)
struct SkyPrecompute {
    float* scattering;        // [res][res][3]
    float* transmittance;     // [res][res][3]
    uint16_t* trans_lut;      // [256][128][3] binary16
    const uint8_t* cloud_tex; // [256][256][3]
    float* cloud_ambient;     // [3]
    int res;
    float fres;
    int use_clouds;
    uint32_t seed;
};
hipError_t launch_sky_probe(hipStream_t st, const SkyPrecompute& sp, int op, int n, const float* in, int in_stride, float* out, int out_stride, f3 ambient);
hipError_t launch_sky_prepare(hipStream_t st, const SkyPrecompute& sp, f3 sun_dir, f3 sun_col, float sun_cos);
hipError_t launch_sky_clouds(hipStream_t st, const SkyPrecompute& sp, f3 sun_dir, f3 sun_col, float sun_cos, int max_samples,
                             uint32_t pass, int u0, int u1);   // table columns [u0, u1)
hipError_t launch_sky_slice(hipStream_t st, const SkyPrecompute& sp, f3 sun_dir, f3 sun_col, float sun_cos, int u0, int u1);

}  // namespace vrt
#endif
