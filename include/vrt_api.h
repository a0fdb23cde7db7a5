/* vrt_api.h -- C ABI of libvrt_hip.so, the MI355X (gfx950) replacement for the reference's
 * renderer/{pathtracer,raytracer,bsdf,atmos,reservoir,voxel_world}.py.
 *
 * The reference (taichi-dev/voxel-rt2) has no FFI: its seam is the Python object
 * `Renderer` that scene.py drives.  Every entry point below names the
 * reference interface it replaces as /root/reference-relative file:line.  The Python facade
 * voxel_rt2_amd/renderer.py binds these with ctypes and re-exposes the reference's method names.
 *
 * Conventions: single host thread per context; every int-returning function gives 0 or a
 * negative VRT_E_* code and vrt_last_error() a thread-local message; the library owns all
 * device memory; host pointers are borrowed for the duration of the call; work is queued on the
 * context's own HIP stream and is asynchronous until a fetch / sync / get_stats call.
 * There is NO CPU backend: vrt_create fails if no gfx950 device is usable.
 *
 * Layouts: images are row-major [row v][column u], v = 0 at the bottom like the reference's
 * (u, v) field indices.  Voxel arrays are [x+G/2][y+G/2][z+G/2] (C order; G = grid_res), the index space of
 * voxel_world.py:14-18.  Matrices are row-major 4x4 in mathematical convention (element
 * [row*4+col]); the facade has already transposed the glm-ordered arrays the reference receives
 * (pathtracer.py:266-268, 278-280) and supplies the inverses.
 */
#ifndef VRT_API_H
#define VRT_API_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vrt_ctx vrt_ctx;

enum {
    VRT_OK = 0,
    VRT_E_INVALID = -1,   /* bad argument / unsupported configuration */
    VRT_E_DEVICE = -2,    /* HIP error or no gfx950 device */
    VRT_E_STATE = -3      /* call out of order (e.g. accumulate before prepare) */
};

/* Renderer.__init__(dx, image_res, up, voxel_edges, exposure): pathtracer.py:28-136, plus the
 * module constants USE_RESTIR_PT / MAX_RAY_DEPTH (pathtracer.py:15-17) and the skybox size
 * (atmos.py:66-67) made into parameters. */
typedef struct vrt_config {
    int32_t width, height;        /* image_res */
    int32_t grid_res;             /* voxel_grid_res: 128 (pathtracer.py:83) or 256 (BASELINE config 5; VoxelWorld and
                                     VoxelOctreeRaytracer take it as a parameter: voxel_world.py:6, raytracer.py:7-9) */
    float dx;                     /* voxel size in world units, must be 2 / grid_res: the grid spans the world box
                                     [-1,1]^3 (scene.py:11: 1/64 at 128) */
    float voxel_edges;            /* voxel_world.py:25 */
    float exposure;               /* pathtracer.py:58 */
    int32_t max_depth;            /* MAX_RAY_DEPTH, 1..64 */
    int32_t use_restir;           /* USE_RESTIR_PT */
    uint32_t seed;                /* seed of the per-pixel random streams (replaces ti.random) */
    int32_t sky_res;              /* skybox edge length, 3840 in the reference; 0 = no sky tables */
    int32_t device;               /* HIP device ordinal */
    int32_t row_begin, row_end;   /* rows [row_begin,row_end) this context produces; 0,0 = all.
                                     Row-tile sharding across GPUs (one context per process). */
} vrt_config;

/* the scalar fields scene.py pokes with [None] (scene.py:148-169) and
 * Renderer.set_directional_light (pathtracer.py:139-144) */
typedef struct vrt_scene_params {
    float floor_height;
    float floor_color[3];
    int32_t floor_material;
    float background_color[3];
    float light_direction[3];     /* normalised */
    float light_cos_theta_max;    /* cos(cone_angle / 2) */
    float light_color[3];
    float light_weight;           /* 3.0 once set_directional_light ran (pathtracer.py:144) */
    int32_t use_physical_sky;
    int32_t use_clouds;
} vrt_scene_params;

/* set_camera_pos / set_proj_mat / set_view_mat / set_camera_is_moving / set_render_scale /
 * set_max_samples: pathtracer.py:146-150, 246-281, 1306-1307 */
typedef struct vrt_camera {
    float view[16], proj[16], view_inv[16], proj_inv[16];
    float pos[3];
    uint32_t jitter_index;        /* how many times set_proj_mat ran: selects the TAA jitter draw
                                     (pathtracer.py:264-265) from random stream 3 */
    int32_t camera_is_moving;
    float render_scale;
    float max_accum_frames;
} vrt_camera;

typedef struct vrt_stats {
    uint64_t path_samples;        /* pixels x accumulate passes since creation */
    uint64_t rays, dda_iters, occupancy_queries, closest_hits, sky_lookups; /* instrumented build only, else 0 */
    double render_ms, temporal_ms, gris_ms;  /* summed device time of the kernels (hipEvent).  Launches of up to 12 M work items (ReSTIR off)
                                                carry their timers one time in eight (the events cost a step of 0.15-0.3 ms 3-25 % of its
                                                rate); the sum is then the timed launches' mean times the number of all launches */
    uint32_t render_launches, temporal_launches, gris_launches;
    uint32_t pipeline_flags;      /* bit 0: launches of consecutive vrt_accumulate calls overlap; bit 1: the next launch's dispatch
                                     is held until the running one starts to drain (stream wait on a kernel-raised word; left out
                                     where a self-test finds that queue operations are serialised, e.g. under rocprofv3 --pmc);
                                     bits 2..4: HALF the render launches the pipeline keeps in flight (1, 2, 4 for 2, 4, 8; 0 while not overlapped).
                                     Launches of half the slots on TWO render streams (value 1 with 2 in bits 5..7) are the shape a runtime
                                     with fewer hardware queues than the four-deep pipeline has streams runs (GPU_MAX_HW_QUEUES below 6);
                                     the development build's three-stream shape (VRT_STREAMS=3) reports 2, the launch order it shares;
                                     bits 5..7: a launch takes 1 / this many of the workgroup slots (1, 2 or 4);
                                     bits 8..23: times the host released that wait (error paths, synchronisation watchdog);
                                     bits 24..31: times the pipeline was drained to change its depth (a caller that changes the
                                     sample count of its calls: the depth follows the launch size) -- EXCEPT in the two-stream shape of
                                     half-slot launches named above (1 in bits 2..4 with 2 in bits 5..7), where
                                     bit 24: the context's stream is a render lane -- launches take turns over the library's two streams
                                     and the context's (the caller's after vrt_set_stream), which is made to wait for the other lanes
                                     when an entry point looks at it or queues work on it, not with every launch; and
                                     bits 25..31: the times the pipeline was drained (at most 127) */
} vrt_stats;

/* buffers readable through vrt_fetch_buffer (tests and the multi-GPU gather) */
enum {
    VRT_BUF_GBUF_DEPTH = 1,       /* f32  [H][W]      gbuff_depth            pathtracer.py:114 */
    VRT_BUF_GBUF_NORMAL = 2,      /* f16x2[H][W]      gbuff_normals          :113 */
    VRT_BUF_GBUF_POSITION = 3,    /* f32x3[H][W]      gbuff_position         :116 */
    VRT_BUF_GBUF_MAT = 4,         /* u32  [H][W]      gbuff_mat_id           :112 */
    VRT_BUF_GBUF_REFL_DEPTH = 5,  /* f32  [H][W]      gbuff_depth_reflection :115 */
    VRT_BUF_HISTORY_DIFFUSE = 6,  /* f32x4[H][W]      history_buffer[...,0]  :43 */
    VRT_BUF_HISTORY_SPECULAR = 7, /* f32x4[H][W]      history_buffer_specular[...,0] :44 */
    VRT_BUF_SKY_SCATTERING = 8,   /* f32x3[R][R]      atmos.py:68 */
    VRT_BUF_SKY_TRANSMITTANCE = 9,/* f32x3[R][R]      atmos.py:69 */
    VRT_BUF_TRANS_LUT = 10        /* f16x3[256][128]  atmos.py:64 */
};

/* Renderer.__init__ (pathtracer.py:28). NULL on failure; see vrt_last_error(). */
vrt_ctx* vrt_create(const vrt_config* cfg);
void vrt_destroy(vrt_ctx* ctx);

/* Renderer.set_voxel / get_voxel storage (pathtracer.py:1325-1334, voxel_world.py:7-18):
 * mat int8[G^3], rgb uint8[G^3][3] with G = grid_res, index [x+G/2][y+G/2][z+G/2]. */
int vrt_upload_voxels(vrt_ctx* ctx, const int8_t* mat, const uint8_t* rgb);
/* MaterialList (materials.py:48-112): 128 rows of 14 f32 in bsdf.py:26-37 field order. */
int vrt_upload_materials(vrt_ctx* ctx, const float* table);
/* Atmos.load_textures (atmos.py:85-87): cloud tile uint8[256][256][3] indexed [x][y]. */
int vrt_upload_cloud_texture(vrt_ctx* ctx, const uint8_t* rgb);
int vrt_set_scene(vrt_ctx* ctx, const vrt_scene_params* scene);
int vrt_set_camera(vrt_ctx* ctx, const vrt_camera* cam);
/* Renderer.prepare_data (pathtracer.py:314-323): packed voxel grid, occupancy pyramid,
 * and with use_physical_sky the transmittance LUT + cloud ambient + cleared sky tables. */
int vrt_prepare(vrt_ctx* ctx);
/* Edit a PREPARED scene: replace the voxels of the box [lo, hi) -- coordinates in the index space of vrt_upload_voxels,
 * 0 <= lo <= hi <= grid_res per axis -- by mat int8[hx][hy][hz] and rgb uint8[hx][hy][hz][3] (C order, h = hi - lo).
 * on_device = 0: host arrays, borrowed for the call; on_device = 1: device memory that the kernel reads directly (a torch tensor's
 * data_ptr()), queued on the context's stream -- the caller keeps it unchanged until work queued on that stream behind the call
 * has run.  Afterwards everything vrt_prepare derives from the voxels (stored materials and colours, packed texels, every level of
 * the occupancy pyramid, the compacted fine level, the culling box and the host's view of it) is exactly what
 * vrt_upload_voxels(final grid) + vrt_prepare would have left, at a cost that follows the box and not the grid; what vrt_prepare
 * does that does not depend on voxels is left alone: the sky preparation, both sky tables, the cloud passes.  Histories and
 * g-buffers are NOT touched: the accumulated frame goes on blending old and new grid; a caller who wants a fresh accumulation
 * calls vrt_reset.  Render launches queued before the call see the old grid, launches queued after it the new one.  The call
 * synchronises with the device once (it reads the culling record back, as vrt_prepare does).
 * VRT_E_INVALID: NULL arguments, lo > hi, a box outside the grid, on_device not 0 or 1; VRT_E_STATE: before vrt_prepare, or after a
 * vrt_upload_voxels that no vrt_prepare has followed; an empty box returns VRT_OK and does nothing.  No counterpart in the
 * reference: its scene is authored before finish(), which never returns. */
int vrt_update_voxels(vrt_ctx* ctx, const int32_t lo[3], const int32_t hi[3], const void* mat, const void* rgb, int on_device);
/* Author a PREPARED scene from triangles: n caller-supplied triangles, in WORLD units, voxelised into the clip box [lo, hi) -- index
 * space of vrt_upload_voxels, 0 <= lo <= hi <= grid_res per axis, as for vrt_update_voxels -- on the device.
 * THE PAYLOAD.  voxel = r | g << 8 | b << 16 | (uint8_t)mat << 24, mat the int8 material byte as vrt_upload_voxels takes it.  A
 * negative byte is stored as it is and its texel gets alpha 0, as everywhere.  mat == 0 is valid and CARVES: covered voxels become
 * empty (and keep the payload's colour bytes).
 * THE SNAP.  A world component w becomes u = (w + 1.0f) * (float)(grid_res / 2) in binary32, uncontracted (include/vrt_detmath.h), then
 * s = (int32_t)rintf(u * 64.0f), round half to even: 64ths of a voxel.  The grid plane p(k) = (float)k * dx - 1.0f lands exactly on
 * s = 64 k, so what Renderer.box_of_voxels returns snaps to cell boundaries exactly.  Everything after the snap is exact integer
 * arithmetic on s; no float survives it.
 * VALIDITY.  A triangle is INVALID if a vertex component is non-finite or outside [-VRT_TRI_MAX_COORD, VRT_TRI_MAX_COORD]; it is
 * skipped and counted in result->invalid.  The bound keeps |s| <= (8 + 1) * 128 * 64 = 73 728 < 2^17; edge components are then < 2^18,
 * components of a cross product of two edges < 2^37, and every projection of a vertex or of a cell's corner onto one (three terms,
 * coordinates < 2^17) < 2^56: int64 never overflows.  reserved0 and reserved1 must be 0: on the host path this is checked before
 * anything runs (VRT_E_INVALID), on the device path such a triangle is treated as invalid.
 * COVERAGE.  Cell c is the closed cube [64 c_a, 64 c_a + 64]^3 in snapped units.  Triangle k COVERS cell c iff the closed triangle --
 * the convex hull of its three snapped vertices; a segment or a point is a valid hull -- and the closed cube share a point.  This is
 * decided by the separating-axis test in int64 on thirteen axes -- the three cube normals, the triangle's normal e0 x e1, the nine
 * e_i x axis_a (e0 = v1 - v0, e1 = v2 - v1, e2 = v0 - v2) -- separated iff the projections are STRICTLY apart on one of them.  The
 * test is complete for the degenerate hulls too: a segment's edges are parallel, so the nine cross products hold its direction
 * crossed with the cube's three, which with the cube normals is the segment / box test; a point leaves the cube normals, the
 * point-in-closed-box test; a zero axis separates nothing.  Consequence: a triangle lying exactly in a grid plane covers the cells
 * on BOTH sides of it, a vertex on a grid vertex covers eight cells.  A caller who wants one layer offsets by half a voxel.
 * THE RESULT.  Only cells inside the clip box exist.  Every cell of the box covered by at least one valid triangle takes the payload
 * of the covering triangle with the HIGHEST index -- later triangles paint over earlier ones, whatever the scheduling, the batches
 * or the host path's chunks -- and every other voxel keeps its content.  Afterwards everything vrt_prepare derives from the voxels
 * (stored materials and colours, packed texels, every level of the occupancy pyramid, the compacted fine level, the culling box and
 * the host's view of it) is exactly what vrt_upload_voxels(final grid) + vrt_prepare would have left; what vrt_prepare does that
 * does not depend on voxels is left alone: the sky preparation, both sky tables, the cloud passes.  Histories and g-buffers are NOT
 * touched (vrt_reset for a fresh accumulation).  Render launches and queries queued before the call see the old grid, those queued
 * after it the new one.  The call synchronises with the device once (it reads the culling record back, as vrt_update_voxels does).
 * `result` (may be NULL) receives the tight index box [lo, hi) of the WRITTEN cells -- those covered by a valid triangle, whether
 * or not their content changed; all six zero if there is none -- their count, and the number of invalid triangles.
 * on_device = 0: host triangles, borrowed for the call, staged in chunks (n is limited by memory only); ownership carries across
 * chunks by the triangles' global indices.  on_device = 1: device memory (a torch tensor's data_ptr()), read on the context's stream.
 * Scratch: 8 bytes per voxel of the box (4 of ownership, 4 of box arrays: 128 MB for a full 256^3 box) and 16 bytes per triangle of
 * a batch of at most 2^20; grown on demand, kept by the context, freed by vrt_destroy.
 * VRT_E_INVALID: NULL tris, lo or hi; n < 0 or n >= 2^32 - 1; lo > hi or a box outside the grid; on_device not 0 or 1; a non-zero
 * reserved word (host path).  VRT_E_STATE: before vrt_prepare, or after a vrt_upload_voxels that no vrt_prepare has followed.
 * n == 0 or an empty box returns VRT_OK, does nothing and zeroes the result.  Solid (interior) fill is vrt_fill_triangles, below.
 * Not done here: thin 6-separating voxelisation (the reserved words leave room for a mode), textures.  No counterpart in the
 * reference. */
typedef struct vrt_triangle { float v0[3]; uint32_t voxel; float v1[3]; uint32_t reserved0; float v2[3]; uint32_t reserved1; } vrt_triangle;   /* 48 bytes */
typedef struct vrt_voxelize_result { int32_t lo[3]; int32_t hi[3]; int64_t voxels; int64_t invalid; } vrt_voxelize_result;   /* 40 bytes */
#define VRT_TRI_MAX_COORD 8.0f
int vrt_voxelize_triangles(vrt_ctx* ctx, int64_t n, const vrt_triangle* tris, const int32_t lo[3], const int32_t hi[3],
                           vrt_voxelize_result* result, int on_device);
/* Author SOLIDS from triangles: the INSIDE of the n caller-supplied triangles, read as a closed mesh, filled with one payload inside
 * the clip box [lo, hi) of a prepared context, on the device.  vrt_voxelize_triangles writes a surface shell; this writes the volume.
 * TRIANGLES, SNAP, VALIDITY.  The same vrt_triangle records -- one device array serves both calls -- the same snap and the same
 * validity rule, reserved words included (host path: VRT_E_INVALID before anything runs; device path: the triangle is invalid).  An
 * invalid triangle is skipped and counted in result->invalid.  The triangles' own `voxel` words are ignored.
 * THE PAYLOAD.  `voxel` = r | g << 8 | b << 16 | (uint8_t)mat << 24 is the single payload of the call.  mat == 0 CARVES: inside cells
 * become empty.  A negative material byte is stored as it is (its texel gets alpha 0, as everywhere).
 * INSIDE.  Everything after the snap is exact integer arithmetic.  Cell c has the centre q = (64 c_x + 32, 64 c_y + 32, 64 c_z + 32)
 * in snapped units.  Cell c of the clip box is INSIDE iff an odd number of valid triangles CROSS BELOW it.  Geometrically: triangle k
 * crosses below c iff the vertical line (along z) through the point q + (eps, eps^2, eps^3), eps positive and infinitesimally small,
 * meets the triangle strictly below that point.  The perturbed point is generic -- it lies on no edge's projected line and on no
 * triangle's plane -- so nothing is ever "on" anything.  For any set of triangles that is closed (every edge shared an even number of
 * times) INSIDE is the ordinary parity of that point, whatever the triangles' orientation.  In integers, which is what is computed:
 *   e0 = v1 - v0, e1 = v2 - v1, n = e0 x e1 (as for COVERAGE above), sigma = sign(n_z).  n_z == 0: the triangle is edge-on or
 *   degenerate seen along z and crosses nothing.
 *   For each directed edge p -> r of v0 -> v1, v1 -> v2, v2 -> v0, with d = r - p: E = d_x (q_y - p_y) - d_y (q_x - p_x), and E' the
 *   sign of the first non-zero of (E, -d_y, d_x).  The COLUMN (c_x, c_y) is in the triangle iff sigma E' > 0 for all three edges.
 *   F = n . (q - v0), and F' the sign of the first non-zero of (F, n_x, n_y, n_z).
 *   Triangle k crosses below c iff the column is in and sigma F' > 0.
 * Consequences: along z a solid is the half-open interval [entry, exit) of cell centres -- a face through cell centres takes the
 * cells on its upper side in and leaves those of the face above it out; across a shared edge or vertex exactly one triangle owns a
 * column; two solids that share a face tile without gap or overlap; a duplicated triangle cancels itself; overlapping closed meshes
 * XOR -- nested spheres give a hollow ball; an OPEN mesh has a defined result (every cell above an odd number of its triangles),
 * which depends on the z axis.
 * Headroom: |q_a - v_a| < 2^17 and |d_a| < 2^18, so |E| < 2^36; |n_a| < 2^37, so |F| < 3 * 2^54 < 2^56: int64 never overflows.
 * THE CLIP BOX IS EXACT.  Only cells inside [lo, hi) are written.  A triangle below the box still counts for every cell of its
 * column; a triangle above or beside the box counts for none.  So filling a box in two halves equals filling it whole.
 * THE RESULT.  Every INSIDE cell of the box takes `voxel`; every other voxel keeps its content.  Afterwards everything vrt_prepare
 * derives from the voxels is exactly what vrt_upload_voxels(final grid) + vrt_prepare would have left, as for vrt_voxelize_triangles;
 * histories and g-buffers are NOT touched; launches and queries queued before the call see the old grid, those after it the new one;
 * the call synchronises with the device once.  `result` (may be NULL) receives the tight index box [lo, hi) of the INSIDE cells (all
 * six zero if there is none), their count, and the number of invalid triangles.
 * on_device = 0: host triangles, borrowed for the call, staged in chunks; = 1: device memory, read on the context's stream.  Neither
 * the chunks nor the scheduling can change a bit: toggles XOR.
 * Scratch: one toggle bit per voxel of the box (a column along z rounded up to whole 32-bit words), the box arrays (4 bytes a voxel)
 * and 16 bytes per triangle of a batch of at most 2^20; it shares vrt_voxelize_triangles' allocation, grown on demand, kept by the
 * context, freed by vrt_destroy.
 * Errors and empty cases are exactly vrt_voxelize_triangles': VRT_E_INVALID: NULL tris, lo or hi; n < 0 or n >= 2^32 - 1; lo > hi or a
 * box outside the grid; on_device not 0 or 1; a non-zero reserved word (host path).  VRT_E_STATE: before vrt_prepare, or after a
 * vrt_upload_voxels that no vrt_prepare has followed.  n == 0 or an empty box returns VRT_OK, does nothing and zeroes the result.
 * Not done here: a fill axis other than z, thin voxelisation, textures.  No counterpart in the reference. */
int vrt_fill_triangles(vrt_ctx* ctx, int64_t n, const vrt_triangle* tris, const int32_t lo[3], const int32_t hi[3],
                       uint32_t voxel, vrt_voxelize_result* result, int on_device);
/* Ask a PREPARED scene: n caller-supplied rays, in WORLD units, through the reference's next_hit (pathtracer.py:218-244: floor plane,
 * hierarchical DDA, surface lookup) on the context's current grid, floor, voxel_edges and scene parameters, in the mode
 * vrt_set_reference_indexing selected -- a query sees what the frames see.  Ray k gets next_hit(origin, dir, t_max,
 * shadow_ray = flags & VRT_RAY_ANY_HIT) in hits[k]:
 *   t       distance along the ray.  Directions are NOT normalised (the render's are not either): the hit point is origin + t * dir,
 *           and t is a distance in world units only for a unit dir;
 *   kind    VRT_HIT_MISS / VRT_HIT_FLOOR / VRT_HIT_VOXEL;
 *   cell    the voxel, in the index space of vrt_upload_voxels -- what vrt_update_voxels takes as lo (hi = lo + 1); -1 for the floor
 *           (with vrt_set_reference_indexing a "hit" outside the grid reports the coordinate -1 or grid_res it was read at);
 *   normal  facing the ray; albedo, mat_id: the edge-darkened colour (voxel_edges) and the material byte as the texel decodes it, or
 *           the floor's.  Zero for a VRT_RAY_ANY_HIT ray: no surface lookup is made for it; t, kind and cell are filled as for a full hit.
 * A miss is: nothing nearer than t_max (strictly: t < t_max, the floor tested first, so a floor / voxel tie is the floor's): t = +inf,
 * kind = 0, cell = -1, everything else zero.  t_max = +inf is the ordinary case.  INVALID rays are not walked and get the miss record:
 * a non-finite origin or direction component, a direction of all zeros, t_max NaN or <= 0.  Every other ray ends: the walk takes at
 * most 512 steps (raytracer.py:103) and a step descends at most one level per query, whatever finite values the ray holds.
 * on_device = 0: host arrays, borrowed for the call, staged in chunks (n is limited by memory only); the call returns when `hits` is
 * filled.  on_device = 1: both are device memory (a torch tensor's data_ptr()); the work is only queued on the context's stream, no
 * host synchronisation -- the caller keeps both unchanged until work queued on that stream behind the call has run.  Ordered like
 * vrt_update_voxels: a query queued after an edit sees the new grid, one queued before it the old.
 * The query READS scene data and nothing else: no history, g-buffer, counter, frame number or statistic is touched, the pending
 * accumulation (vrt_accumulate) is not forced, and frames rendered around it are bit for bit the frames rendered without it.
 * VRT_E_INVALID: NULL arguments, n < 0, on_device not 0 or 1; VRT_E_STATE: before vrt_prepare, or after a vrt_upload_voxels that no
 * vrt_prepare has followed; n = 0 returns VRT_OK.  No counterpart in the reference: next_hit is a ti.func of its render kernel. */
typedef struct vrt_ray { float origin[3]; float t_max; float dir[3]; uint32_t flags; } vrt_ray;   /* 32 bytes */
typedef struct vrt_ray_hit { float t; int32_t kind; int32_t cell[3]; float normal[3]; float albedo[3]; int32_t mat_id; } vrt_ray_hit;   /* 48 bytes */
enum { VRT_HIT_MISS = 0, VRT_HIT_FLOOR = 1, VRT_HIT_VOXEL = 2 };
enum { VRT_RAY_ANY_HIT = 1 };
int vrt_cast_rays(vrt_ctx* ctx, int64_t n, const vrt_ray* rays, vrt_ray_hit* hits, int on_device);
/* Ask a PREPARED scene where a moving box first touches it: n caller-supplied axis-aligned boxes, in WORLD units.  At parameter t box k
 * occupies [lo + t * move, hi + t * move]; hits[k] reports the smallest t in [0, t_max) at which the box's OPEN interior meets a solid
 * voxel or the floor.  move = 0 is the plain overlap test.  All arithmetic is binary32, uncontracted (include/vrt_detmath.h), left to
 * right as written; division is the correctly rounded one.
 * Plane k of the grid is p(k) = (float)k * dx - 1.0f (exact in binary32 for grid_res 128 and 256); cell c, in the index space of
 * vrt_upload_voxels, spans [p(c_a), p(c_a + 1)] on axis a.
 * ONE CELL.  For every axis a:
 *   move_a > 0:   e_a = (p(c_a) - hi_a) / move_a,      x_a = (p(c_a + 1) - lo_a) / move_a;
 *   move_a < 0:   e_a = (p(c_a + 1) - lo_a) / move_a,  x_a = (p(c_a) - hi_a) / move_a;
 *   move_a == 0 (either sign of zero): the axis overlaps iff lo_a < p(c_a + 1) && hi_a > p(c_a); then e_a = -inf, x_a = +inf, otherwise
 *                 the cell is never met.
 * enter = max(e_x, e_y, e_z) and exit = min(x_x, x_y, x_z), formed with dm_max / dm_min in axis order.  The cell is MET iff
 * enter < exit && exit > 0.  Met with enter < 0: the box overlaps the cell at the start.  Met with enter >= 0: a contact at
 * t = enter + 0.0f (a -0 becomes +0), which counts iff t < t_max; the contact axis is the lowest a with e_a == enter and the normal is
 * -1 or +1 on that axis, against the sign of move_a, zero on the other two.  Touching is not overlapping (the inequalities are strict):
 * a box resting on a voxel's top face is stopped at t = 0 when it moves down and slides free when it moves sideways.
 * THE FLOOR is the infinite plane y = floor_height, solid below -- not the render's radius-10 disc.  lo_y < floor_height: the box
 * overlaps it at the start.  Else, if move_y < 0: t_f = (floor_height - lo_y) / move_y + 0.0f, normal (0, 1, 0), which counts iff
 * t_f < t_max.  VRT_SWEEP_NO_FLOOR leaves the floor out.
 * THE RECORD.  (1) The floor overlaps at the start: kind = VRT_SWEEP_START, t = 0, cell = -1, normal = 0.  (2) Else a solid cell
 * overlaps at the start: kind = VRT_SWEEP_START, t = 0, cell = the overlapping cell with the smallest linear index (x * G + y) * G + z,
 * normal = 0.  (3) Else the smallest t over the floor and all solid cells wins: the floor is tested first, so a floor / voxel tie is the
 * floor's (kind = VRT_SWEEP_FLOOR, cell = -1); among cells with bit-equal t the smallest linear index wins (kind = VRT_SWEEP_VOXEL).
 * (4) Nothing is met: t = +inf, kind = VRT_SWEEP_MISS, cell = -1, normal = 0.
 * "Solid" is the bit of the occupancy pyramid's finest level (material > 0), and only cells inside the grid exist:
 * vrt_set_reference_indexing does NOT change the answer (there is no walk whose steps could leave the grid).
 * INVALID boxes are not tested and get the miss record: a non-finite field (t_max = +inf is allowed); lo_a > hi_a on some axis; a lo or
 * hi component outside [-VRT_SWEEP_MAX_COORD, VRT_SWEEP_MAX_COORD] (the grid is [-1, 1]^3; the bound keeps the rounding of p - hi far
 * below one cell); t_max NaN or <= 0.  lo == hi on an axis (a sheet, a segment, a point) is valid; move may be any finite value --
 * subnormal, 1e30, all zeros.  `reserved` must be 0: on the host path this is checked before anything runs (VRT_E_INVALID), on the
 * device path such a box is treated as invalid.  Every box ends: the work is bounded by the grid's (grid_res / 4)^3 bricks.
 * on_device = 0: host arrays, borrowed for the call, staged in chunks (n is limited by memory only); the call returns when `hits` is
 * filled.  on_device = 1: both are device memory (a torch tensor's data_ptr()); the work is only queued on the context's stream, no
 * host synchronisation -- the caller keeps both unchanged until work queued on that stream behind the call has run.  Ordered like
 * vrt_update_voxels: a query queued after an edit sees the new grid, one queued before it the old.
 * The query READS scene data and nothing else: no history, g-buffer, counter, frame number or statistic is touched, the pending
 * accumulation (vrt_accumulate) is not forced, and frames rendered around it are bit for bit the frames rendered without it.
 * VRT_E_INVALID: NULL arguments, n < 0, on_device not 0 or 1, a non-zero `reserved` (host path); VRT_E_STATE: before vrt_prepare, or
 * after a vrt_upload_voxels that no vrt_prepare has followed; n = 0 returns VRT_OK.  No counterpart in the reference: its scene is a
 * picture. */
typedef struct vrt_box_sweep { float lo[3]; uint32_t flags; float hi[3]; uint32_t reserved; float move[3]; float t_max; } vrt_box_sweep;   /* 48 bytes */
typedef struct vrt_sweep_hit { float t; int32_t kind; int32_t cell[3]; float normal[3]; } vrt_sweep_hit;   /* 32 bytes */
enum { VRT_SWEEP_MISS = 0, VRT_SWEEP_FLOOR = 1, VRT_SWEEP_VOXEL = 2, VRT_SWEEP_START = 3 };
enum { VRT_SWEEP_NO_FLOOR = 1 };
#define VRT_SWEEP_MAX_COORD 64.0f
int vrt_sweep_boxes(vrt_ctx* ctx, int64_t n, const vrt_box_sweep* boxes, vrt_sweep_hit* hits, int on_device);
/* How much light arrives along a ray: n caller-supplied rays, in WORLD units, each path-traced n_samples times on a PREPARED scene, and
 * the mean of the samples in out[k].  Sample s (0 <= s < n_samples) of ray k is one run of the reference's render body
 * (pathtracer.py:355-632) with ReSTIR off and a static camera, started at `origin` along `dir` instead of the camera's position and
 * get_cast_dir, on random stream (cfg.seed, first_frame + s, ray.stream, 0) -- a pixel's stream is (seed, frame, v * W + u, 0) -- and on
 * the context's current grid, floor, materials, scene parameters, sky tables and max_depth, in the mode vrt_set_reference_indexing
 * selected.  The estimator is the one without ReSTIR whatever cfg.use_restir says, and the camera's camera_is_moving is ignored: no
 * albedo demodulation.  The sample's value is diffuse + specular as the render forms them for its two colour buffers, each of the two
 * first replaced by zero where the temporal prepass would scrub it (pathtracer.py:1069-1075: a NaN, infinite or negative component).
 *   rgb   binary32, in this order: sum = 0; sum += value_s for s = 0 .. n_samples - 1, per component; then sum / (float)n_samples.  How
 *         the work is scheduled or cut into chunks does not change a bit of it;
 *   t     the distance of the ray's first hit: vrt_cast_rays' t for t_max = +inf, +inf for a ray that leaves into the sky.
 * Directions are NOT normalised (normalising a unit vector again can move a bit, and the camera's rays are taken as they are): the
 * estimator ASSUMES a unit dir -- the BSDF, the sun's cone and the sky lookup all read it as one.  `reserved` must be 0.
 * INVALID rays -- a non-finite origin or direction component, a direction of all zeros -- are not traced and get rgb = 0, t = +inf.
 * Every other ray ends: a path has at most max_depth segments, each a walk of at most 512 steps.
 * on_device = 0: host arrays, borrowed for the call, staged in chunks; the call returns when `out` is filled.  on_device = 1: both are
 * device memory; the work is only queued on the context's stream, no host synchronisation -- the caller keeps both unchanged until
 * work queued on that stream behind the call has run (`out` also carries the running sums between chunks).  Ordered like
 * vrt_update_voxels: a query queued after an edit sees the new grid, one queued before it the old.
 * The query READS scene data and nothing else: no g-buffer, reservoir, history, counter, frame number or statistic is touched, the
 * pending accumulation (vrt_accumulate) is not forced, and frames rendered around it are bit for bit the frames rendered without it.
 * VRT_E_INVALID: NULL arguments, n < 0, n_samples < 1 or > VRT_RADIANCE_MAX_SAMPLES, on_device not 0 or 1, a ray whose `reserved` is not
 * 0 (host path: checked before anything is traced; device path: the library does not read device memory on the host, such a ray is
 * treated as invalid); VRT_E_STATE: before vrt_prepare, or after a vrt_upload_voxels that no vrt_prepare has followed; n = 0 returns
 * VRT_OK.  No counterpart in the reference: its estimator can be reached through the camera only. */
typedef struct vrt_path_ray { float origin[3]; uint32_t stream; float dir[3]; uint32_t reserved; } vrt_path_ray;   /* 32 bytes */
typedef struct vrt_radiance { float rgb[3]; float t; } vrt_radiance;                                               /* 16 bytes */
enum { VRT_RADIANCE_MAX_SAMPLES = 65536 };
int vrt_trace_radiance(vrt_ctx* ctx, int64_t n, const vrt_path_ray* rays, int n_samples, uint32_t first_frame, vrt_radiance* out, int on_device);
/* How much light falls on a surface point: n caller-supplied sensors -- a point on a surface with its unit normal, in WORLD units -- on a
 * PREPARED scene, each sampled n_samples times, and the means in out[k].  Total irradiance is sky_rgb + sun_rgb; the caller adds them.
 * Sample s of sensor k uses frame f = first_frame + s and is, in binary32:
 *   1. g = the random stream (cfg.seed, f, sensor.stream, 4) -- 4: sensor directions; o = pos + normal * 1e-6 per component (a product,
 *      then a sum: pathtracer.py:428);
 *   2. the sun (pathtracer.py:436-468 without the BSDF and MIS factors): ldir = sample_cone_oriented(light_cos_theta_max, light_direction)
 *      on g's first two draws, ndl = dot(ldir, normal).  If ndl > 0 and the shadow ray next_hit(o, ldir, inf, shadow_ray) returns >= inf:
 *      vis_s = 1 and sun_s = ((T * light_weight) * light_color) * ndl, T = sample_skybox_transmittance(ldir) under use_physical_sky, else
 *      1.  Otherwise vis_s = 0 and sun_s = 0.  The shadow ray is cast even when the sun is black: `sun` is a visibility;
 *   3. the hemisphere: w = sample_cosine_weighted_hemisphere(normal) on g's next two draws.  L_s is what vrt_trace_radiance forms for ray
 *      (o, w, sensor.stream) at frame f -- a fresh path on stream (seed, f, stream, 0), scrubbed diffuse + specular -- except that a ray
 *      whose FIRST segment escapes into the sky is evaluated with hit_sun = 0: step 2 has counted the sun, the disc is not counted again.
 *      sky_s = 1 for such a ray, else 0.  hemi_s = L_s * 3.14159274f per component;
 *   4. four running sums over s = 0 .. n_samples - 1, in order: sky_rgb += hemi_s, sky += sky_s, sun_rgb += sun_s, sun += vis_s, each
 *      divided by (float)n_samples at the end.  How the work is scheduled or cut into chunks does not change a bit of them.
 * So `sky` is the share of the cosine-weighted hemisphere that is open, `sun` the share of the sun's disc that is visible.  The normal is
 * ASSUMED unit and is NOT normalised, as vrt_trace_radiance's dir.  `reserved` must be 0.
 * INVALID sensors -- a non-finite component, a normal of all zeros -- are not traced and get an all-zero record.  A sample of a valid
 * sensor whose normal is so far from unit that (o, w) is not a ray vrt_trace_radiance would trace (o overflows, or w comes out zero or
 * non-finite: a normal longer than about 1.8e19) is not walked either, and its four terms are zero.
 * n_samples, on_device, ordering, purity and error codes are vrt_trace_radiance's, word for word: n_samples in 1 ..
 * VRT_RADIANCE_MAX_SAMPLES; on_device = 0: host arrays, the call returns when `out` is filled; 1: device memory, queued on the context's
 * stream, `out` carries the running sums between chunks; a gather queued after an edit sees the new grid; the call READS scene data and
 * nothing else, does not force the pending accumulation and touches no statistic; it follows vrt_set_reference_indexing.
 * VRT_E_INVALID: NULL arguments, n < 0, n_samples out of range, on_device not 0 or 1, a sensor whose `reserved` is not 0 (host path:
 * checked before anything runs; device path: such a sensor is treated as invalid); VRT_E_STATE: before vrt_prepare; n = 0 returns VRT_OK.
 * No counterpart in the reference. */
typedef struct vrt_sensor { float pos[3]; uint32_t stream; float normal[3]; uint32_t reserved; } vrt_sensor;        /* 32 bytes */
typedef struct vrt_irradiance { float sky_rgb[3]; float sky; float sun_rgb[3]; float sun; } vrt_irradiance;         /* 32 bytes */
int vrt_gather_irradiance(vrt_ctx* ctx, int64_t n, const vrt_sensor* sensors, int n_samples, uint32_t first_frame, vrt_irradiance* out, int on_device);
/* The light at a point in EMPTY space, for any normal a caller may later present: n caller-supplied probes -- a position in WORLD units, no
 * normal -- on a PREPARED scene, each sampled n_samples times, and per probe the means in out[k]: nine spherical-harmonic coefficients per
 * colour channel of the radiance arriving from all directions, with the sun kept apart as a directional term (an irradiance volume's
 * record).  Sample s of probe k uses frame f = first_frame + s and is, in binary32 and uncontracted (include/vrt_detmath.h):
 *   1. g = the random stream (cfg.seed, f, probe.stream, 5) -- 5: probe directions;
 *   2. the sun: ldir = sample_cone_oriented(light_cos_theta_max, light_direction) on g's first two draws, exactly as vrt_gather_irradiance
 *      draws it.  The shadow ray next_hit(pos, ldir, inf, shadow_ray) is ALWAYS cast: there is no normal and so no ndl test.  If it returns
 *      >= inf: vis_s = 1 and sun_s = (T * light_weight) * light_color, T = sample_skybox_transmittance(ldir) under use_physical_sky, else 1.
 *      Otherwise vis_s = 0 and sun_s = 0.  This is the sun's irradiance on a surface that FACES it: the caller multiplies by
 *      max(0, dot(n, light_direction));
 *   3. the sphere: on g's next two draws u0, u1: a = 1 - 2 * u0, b = sqrt(1 - a * a), w = normalized((b * cos(2 pi u1), b * sin(2 pi u1), a))
 *      -- sample_cosine_weighted_hemisphere's lines without the normal and without the 1e-5 shrink: uniform on the sphere.  L_s is what
 *      vrt_gather_irradiance's step 3 forms for ray (pos, w, probe.stream) at frame f -- a fresh path on stream (seed, f, stream, 0),
 *      scrubbed diffuse + specular, and a ray whose FIRST segment escapes into the sky evaluated with hit_sun = 0: step 2 has counted the
 *      sun.  sky_s = 1 for such a ray, else 0.  The origin is pos itself, with no offset;
 *   4. the projection: with (x, y, z) = w, Lw = L_s * 12.5663706f per channel (4 pi: the uniform density is 1 / (4 pi)) and, each line
 *      evaluated left to right,
 *          Y0 = 0.282094792f                          Y1 = 0.488602512f * y          Y2 = 0.488602512f * z
 *          Y3 = 0.488602512f * x                      Y4 = 1.09254843f * (x * y)     Y5 = 1.09254843f * (y * z)
 *          Y6 = 0.315391565f * (3.0f * (z * z) - 1.0f)   Y7 = 1.09254843f * (x * z)     Y8 = 0.546274215f * (x * x - y * y)
 *      the term of coefficient i, channel ch is Lw[ch] * Yi;
 *   5. thirty-two running sums over s = 0 .. n_samples - 1, in order: sh[i][ch] += term, sky += sky_s, sun_rgb += sun_s, sun += vis_s, each
 *      divided by (float)n_samples at the end.  How the work is scheduled or cut into chunks does not change a bit of them.
 * The basis is the real spherical harmonics of bands 0 to 2 with the world's Z AS THE POLAR AXIS, in the order (l, m) = (0, 0), (1, -1),
 * (1, 0), (1, 1), (2, -2), (2, -1), (2, 0), (2, 1), (2, 2).  The world's UP is Y, not z: Y1 is the coefficient that tells up from down.
 * sh reconstructs radiance, L(d) ~ sum_i sh[i] * Yi(d); the irradiance on a unit normal n is
 * pi * sh[0] * Y0 + (2 pi / 3) * sum_{i = 1..3} sh[i] * Yi(n) + (pi / 4) * sum_{i = 4..8} sh[i] * Yi(n) + sun_rgb * max(0, dot(n, light_direction)).
 * `sky` is the open share of the sphere, `sun` the visible share of the sun's disc.
 * INVALID probes -- a non-finite pos component -- are not walked and get an all-zero record.  (A sample whose ray (pos, w) vrt_trace_radiance
 * would not trace is all zeros too; for a finite pos there is none.)  A probe INSIDE a solid voxel, below the floor or outside the grid's
 * box is NOT special-cased: it gets whatever next_hit gives from there.
 * n_samples, on_device, ordering, purity and error codes are vrt_gather_irradiance's, word for word: n_samples in 1 ..
 * VRT_RADIANCE_MAX_SAMPLES; on_device = 0: host arrays, the call returns when `out` is filled; 1: device memory, queued on the context's
 * stream, `out` carries the running sums between chunks; a gather queued after an edit sees the new grid; the call READS scene data and
 * nothing else, does not force the pending accumulation and touches no statistic; it follows vrt_set_reference_indexing.
 * VRT_E_INVALID: NULL arguments, n < 0, n_samples out of range, on_device not 0 or 1 (a probe has no `reserved` field to check);
 * VRT_E_STATE: before vrt_prepare; n = 0 returns VRT_OK.  No counterpart in the reference. */
typedef struct vrt_probe { float pos[3]; uint32_t stream; } vrt_probe;                                              /* 16 bytes */
typedef struct vrt_sh_probe { float sh[9][3]; float sky; float sun_rgb[3]; float sun; } vrt_sh_probe;                /* 128 bytes */
int vrt_gather_probes(vrt_ctx* ctx, int64_t n, const vrt_probe* probes, int n_samples, uint32_t first_frame, vrt_sh_probe* out, int on_device);
/* The mirror image of vrt_update_voxels: the stored materials and colours of the box [lo, hi) copied out as mat int8[hx][hy][hz] and
 * rgb uint8[hx][hy][hz][3] -- what a program reads after device-side edits, which the host never saw.  on_device = 0: host arrays, the
 * call synchronises; 1: device memory, queued on the context's stream.  Box rules and error codes are vrt_update_voxels'; the pending
 * accumulation is not forced. */
int vrt_fetch_voxels(vrt_ctx* ctx, const int32_t lo[3], const int32_t hi[3], void* mat, void* rgb, int on_device);
/* Ask a PREPARED grid how far each cell of the box [lo, hi) is from the nearest solid voxel, and which voxel that is: the exact
 * squared Euclidean distance field, on the device.
 * CELLS AND TARGETS.  Only cells inside the grid exist; they live in the index space of vrt_upload_voxels.  A cell is SOLID iff its
 * stored material byte is > 0 (signed) -- the bit of the occupancy pyramid's finest level, as for vrt_sweep_boxes.  The TARGETS are
 * the solid cells of the WHOLE grid; with VRT_DIST_TO_EMPTY in `flags` they are the non-solid cells of the whole grid.  The floor plane
 * is not a target.  vrt_set_reference_indexing does not change the answer.
 * DISTANCE.  D(c) = min over targets t of (c_x - t_x)^2 + (c_y - t_y)^2 + (c_z - t_z)^2, an integer: cell centres are one unit apart.
 * d2[c] = D(c) if a target exists and D(c) <= max_d2, else VRT_DIST_FAR.  A target cell has D = 0.  max_d2 >= 3 (grid_res - 1)^2 means
 * unbounded: no two cells are further apart.
 * NEAREST (may be NULL: then nothing is computed for it).  Where d2[c] is not VRT_DIST_FAR, nearest[c] is the linear index
 * (t_x * grid_res + t_y) * grid_res + t_z of the target that attains D(c); among several such targets the SMALLEST linear index wins,
 * which is lexicographic order in (x, y, z).  Where d2[c] is VRT_DIST_FAR, nearest[c] is -1.
 * OUTPUT AND COST.  d2 and nearest are int32[hx][hy][hz] over the cells of the box, C order, z fastest.  Targets outside the box count.
 * The cost follows the box grown by floor(sqrt(max_d2)) on every side and clipped to the grid, not the whole grid; that is exact, since
 * a target within max_d2 of a box cell differs from it by at most floor(sqrt(max_d2)) on every axis.
 * ORDERING AND PURITY are vrt_fetch_voxels': the call is queued on the context's stream, behind every edit queued so far and ahead of
 * later ones; the pending accumulation is not forced; no history, g-buffer, counter or statistic is touched, and frames rendered
 * around it are bit for bit the frames rendered without it.  on_device = 0: host arrays, the call returns when they are filled; = 1:
 * device memory, the work is only queued.
 * Scratch: a buffer of the context's own (neither the voxeliser's nor the query staging buffer), grown on demand, kept by the context,
 * freed by vrt_destroy: per voxel of the grown box at most 8 bytes of pass values (4 for the z pass over the box's z range, 4 for the
 * y pass over the box's y and z range) plus, with `nearest`, at most 2 bytes of chosen coordinates; on the host path 4 bytes per voxel
 * of the box for each staged result.  Unbounded over a whole 256^3 grid: 168 MB with `nearest`, 134 MB without.
 * VRT_E_INVALID: NULL ctx, lo, hi or d2; lo > hi or a box outside the grid (vrt_update_voxels' rules); max_d2 < 0 or
 * max_d2 > VRT_DIST_MAX_D2; unknown flag bits; on_device not 0 or 1.  VRT_E_STATE: before vrt_prepare, or after a vrt_upload_voxels that
 * no vrt_prepare has followed.  An empty box returns VRT_OK and writes nothing.  No counterpart in the reference. */
enum { VRT_DIST_TO_EMPTY = 1 };
#define VRT_DIST_FAR    0x7fffffff
#define VRT_DIST_MAX_D2 195075            /* 3 * 255^2: every distance a 256^3 grid holds */
int vrt_distance_field(vrt_ctx* ctx, const int32_t lo[3], const int32_t hi[3], int32_t max_d2, uint32_t flags,
                       void* d2 /* int32[hx][hy][hz] */, void* nearest /* int32[hx][hy][hz], may be NULL */, int on_device);
/* Ask a PREPARED grid which voxels of the box [lo, hi) hang together: connected-component labels, on the device.
 * CELLS AND MEMBERS.  Only the cells of the box take part; they live in the index space of vrt_upload_voxels.  A cell is SOLID iff its
 * stored material byte is > 0 (signed) -- the same rule as vrt_distance_field and vrt_sweep_boxes.  The MEMBERS are the solid cells of
 * the box; with VRT_LABEL_EMPTY in `flags` they are the non-solid cells of the box instead.  The floor plane is not a cell.
 * vrt_set_reference_indexing does not change the answer.
 * ADJACENCY.  Two members are adjacent iff their coordinates differ by at most 1 on every axis and by 1 in total (the 6 face
 * neighbours; the default); with VRT_LABEL_CONN_18 by at most 2 in total (faces and edges), with VRT_LABEL_CONN_26 by at most 3 (faces,
 * edges and corners).  Both connectivity flags at once are VRT_E_INVALID.  Cells outside the box DO NOT EXIST: a component that
 * continues outside the box is cut at the box's faces, and two parts of the box that are joined only through cells outside it are two
 * components -- on purpose, and unlike vrt_distance_field, whose targets outside the box count.  Cells outside the grid never exist.
 * LABEL.  A COMPONENT is a class of the transitive closure of adjacency.  labels[c] is the smallest linear GRID index
 * (x * grid_res + y) * grid_res + z among the cells of c's component, and -1 where c is not a member.  A cell is the ROOT of its
 * component iff labels[c] is its own index.  The labels are a function of the grid, the box and the flags alone.  At 256^3 they reach
 * 16 777 215 and stay positive in int32.  labels is int32[hx][hy][hz] over the cells of the box, C order, z fastest.
 * RESULT (may be NULL).  cells: the number of members; components: the number of roots; reserved: 0.  `result` lives where `labels`
 * lives: host memory with on_device = 0, device memory with on_device = 1.
 * ORDERING AND PURITY are vrt_distance_field's: the call is queued on the context's stream, behind every edit queued so far and ahead of
 * later ones; the pending accumulation is not forced; no history, g-buffer, counter or statistic is touched, and frames rendered
 * around it are bit for bit the frames rendered without it.  on_device = 0: host arrays, the call returns when they are filled; = 1:
 * device memory, the work is only queued: the call does not synchronise with the host.
 * Scratch: the union-find works in the output array itself.  Besides it the context holds a few counter words, and on the host path it
 * stages 4 bytes per box cell plus 16 -- in a buffer of the context's own (not the distance field's, the voxeliser's or the query
 * staging buffer), grown on demand, kept by the context, freed by vrt_destroy.
 * VRT_E_INVALID: NULL ctx, lo, hi or labels; lo > hi or a box outside the grid (vrt_update_voxels' rules); unknown flag bits or both
 * connectivity bits; on_device not 0 or 1.  VRT_E_STATE: before vrt_prepare, or after a vrt_upload_voxels that no vrt_prepare has
 * followed.  An empty box returns VRT_OK, writes no label and zeroes `result`.  No counterpart in the reference. */
enum { VRT_LABEL_EMPTY = 1, VRT_LABEL_CONN_18 = 2, VRT_LABEL_CONN_26 = 4 };
typedef struct vrt_label_result { int64_t cells; int32_t components; int32_t reserved; } vrt_label_result;            /* 16 bytes */
int vrt_label_components(vrt_ctx* ctx, const int32_t lo[3], const int32_t hi[3], uint32_t flags,
                         void* labels /* int32[hx][hy][hz] */, vrt_label_result* result /* may be NULL */, int on_device);
/* MOVE or COPY voxels of a PREPARED grid under an affine map, on the device: the piece found by vrt_label_components, carried as far as
 * vrt_sweep_boxes allows, turned, mirrored or scaled -- without the voxels visiting the host.  Integers only: the result is a function of
 * the stored voxels and the arguments alone, and no float exists anywhere in the library's part.
 * THE MAP takes a DESTINATION cell to its SOURCE cell (nearest-neighbour resampling: every destination cell asks where it comes from).
 * For a destination cell d, in int64: S_a = sum_b m[3a+b] * (2 d_b + 1) + t[a], a = 0..2, and the source cell is s_a = S_a >> 17, an
 * ARITHMETIC shift: a floor, so cells are half-open.  (2 d + 1) is the cell's centre in half voxels; m is Q16 (65536 = 1.0); Q16 times half
 * voxels is 2^-17 voxels, the unit of t.  VALID: |m[i]| <= 2^20 and |t[a]| <= 2^40.  THE BOUND: d < 256, so 2 d + 1 < 2^9, every product is
 * below 2^29 in magnitude, a row's three below 2^31 and S below 2^31 + 2^40 < 2^41: no int64 operation can overflow, and |s| < 2^24 fits
 * int32.  Singular, mirrored, scaling and shearing maps are all valid: the rule defines their result (the zero matrix draws every
 * destination cell from the one cell t names).  A turn that is no multiple of 90 degrees does not keep the number of voxels -- a source
 * cell may be drawn by no destination cell, or by two: that is what nearest-neighbour resampling does, and `written` and `erased` show it.
 * BEFORE.  Everything is read from the stored voxels as they are when the call's work starts (a snapshot): source and destination boxes
 * may overlap.
 * SELECTED.  Source cell c is selected iff select == NULL or select[c] == select_value; `select` is int32 over the cells of the source
 * box, C order, z fastest -- the labels of vrt_label_components over the same box plug in directly, select_value the component's root.
 * A PIECE CELL is a selected cell of the source box whose material byte BEFORE is > 0 (signed): the solid rule of vrt_label_components.
 * RECEIVES.  Cell d of the destination box receives iff s(d) lies in the source box and is a piece cell.  Only cells of the destination
 * box can receive.
 * VACATED.  With VRT_MOVE_ERASE_SOURCE every piece cell is vacated, whether or not any destination cell drew from it; without, none is.
 * OCCUPIED.  Cell d is occupied iff its material byte BEFORE is > 0 and it is not vacated.
 * FINAL GRID.  A receiving cell that is not both occupied and under VRT_MOVE_KEEP_SOLID takes the material and colour bytes of s(d) BEFORE
 * and is WRITTEN.  Otherwise a vacated cell becomes material 0, colour 0, 0, 0.  Every other voxel of the grid keeps its bytes.
 * RESULT (host memory, may be NULL).  written: the number of written cells; lo, hi: their tight box [lo, hi), all zero when there is
 * none; blocked: the number of receiving cells that are occupied (whatever VRT_MOVE_KEEP_SOLID then does with them); erased: the number
 * of vacated cells.
 * VRT_MOVE_IF_FREE.  If blocked > 0 nothing changes at all: written = erased = 0 and the box is zero; blocked is still reported.  The
 * device decides: there is no host round trip between the count and the edit.
 * VRT_MOVE_DRY_RUN.  The grid and all derived state keep every byte; the record is what the call would have reported.
 * STATE, ORDERING AND SYNCHRONISATION are vrt_update_voxels': everything vrt_prepare derives from the voxels is what a fresh upload of
 * the final grid and a vrt_prepare would leave; histories and g-buffers are not touched (vrt_reset is the caller's); the call is queued
 * on the context's stream, ordered against launches, queries and other edits, and forces the pending accumulation first.  It waits for
 * the device exactly once, for the result and the culling record.  A dry run is ordered like vrt_fetch_voxels instead: it forces nothing.
 * `select` with select_on_device = 0 is host memory, staged by the call; with 1 it is device memory, read in place.
 * EMPTY BOXES.  An empty source box does nothing and zeroes the result.  An empty destination box with a non-empty source box receives
 * nothing and still vacates under VRT_MOVE_ERASE_SOURCE: the rule is applied, not special-cased.
 * Scratch: a buffer of the context's own (no other call's), grown on demand, kept by the context, freed by vrt_destroy: 4 bytes per cell
 * of the source box for the snapshot, 4 bytes per cell of the LARGER of the two boxes for the box arrays the edits take, 4 bytes per
 * cell of the source box for a staged selection, and under 1 KB of record and padding.  A whole 256^3 grid onto itself: 134 MB, 201 MB
 * with a host selection.
 * VRT_E_INVALID: NULL ctx or move; a source or destination box with lo > hi or outside the grid (vrt_update_voxels' rule); m or t out of
 * bounds; unknown flag bits; reserved != 0; select_on_device not 0 or 1.  VRT_E_STATE: before vrt_prepare, or after a vrt_upload_voxels
 * that no vrt_prepare has followed.  Every argument is checked on the host before anything is launched.  No counterpart in the reference. */
enum { VRT_MOVE_ERASE_SOURCE = 1, VRT_MOVE_KEEP_SOLID = 2, VRT_MOVE_DRY_RUN = 4, VRT_MOVE_IF_FREE = 8 };
typedef struct vrt_voxel_move {            /* 120 bytes */
    int32_t src_lo[3], src_hi[3];          /* the source box [lo, hi), index space of vrt_upload_voxels */
    int32_t dst_lo[3], dst_hi[3];          /* the destination box: the only cells that can receive */
    int32_t m[9];                          /* row-major 3x3, Q16: maps DESTINATION to SOURCE */
    int32_t select_value;
    int64_t t[3];                          /* in 2^-17 voxels */
    uint32_t flags, reserved;              /* reserved == 0 */
} vrt_voxel_move;
typedef struct vrt_move_result { int32_t lo[3], hi[3]; int64_t written, blocked, erased; } vrt_move_result;   /* 48 bytes */
int vrt_move_voxels(vrt_ctx* ctx, const vrt_voxel_move* move, const void* select /* int32[src box], C order, or NULL */,
                    int select_on_device, vrt_move_result* result /* host, may be NULL */);
/* Renderer.accumulate_clouds / compute_atmosphere (pathtracer.py:325-329) */
int vrt_sky_accumulate_clouds(vrt_ctx* ctx, int max_samples);
int vrt_sky_compute_slice(vrt_ctx* ctx, int slice_idx, int max_slices);
/* The same precompute split across GPUs (the reference already slices the atmosphere pass by table columns,
 * atmos.py:159-164, scene.py:243-253): one cloud pass (atmos.py:140-157) over the columns of ONE slice, and the copy of table
 * columns between the library's tables and caller-owned device memory that an all-gather needs.  A texel depends on no other
 * texel in either pass, so a rank that owns slice r runs the cloud passes and the atmosphere pass on slice r only and the
 * ranks exchange columns: voxel_rt2_amd/parallel.py, precompute_sky_sharded(). */
int vrt_sky_accumulate_clouds_slice(vrt_ctx* ctx, int max_samples, int slice_idx, int max_slices);
int vrt_sky_table_io(vrt_ctx* ctx, int which /* VRT_BUF_SKY_SCATTERING | VRT_BUF_SKY_TRANSMITTANCE */, int u0, int u1,
                     void* device_ptr /* f32[u1-u0][sky_res][3] */, int to_library);
/* Renderer.accumulate (pathtracer.py:1310-1319), n_samples times.
 * The call queues its render launches; the ACCUMULATION of a launch (temporal filter -> histories, HDR frame) may be queued later
 * than the call that rendered it: with a static camera at render scale 1, ReSTIR off and no tile ring (vrt_set_hdr_targets),
 * history exchange or row stripes, the library accumulates several consecutive launches in one pass, each with the camera and
 * scene parameters that stood when ITS call was made -- vrt_set_camera (a new jitter), vrt_set_scene and vrt_end_frame between
 * calls neither force nor disturb it.  The pending accumulation is queued on the context's stream, before anything else the call
 * does, by every call that can observe or change what a pass per launch would have produced: vrt_sync, every vrt_fetch_*
 * (blocking, device, async), vrt_fetch_buffer and vrt_denoise, vrt_get_stats / vrt_reset_stats, vrt_reset, vrt_set_stream,
 * vrt_set_hdr_targets, vrt_set_history_exchange / vrt_history_rows_io, vrt_set_row_stripes, vrt_upload_*, vrt_update_voxels, vrt_prepare,
 * vrt_set_instrumented, vrt_set_reference_indexing, vrt_destroy, a vrt_accumulate call whose launch is of another kind (moving
 * camera, render scale below 1, another pipeline depth) or fails.  Results are those of a pass per launch, bit for bit; a caller
 * that orders its own work on the context's stream behind a frame (an event for another stream) calls vrt_sync or a fetch first.
 * vrt_stats counts one accumulation pass per render launch as before. */
int vrt_accumulate(vrt_ctx* ctx, int n_samples);
/* Renderer.reset_framebuffer (pathtracer.py:664-668) / copy_prev_matrices (283-287) */
int vrt_reset(vrt_ctx* ctx);
int vrt_end_frame(vrt_ctx* ctx);
/* color_buffer after accumulate() = the HDR frame: f32[H][W][3].  Rows outside
 * [row_begin,row_end) are zero. */
int vrt_fetch_hdr(vrt_ctx* ctx, float* out);
/* same, this context's rows only, copied device-to-device into caller-owned device memory
 * (f32[row_end-row_begin][W][3]); the call returns after the copy completed. */
int vrt_fetch_hdr_device(vrt_ctx* ctx, void* device_ptr);
/* same copy, only queued on the context's stream (no host synchronisation) */
int vrt_fetch_hdr_device_async(vrt_ctx* ctx, void* device_ptr);
/* Queue all further work of this context on the caller's HIP stream (e.g. torch.cuda.current_stream().cuda_stream),
 * so that rendering, the tile copy and a following RCCL collective are ordered on the device without host
 * round trips; NULL returns to a private stream.  The stream must outlive the context or be reset first.
 * Everything a caller can observe (results, fetches, stats) is ordered on this stream.  Render launches of
 * consecutive vrt_accumulate calls may run on two to eight internal streams of the context so that one starts while the
 * previous one drains; each is followed, on THIS stream, by the temporal pass that waits for it (one pass for several
 * launches where the accumulation is deferred: vrt_accumulate).  How many streams depends on the launch size and on the
 * hardware queues the HIP runtime was started with (GPU_MAX_HW_QUEUES, read at vrt_create): busy streams that share a
 * queue serialise, so with the runtime's default of four a 1080p context runs two render streams, with sixteen four. */
int vrt_set_stream(vrt_ctx* ctx, void* hip_stream);
/* Renderer.fetch_image (pathtracer.py:1321-1323, 634-662): LDR rgba f32[H][W][4] */
int vrt_fetch_ldr(vrt_ctx* ctx, float* out);
/* The reference presents EVERY frame (scene.py:255-262: accumulate, fetch_image, copy_prev_matrices).  These forms of
 * vrt_fetch_hdr / vrt_fetch_ldr queue the tonemap and the copy behind the passes queued so far, on a stream of the
 * library's own, and return: the caller goes on queueing frames and collects the image with vrt_fetch_wait(slot),
 * slot = 0..3 chosen by the caller, one fetch per slot at a time.  `out` should be page-locked memory (vrt_host_alloc) so
 * that the copy runs beside the following launches; for a shard only its rows of `out` are written. */
int vrt_fetch_hdr_async(vrt_ctx* ctx, float* out, int slot);
int vrt_fetch_ldr_async(vrt_ctx* ctx, float* out, int slot);
/* the LDR image as rgba8[H][W][4] = u8(clamp(c, 0, 1) * 255 + 0.5): what a display or a PNG takes, a quarter of the bytes
 * (at 1080p the f32 image is 33 MB a frame, more than the host link carries at a frame per millisecond) */
int vrt_fetch_ldr8_async(vrt_ctx* ctx, uint8_t* out, int slot);
int vrt_fetch_wait(vrt_ctx* ctx, int slot);
/* page-locked host memory for the asynchronous fetches (hipHostMalloc / hipHostFree) */
int vrt_host_alloc(vrt_ctx* ctx, uint64_t bytes, void** out);
int vrt_host_free(vrt_ctx* ctx, void* ptr);
/* Multi-GPU hand-over without a copy (the RCCL gather of the row tiles): the last temporal pass of every
 * vrt_accumulate call also writes this context's HDR rows (f32[row_end-row_begin][W][3]) to device_ptrs[k % n], k = tiles
 * written so far (vrt_hdr_targets_written); n = 0 ends it.  The pass is queued on the context's stream by the call, so an
 * event the caller records on that stream afterwards orders the gather behind the tile; n must exceed the gathers the
 * caller keeps in flight. */
int vrt_set_hdr_targets(vrt_ctx* ctx, void* const* device_ptrs, int n);
int vrt_hdr_targets_written(vrt_ctx* ctx, uint64_t* count);
/* Multi-GPU partition by INTERLEAVED ROW STRIPES instead of contiguous row tiles ("prefer interleaved 8-row stripes
 * (row_tile % 8 == rank) if contiguous tiles miss the target"): a whole-frame context (row_begin = row_end = 0) produces, of every
 * stripe_rows * n_parts rows, the stripe_rows rows starting at part * stripe_rows -- every rank then carries the frame's average
 * cost by construction, without a balancing pass.  stripe_rows is a multiple of 8 (the pixel tile, pathtracer.py:74); each stripe
 * is rendered with two more rows either side (what the accumulation pass reads of its neighbours: (stripe_rows + 4) / stripe_rows
 * of the work -- 32 rows: +12.5 %).  Buffers stay frame-sized; vrt_fetch_hdr returns the frame with the other rows zero;
 * vrt_fetch_hdr_device / the tiles of vrt_set_hdr_targets hold the context's rows stripe after stripe.  Static camera, ReSTIR off.
 * Call before the first vrt_accumulate; stripe_rows = 0 turns it off.  No counterpart in the reference (one GPU). */
int vrt_set_row_stripes(vrt_ctx* ctx, int stripe_rows, int n_parts, int part);
/* The MOVING camera on contiguous row tiles (set_camera_is_moving, scene.py:206-262).  The moving-camera accumulation pass resamples
 * the previous frame's histories, depth and normals at each pixel's reprojected position (pathtracer.py:993-1000, 1092-1183), which
 * can be any row of the frame, while a tile's buffers hold its own rows and a halo.  A row tile that opts in keeps a whole-frame copy
 * of that previous state; each vrt_accumulate call stores the tile's own rows in it (behind the call's last pass, on the context's
 * stream), and the caller imports every other row from the other tiles between calls (voxel_rt2_amd/parallel.py, exchange_history).
 * Per step: vrt_accumulate(1) -> export own rows / all-gather / import the others -> vrt_set_camera / vrt_reset -> vrt_accumulate.
 *   vrt_set_history_exchange: before the first vrt_accumulate (else VRT_E_STATE).  On a row tile it allocates the planes (40 B a
 *     pixel of the whole frame), zeroed like a fresh context's state; on a whole-frame context it is accepted and changes nothing;
 *     with row stripes (either order) VRT_E_INVALID: stripes stay static-camera only.  vrt_set_camera accepts camera_is_moving on a
 *     row tile only with it on.  A moving vrt_accumulate on such a tile takes n_samples = 1 (else VRT_E_INVALID) and needs every row
 *     outside the tile's own imported since the previous call (else VRT_E_STATE; not before the first call).  vrt_reset also
 *     zeroes the whole frame's histories (every rank resets in the same step); imported g-buffer rows stay.
 *   vrt_history_rows_io: rows [row0, row1) between the library and caller-owned DEVICE memory, queued on the context's stream.
 *     Record: four planes back to back, each [row1-row0][W]: diffuse history f32x4, specular history f32x4, g-buffer depth f32,
 *     g-buffer normal u32 (the oct encoding of VRT_BUF_GBUF_NORMAL) -- 40 bytes a pixel.  to_library = 0 exports rows inside the
 *     context's own rows, as the most recent vrt_accumulate left them; 1 imports rows outside them (row tile with the exchange on,
 *     else VRT_E_STATE).  Other ranges: VRT_E_INVALID.  No counterpart in the reference (one GPU). */
int vrt_set_history_exchange(vrt_ctx* ctx, int on);
int vrt_history_rows_io(vrt_ctx* ctx, int row0, int row1, void* device_ptr, int to_library);
int vrt_fetch_buffer(vrt_ctx* ctx, int which, void* out);
/* The accumulated frame through a spatial filter, for the frames that have few samples behind them (after a vrt_reset, behind a moving
 * camera): an edge-avoiding a-trous filter -- B3-spline 5x5, the stride doubling per iteration -- over albedo-demodulated diffuse and over
 * specular, each by itself; taps gated by material id, normal and distance to the centre pixel's plane and weighted by their sample
 * count; the result fades back to the unfiltered accumulation as the pixel's own sample count grows.  out: f32[H][W][3], laid out like
 * vrt_fetch_hdr's.  on_device = 0: host memory, the call returns when `out` is filled; 1: device memory, the work is only queued on the
 * context's stream.  params = NULL means {5, 0.25f, 0.5f, 64.0f}: defaults of TASTE, not validated on images by anybody.
 * The call forces the pending accumulation (vrt_accumulate) as every fetch does, and then READS and nothing else: no history, g-buffer,
 * HDR buffer, counter or statistic is written, and frames rendered after it are bit for bit the frames rendered without it.  Launches
 * queued after the call do not overtake it: it has read what they write before they write it.
 * Inputs, with idx = v * W + u, each exactly what vrt_fetch_buffer / vrt_fetch_hdr would return at the moment of the call:
 *   Hd, Hs  VRT_BUF_HISTORY_DIFFUSE, VRT_BUF_HISTORY_SPECULAR (f32x4; w: the samples behind the pixel)
 *   P       VRT_BUF_GBUF_POSITION           N   oct_decode(VRT_BUF_GBUF_NORMAL) (math_utils.py:209-215 on the two binary16 halves)
 *   M       VRT_BUF_GBUF_MAT: id = M & 255, A = unpack_albedo(M) = (float)((M >> 8, 16, 24) & 255) / 255.0f per channel
 *   HDR     vrt_fetch_hdr
 *   moving  camera_is_moving of the camera the most recent vrt_accumulate rendered with (recorded at that call: vrt_set_camera may
 *           have run since)
 * Arithmetic: binary32, uncontracted (include/vrt_detmath.h), every expression left to right as written, 3-vector operations per
 * channel; dot3(a, b) = a.x * b.x + a.y * b.y + a.z * b.z and lum(c) = dot3((0.2125f, 0.7154f, 0.0721f), c).
 *   1. Split and demodulate.  A pixel is a SURFACE pixel unless P.x * P.x + P.y * P.y + P.z * P.z < 1e-7f.  For a surface pixel
 *      A' = dm_max(A, 0.00392156886f), Id = moving ? Hd.xyz : Hd.xyz / A' (the moving camera's diffuse history is demodulated already),
 *      Is = Hs.xyz, and the counts cd = Hd.w, cs = Hs.w, which stay as they are through all iterations.
 *   2. Iterations i = 0 .. iterations - 1 at stride s = 1 << i, on the two signals X = d, s independently.  For a surface pixel p =
 *      (u, v): sum = 0, wsum = 0; taps dy = -2 .. 2 (outer loop), dx = -2 .. 2 (inner loop), q = (u + dx * s, v + dy * s).  A tap is
 *      skipped when q lies outside the frame, when q is no surface pixel, and unless ALL of id_q == id_p, dot3(N_p, N_q) >= 0.9f and
 *      dm_abs(dot3(N_p, P_q - P_p)) <= tol hold, tol = plane_tolerance * cfg.dx formed once; the centre is a tap like any other.
 *      w = (K[|dx|] * K[|dy|]) * c_q with K = {0.375f, 0.25f, 0.0625f} and c_q the tap's count for this signal.  For i >= 1 and
 *      sigma_l > 0: lp = lum(X_p), lq = lum(X_q), t = dm_abs(lq - lp) / (sigma_l * ((lp + lq) * 0.5f) + 0.001f), w = w / (1.0f + t * t).
 *      sum = sum + w * X_q, wsum = wsum + w.  X'_p = wsum > 0 ? sum / wsum : X_p.  An iteration reads the previous iteration's values only.
 *   3. Fade and recompose.  F: the last iteration's value, U: step 1's.  Per signal a = full_at > 0 ? dm_min(c_p / full_at, 1.0f) : 0.0f
 *      and R = F + (U - F) * a; out = (R_d * (moving ? A : A')) + R_s.  A pixel that is no surface pixel gets HDR[idx], bit for bit.
 * VRT_E_INVALID: NULL ctx or out, on_device not 0 or 1, iterations outside 1 .. 6, a plane_tolerance, sigma_l or full_at that is not
 * finite or is negative.  VRT_E_STATE: no vrt_accumulate since vrt_create or since the last vrt_reset; a row tile (row_begin / row_end),
 * row stripes or the history exchange (the filter reaches 62 rows, a tile holds a 2-row halo); the most recent vrt_accumulate rendered
 * at a render scale other than 1.  ReSTIR, the moving camera, instrumented launches, reserved CUs and vrt_set_reference_indexing are all
 * allowed.  No counterpart in the reference, which shows its frames as they accumulate. */
typedef struct vrt_denoise_params { int32_t iterations; float plane_tolerance; float sigma_l; float full_at; } vrt_denoise_params;   /* 16 bytes */
int vrt_denoise(vrt_ctx* ctx, const vrt_denoise_params* params, void* out, int on_device);
/* waits for everything queued so far, the accumulation of every rendered launch included (see vrt_accumulate) */
int vrt_sync(vrt_ctx* ctx);
int vrt_get_stats(vrt_ctx* ctx, vrt_stats* out);
int vrt_reset_stats(vrt_ctx* ctx);
const char* vrt_last_error(void);
/* The render kernels are persistent: their grid fills every CU (two workgroups of 79 KB LDS each, or one of 148 KB at
 * grid_res 256), so another kernel -- an RCCL collective of a multi-GPU run -- finds no workgroup slot until a launch
 * drains.  This leaves n_cus CUs' worth of slots out of the grid (0 = none, the single-GPU default).  No counterpart in the
 * reference (one GPU, pathtracer.py); voxel_rt2_amd/parallel.py calls it when the process group has more than one rank. */
int vrt_reserve_cus(vrt_ctx* ctx, int n_cus);
/* Select the kernel variants that count rays / DDA iterations / occupancy queries / hits
 * (vrt_stats.rays etc.); off by default -- the counters are what the reference's disabled
 * iteration heat-map (pathtracer.py:419-425) would have shown.  on = 1 counts the reference algorithm's work (every
 * camera ray walked, as the reference and the oracle do); on = 2 counts what the timed schedule does (the samples fused
 * into one launch share their camera rays, so a pixel's camera ray is walked -- and counted -- once). */
int vrt_set_instrumented(vrt_ctx* ctx, int on);
/* Occupancy queries OUTSIDE the grid.  The reference's walk can take one more step after its ray has left the grid
 * (hit_distance a rounding error short of `far`, raytracer.py:104) and then calls query_occupancy with a cell coordinate of -1
 * or grid_res; linearize_index (raytracer.py:17-38) does not check, so the bit it reads belongs to ANOTHER cell (x = 128 is
 * x = 0 of the next row; z = 128 at LOD 0 is the start of the LOD-1 region) and a set bit is reported as a hit on a voxel
 * outside the grid, which voxel_surface_color paints black (voxel_world.py:27-32, 46): black specks on the far faces of dense
 * grids.  on = 0 (default): such a query reads "empty" -- the walk's documented meaning.  on = 1: it reads the bit the
 * reference's index arithmetic addresses (bits before the array or behind its 2 * grid_res^3 read 0), so the frame equals
 * what the reference's source computes, specks included; every ray is walked (no culling) and the launches use the
 * instrumented kernel instantiations, which carry that code.  Takes effect at the next vrt_accumulate. */
int vrt_set_reference_indexing(vrt_ctx* ctx, int on);
/* Hash of the sources this library was built from (voxel_rt2_amd/build.py): ties measured counters
 * (profiles/traffic.json) to the build they were measured on. */
const char* vrt_build_id(void);
/* Evaluate one vrt_detmath.h operation on the device (numeric-contract test hook):
 * op 0 sin 1 cos 2 exp 3 log 4 pow 5 acos 6 atan2 7 min 8 max 9 f16 round trip 10 a/b 11 sqrt
 * 12 a*b+a (uncontracted) 13 float->int. */
int vrt_detmath_probe(int device, int op, int n, const float* a, const float* b, float* out);
/* Evaluate single functions of the sky / cloud precompute on the device (test hook; the rows the reference's own atmos.py was
 * executed on: tests/golden/reference/functions_sky.npz).  op: 0 rsi (atmos.py:9-15) | 1 get_ozone_density (:500-518) | 2 get_density
 * (:520-523) | 3 cloud_phase (:262-267) | 4 sample_cloud_density (:195-224) | 5 clouds_shadow_od (:231-260) | 6 get_ray_transmittance
 * (:475-498) | 7 clouds_scattering (:269-349) | 8 / 9 atmospheric_scattering at template depth 0 / 1 (:355-425).  `in` holds n rows of
 * in_stride floats: position, direction, then the function's other arguments (functions 7-9: sun direction, sun colour, cone cosine,
 * dither or step count, index of the row's random stream); `out` n rows of out_stride floats.  trans_lut (f16[256][128][3]) and
 * cloud_ambient (f32[3]), when not NULL, replace what vrt_prepare computed.  Needs sky_res > 0. */
int vrt_sky_probe(vrt_ctx* ctx, int op, int n, const float* in, int in_stride, float* out, int out_stride, const uint16_t* trans_lut,
                  const float* cloud_ambient);
/* Walk single rays on the device (test hook; the sky functions have vrt_sky_probe).  After vrt_prepare, on the context's grid and
 * occupancy pyramid (read from global memory) and in the mode vrt_set_reference_indexing selected.  origin_dir holds n rays of
 * 6 floats -- origin, direction -- in VOXEL units (origin 0..grid_res inside the grid), as VoxelOctreeRaytracer.raytrace takes them
 * (raytracer.py:72; ray_min_t = eps, ray_max_t = inf as at its only call site, pathtracer.py:201-202).  `out` receives 32 bytes a
 * ray: distance f32, cell 3 x i32, normal 3 x f32, DDA steps i32.  mode = walk + 4 * box:
 *   walk 0: the loop of the fused render kernel with the branchy descent | 1: the same loop with the flat descent | 2: the
 *           resumable record the pooled kernel steps (set up, suspended through a slot's packed fields every third step, result);
 *   box  0: nothing is culled | 1: rays are tested against the bounding box of the solid voxels grown by 8 voxels, as the render
 *           launches do (with the reference's indexing they do not, and neither does the probe).
 * A culled ray reports distance inf, cell -1, normal 0 and 0 steps; at grid_res 128 a walk also ends where it leaves the box. */
int vrt_trace_probe(vrt_ctx* ctx, int mode, int n, const float* origin_dir, void* out);
/* Evaluate single shading functions on the device (test hook; the rows the reference's own bsdf.py, math_utils.py, reservoir.py and
 * Renderer.shift were executed on: tests/golden/reference/functions.npz and functions_edges.npz).  After vrt_prepare: the shift reads the
 * context's materials, scene and camera.  `in` holds n rows of in_stride floats, `out` n rows of out_stride floats; integers and bit patterns
 * travel as float bit patterns.  One row per lane.  op (row layouts as oracle/orc_api.cpp's orc_unit_* probes take them):
 *   0  mat 14, v, n, l, form            -> diffuse rgb, specular rgb, pdf (disney_evaluate_split + pdf_disney, bsdf.py:138-172, 383-393)
 *   1  mat 14, v, n, l, lobe, form      -> pdf_disney_lobewise (:365-381)
 *   2  mat 14, v, n, seed, count        -> count x (direction, brdf rgb, pdf, lobe): sample_disney (:395-458), draw i from stream (seed, 0, i, 0)
 *   3  cos_max, n, seed, count          -> count x direction: sample_cone_oriented (math_utils.py:44-59)
 *   4  v -> octahedral code | 5 code -> v | 6 id, albedo -> packed material | 7 packed material -> albedo | 8 x, y, z -> hash3 | 9 x -> uchimura
 *   10 sample 21, M, weight             -> the same 23 floats after a Reservoir's encode -> decode (reservoir.py:104-141)
 *   11 dst_pos, dst_normal, dst_mat 14, src_pos, sample 21, view, dst_M
 *                                       -> diffuse rgb, specular rgb, jacobian of Renderer.shift (pathtracer.py:672-812), then the Jacobian alone
 *                                          as the reuse pass's classify kernel works it out, then 1 / 0: that kernel skips / evaluates the shift.
 *   form: the device code has three formulations of the BSDF -- 0 the render kernels', 1 the reuse pass's, 2 the reuse pass's for a
 *   reconnection vertex -- which must agree bit for bit.  sample = F, rc_pos, rc_normal, rc_incident_dir, rc_incident_L, rc_NEE_dir,
 *   rc_mat_info, cached_jacobian_term, lobes.  count <= 16 and out_stride >= count x the floats of one draw.
 * VRT_E_INVALID: op outside 0..11, a stride smaller than the op's row, NULL pointers, n <= 0; VRT_E_STATE: before vrt_prepare. */
int vrt_shade_probe(vrt_ctx* ctx, int op, int n, const float* in, int in_stride, float* out, int out_stride);
/* Diagnostic builds only (library compiled with -DVRT_DIAG_REGIONS, see tools/diag_regions.py): copy out the
 * 32 x {wave entries, active lanes} counters of the instrumented regions of the render kernel and optionally
 * zero them.  The shipped library returns VRT_E_STATE -- it carries no region counters. */
int vrt_diag_regions(vrt_ctx* ctx, unsigned long long* out64, int reset);

#ifdef __cplusplus
}
#endif
#endif /* VRT_API_H */
