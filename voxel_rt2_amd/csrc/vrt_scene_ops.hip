// vrt_scene_ops.hip -- the calls on a prepared scene: the box edit (vrt_update_voxels), the queries (vrt_cast_rays, vrt_sweep_boxes,
// vrt_trace_radiance, vrt_gather_irradiance, vrt_gather_probes), vrt_fetch_voxels, vrt_distance_field, vrt_label_components and the two triangle edits
// (vrt_voxelize_triangles, vrt_fill_triangles).
// A part of vrt_api.hip's translation unit (#included there behind vrt_pipeline.hip, not compiled by itself), so that everything here
// stays static.  What the calls share is written once: the scratch buffers' growth (grow_scratch), the box argument's checks
// (scene_box), the tail of an edit (finish_edit), the sampled queries' scaffold (sampled_query<Q>) and the triangle edits' (tri_edit<E>).

// A scratch buffer the context keeps and grows on demand: at least `need` bytes behind *p, *bytes what it holds.  (hipFree waits for the
// device: no kernel is still using the old one.)
static int grow_scratch(vrt_ctx* c, uint8_t** p, size_t* bytes, size_t need) {
    if (*bytes >= need) return VRT_OK;
    HIP_TRY(dfree(c, p));
    *bytes = 0;
    HIP_TRY(dmalloc(c, p, need));
    *bytes = need;
    return VRT_OK;
}
// What the eight floats of the culling record (k_cull_box) say to the host: is there anything to cull, is the grid dense.
static void note_cull_record(vrt_ctx* c, const float box[8]) {
    c->cull_active = box[6] != 0.0f;
    // at least half of the 4x4x4 bricks hold a voxel: a dense grid (shadow rays end after a step or two: launch_render_pool)
    c->dense_grid = box[7] >= 0.5f;
    if (c->knobs.dense >= 0) c->dense_grid = c->knobs.dense != 0;   // A/B
}
// The culling record's host side behind an edit, as vrt_prepare reads it behind its own k_cull_box.  One synchronisation: source and
// destination of the copy are on this stack frame.
static int read_cull_record(vrt_ctx* c) {
    float box[8];
    HIP_TRY(hipMemcpyAsync(box, c->d_cull, sizeof(box), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(sync_guarded(c, c->stream));
    note_cull_record(c, box);
    return VRT_OK;
}
// The box argument [lo, hi) of a call on a prepared grid: built, checked against the grid, then the prepared state.  `what`: the entry
// point's name and verb, for the message.  `also`: the message of an argument check of the caller's own that failed (NULL: none did),
// reported where the callers have always reported it -- behind the box, ahead of the state.
static int scene_box(const vrt_ctx* c, const int32_t lo[3], const int32_t hi[3], const char* what, EditBox& box, const char* also = nullptr) {
    for (int a = 0; a < 3; a++) { box.lo[a] = lo[a]; box.hi[a] = hi[a]; }
    if (!edit_box_valid(box, c->cfg.grid_res)) return fail(VRT_E_INVALID, "the box must satisfy 0 <= lo <= hi <= grid_res on every axis");
    if (also) return fail(VRT_E_INVALID, also);
    if (!c->prepared) return fail(VRT_E_STATE, std::string(what) + " a prepared grid: call vrt_prepare first (also after vrt_upload_voxels)");
    return VRT_OK;
}
// The tail of every edit: the box arrays (device memory) into the grid and everything vrt_prepare derives from it (launch_edit), then the
// culling record read back -- whose wait also ends the loan of the caller's host arrays.
static int finish_edit(vrt_ctx* c, const EditBox& box, const int8_t* box_mat, const uint8_t* box_rgb) {
    c->main_dirty = true;
    HIP_TRY(launch_edit(c->stream, c->cfg.grid_res, box, box_mat, box_rgb, c->d_mat, c->d_rgb, c->d_grid, c->d_l0, c->d_l1, c->d_l2, c->d_l3,
                        c->d_l0c, c->d_l0c_base, c->d_cull));
    return read_cull_record(c);
}

extern "C" {

// Replace the voxels of the box [lo, hi) of a prepared context and bring what vrt_prepare derives from the voxels up to date, at the
// box's cost (launch_edit).  Ordered like vrt_upload_voxels: the pending accumulation first, the work on the context's stream --
// behind every render launch queued so far, whose pass is on it -- and main_dirty holds later launches back until it is done.
int vrt_update_voxels(vrt_ctx* c, const int32_t lo[3], const int32_t hi[3], const void* mat, const void* rgb, int on_device) {
    if (!c || !lo || !hi || !mat || !rgb) return fail(VRT_E_INVALID, "null argument");
    if (on_device != 0 && on_device != 1) return fail(VRT_E_INVALID, "on_device must be 0 or 1");
    EditBox box;
    if (const int rc = scene_box(c, lo, hi, "vrt_update_voxels edits", box)) return rc;
    const size_t nv = (size_t)edit_box_voxels(box);
    if (nv == 0) return VRT_OK;
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    const int8_t* box_mat = (const int8_t*)mat;
    const uint8_t* box_rgb = (const uint8_t*)rgb;
    if (!on_device) {
        const size_t rgb_at = (nv + 255) & ~(size_t)255;
        if (grow_scratch(c, &c->d_edit_stage, &c->edit_stage_bytes, rgb_at + 3 * nv) != VRT_OK) return VRT_E_DEVICE;
        c->main_dirty = true;
        HIP_TRY(hipMemcpyAsync(c->d_edit_stage, mat, nv, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->d_edit_stage + rgb_at, rgb, 3 * nv, hipMemcpyHostToDevice, c->stream));
        box_mat = (const int8_t*)c->d_edit_stage;
        box_rgb = c->d_edit_stage + rgb_at;
    }
    return finish_edit(c, box, box_mat, box_rgb);
}
// Move or copy the piece cells of the source box under the map of `mv` (vrt_move.h): snapshot and count on the context's stream, then
// the source box's arrays and the destination box's, each through launch_edit like any other box -- ordered and synchronised as
// vrt_update_voxels, with ONE wait, for the record and the culling record together.  VRT_MOVE_DRY_RUN reads and nothing else: it is
// ordered like vrt_fetch_voxels (no enter(), no flush) and waits for its record alone.  The source box's edit is left out where the
// call vacates nothing (no VRT_MOVE_ERASE_SOURCE): its arrays would be the grid's own bytes.
static_assert(sizeof(vrt_voxel_move) == 120 && sizeof(vrt_move_result) == 48 && sizeof(MoveRecord) == 48, "record sizes of include/vrt_api.h");
static_assert(VRT_MOVE_ERASE_SOURCE == 1 && VRT_MOVE_KEEP_SOLID == 2 && VRT_MOVE_DRY_RUN == 4 && VRT_MOVE_IF_FREE == 8 && VRT_MOVE_FLAGS == 15u, "the flag bits vrt_move.h tests");
static_assert(VRT_MOVE_TILE == 256 * VRT_MOVE_RUN, "k_move_dst: a thread a run");
int vrt_move_voxels(vrt_ctx* c, const vrt_voxel_move* mv, const void* select, int select_on_device, vrt_move_result* result) {
    if (!c || !mv) return fail(VRT_E_INVALID, "null argument");
    if (select_on_device != 0 && select_on_device != 1) return fail(VRT_E_INVALID, "select_on_device must be 0 or 1");
    long long t[3];
    for (int a = 0; a < 3; a++) t[a] = (long long)mv->t[a];
    EditBox src, dst;
    for (int a = 0; a < 3; a++) { dst.lo[a] = mv->dst_lo[a]; dst.hi[a] = mv->dst_hi[a]; }
    const char* const bad = !move_valid(mv->m, t, mv->flags, mv->reserved) ? "m within +-2^20, t within +-2^40, known flag bits and reserved == 0 are required"
                            : !edit_box_valid(dst, c->cfg.grid_res)         ? "the destination box must satisfy 0 <= lo <= hi <= grid_res on every axis"
                                                                            : nullptr;
    if (const int rc = scene_box(c, mv->src_lo, mv->src_hi, "vrt_move_voxels edits", src, bad)) return rc;
    if (result) memset(result, 0, sizeof(*result));
    const size_t n_src = (size_t)edit_box_voxels(src), n_dst = (size_t)edit_box_voxels(dst);
    if (n_src == 0) return VRT_OK;
    const bool dry = (mv->flags & VRT_MOVE_DRY_RUN) != 0u;
    if (dry) HIP_TRY(hipSetDevice(c->device));
    else if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    const MovePlan p = move_plan(src, dst, mv->m, t, mv->select_value, mv->flags, c->cfg.grid_res);
    const bool staged = select != nullptr && !select_on_device;
    const MoveLayout l = move_layout(n_src, n_dst, staged);
    if (grow_scratch(c, &c->d_move, &c->move_bytes, l.bytes) != VRT_OK) return VRT_E_DEVICE;
    uint32_t* const snap = (uint32_t*)c->d_move;
    int8_t* const box_mat = (int8_t*)(c->d_move + l.mat_at);
    uint8_t* const box_rgb = c->d_move + l.rgb_at;
    MoveRecord* const rec = (MoveRecord*)(c->d_move + l.record_at);
    const int* d_select = (const int*)select;
    if (!dry) c->main_dirty = true;
    if (staged) {
        HIP_TRY(hipMemcpyAsync(c->d_move + l.select_at, select, 4 * n_src, hipMemcpyHostToDevice, c->stream));
        d_select = (const int*)(c->d_move + l.select_at);
    }
    HIP_TRY(launch_move_count(c->stream, p, c->d_mat, c->d_rgb, d_select, snap, rec));
    MoveRecord r;   // (on this stack frame: the one wait below covers the copy)
    HIP_TRY(hipMemcpyAsync(&r, rec, sizeof(r), hipMemcpyDeviceToHost, c->stream));
    if (dry) HIP_TRY(sync_stream_only(c, c->stream));   // (also ends the loan of the host selection)
    else {
        const EditBox* const boxes[2] = {(mv->flags & VRT_MOVE_ERASE_SOURCE) ? &src : nullptr, n_dst ? &dst : nullptr};
        for (int k = 0; k < 2; k++) {   // source box first; the arrays are shared: stream order lets the second box reuse them
            if (!boxes[k]) continue;
            if (k == 0) HIP_TRY(launch_move_src_arrays(c->stream, p, c->d_mat, c->d_rgb, snap, box_mat, box_rgb, rec));
            else HIP_TRY(launch_move_dst_arrays(c->stream, p, c->d_mat, c->d_rgb, snap, box_mat, box_rgb, rec));
            HIP_TRY(launch_edit(c->stream, c->cfg.grid_res, *boxes[k], box_mat, box_rgb, c->d_mat, c->d_rgb, c->d_grid, c->d_l0, c->d_l1, c->d_l2, c->d_l3, c->d_l0c,
                                c->d_l0c_base, c->d_cull));
        }
        if (const int rc = read_cull_record(c)) return rc;
    }
    if (result) {
        long long written, blocked, erased;
        move_result(mv->flags, r, result->lo, result->hi, written, blocked, erased);
        result->written = written; result->blocked = blocked; result->erased = erased;
    }
    return VRT_OK;
}
// ---- asking the scene: vrt_cast_rays, vrt_trace_radiance, vrt_gather_irradiance, vrt_gather_probes, vrt_fetch_voxels ------------------------------
// All READ scene data (pyramid, texels, stored voxels), on the context's stream: behind every edit queued so far, ahead of every
// later one.  Render launches read the same data on their own streams and nothing here writes what they or their passes touch, so
// neither main_dirty nor the pending accumulation is concerned: no enter(), no flush.
extern "C++" {   // (templates below)
// What every query reads.  Of the frame parameters: the floor (floor_height, floor_color, floor_material) and voxel_edges; the sampled
// queries also the background, the light (light_dir, light_color, light_cos_max, light_weight), the sky switch (use_sky), max_depth and
// the seed.  Of the scene: the pyramid, the texels and the culling box; the sampled queries also the materials and the sky tables.
// Nothing else: not the camera (matrices, camera_pos, taa_jitter, camera_is_moving, render_scale, max_accum_frames), not the pixel grid
// (W, H, inv_res, row0 / row1, the stripe fields), not exposure, not the frame counter -- the host emulation hands the same functions a
// record with exactly the listed fields set and every other field poisoned, and gets the same bytes (tests/emul/query_emul.h), and the
// device answers the oracle's records from contexts in every frame state (tests/test_gpu_query_states.py).
struct QueryInputs { FrameParams fp; SceneData sc; };
static QueryInputs query_inputs(vrt_ctx* c) {
    QueryInputs q{make_frame_params(c), make_scene_data(c)};
    // the scene's box, whatever the render launches count: culled rays are misses either way (cast_row); not with the reference's
    // indexing, where a ray clear of every solid voxel can still "hit" outside the grid (plan_render_variant)
    q.sc.cull = c->d_cull + (c->cull_active && !c->ref_oob && c->knobs.cull != 0 ? 0 : 8);
    return q;
}
// A query's host path: the caller's n records, `block` at a time, copied to the staging buffer, worked on by queue(m, d_in, d_out) --
// which queues on the context's stream -- and copied back; then the wait.
template <class In, class Out, class Queue>
static int staged_query(vrt_ctx* c, long long n, long long block, const In* in, Out* out, Queue queue) {
    if (grow_scratch(c, &c->d_cast_stage, &c->cast_stage_bytes, (size_t)block * (sizeof(In) + sizeof(Out))) != VRT_OK) return VRT_E_DEVICE;
    In* d_in = (In*)c->d_cast_stage;
    Out* d_out = (Out*)(c->d_cast_stage + (size_t)block * sizeof(In));
    for (long long at = 0; at < n; at += block) {   // (stream order lets block k + 1 reuse what block k's copy back has read)
        const long long m = std::min(block, n - at);
        HIP_TRY(hipMemcpyAsync(d_in, in + at, (size_t)m * sizeof(In), hipMemcpyHostToDevice, c->stream));
        if (queue(m, (const In*)d_in, d_out) != VRT_OK) return VRT_E_DEVICE;
        HIP_TRY(hipMemcpyAsync(out + at, d_out, (size_t)m * sizeof(Out), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(sync_stream_only(c, c->stream));   // (also ends the loan of the host arrays)
    return VRT_OK;
}
// The scratch plane of vrt_trace_radiance, vrt_gather_irradiance and vrt_gather_probes: a work counter (256 bytes) and VRT_RADIANCE_ITEMS
// item values of the first, VRT_SENSOR_ITEMS records of the second or VRT_PROBE_ITEMS items of the third -- the same bytes; all run on the
// context's stream, whose order lets them share it.
static_assert((size_t)VRT_SENSOR_ITEMS * sizeof(vrt_irradiance) <= (size_t)VRT_RADIANCE_ITEMS * sizeof(f3), "the sensor plane must fit the radiance plane");
static_assert(sizeof(vrt_irradiance) == VRT_SENSOR_ITEM_BYTES && sizeof(vrt_sensor) == 32, "record sizes of include/vrt_api.h");
static_assert((size_t)VRT_PROBE_ITEMS * sizeof(ProbeItem) <= (size_t)VRT_RADIANCE_ITEMS * sizeof(f3), "the probe plane must fit the radiance plane");
static_assert(sizeof(ProbeItem) == VRT_PROBE_ITEM_BYTES && sizeof(vrt_probe) == 16 && sizeof(vrt_sh_probe) == 128, "record sizes of include/vrt_api.h");
static_assert(VRT_PROBE_ITEMS >= (1 << 18), "one sample of a full block (plan_query_rays) must fit the probe plane");
// A sampled query (vrt_query.h) reads what vrt_cast_rays reads plus the materials and the sky tables, and is ordered the same way.
// Blocks of records (plan_query_rays), a block's samples in chunks of whole samples (plan_query_chunk): one item launch and one fold
// launch a chunk, all on the context's stream, where stream order lets every chunk reuse the scratch plane.  name, noun: the entry
// point's, for its messages.
template <class Q>
static int sampled_query(vrt_ctx* c, const char* name, const char* noun, int64_t n, const typename Q::In* in, int n_samples, uint32_t first_frame,
                         typename Q::Out* out, int on_device) {
    if (!c || !in || !out) return fail(VRT_E_INVALID, "null argument");
    if (n < 0) return fail(VRT_E_INVALID, "n must not be negative");
    if (n_samples < 1 || n_samples > VRT_RADIANCE_MAX_SAMPLES) return fail(VRT_E_INVALID, "n_samples must be 1 .. VRT_RADIANCE_MAX_SAMPLES");
    if (on_device != 0 && on_device != 1) return fail(VRT_E_INVALID, "on_device must be 0 or 1");
    if (!c->prepared) return fail(VRT_E_STATE, std::string(name) + " asks a prepared scene: call vrt_prepare first (also after vrt_upload_voxels)");
    if (n == 0) return VRT_OK;
    if constexpr (Q::has_reserved)
        if (!on_device)
            for (int64_t k = 0; k < n; k++) if (in[k].reserved != 0u) return fail(VRT_E_INVALID, std::string("a ") + noun + "'s `reserved` field must be 0");
    HIP_TRY(hipSetDevice(c->device));
    const QueryInputs q = query_inputs(c);
    if (!c->d_radiance_plane) HIP_TRY(dmalloc(c, &c->d_radiance_plane, 256 + (size_t)VRT_RADIANCE_ITEMS * sizeof(f3)));   // [0]: the work counter
    auto queue = [&](long long m, const typename Q::In* d_in, typename Q::Out* d_out) -> int {
        const int per = plan_query_chunk(Q::max_items, m, n_samples);
        for (int s0 = 0; s0 < n_samples; s0 += per) {
            const int count = std::min(per, n_samples - s0);
            const bool staged = plan_cast_staged(m * count, c->knobs.cast_view);   // on the items of THIS launch: a short last chunk chooses for itself
            HIP_TRY(launch_sampled_query<Q>(c->stream, c->cfg.grid_res, staged, c->ref_oob, c->n_cu, q.fp, q.sc, m, s0, count, n_samples, first_frame, d_in,
                                            (typename Q::Item*)(c->d_radiance_plane + 256), d_out, (unsigned*)c->d_radiance_plane));
        }
        return VRT_OK;
    };
    const long long block = plan_query_rays((long long)n);
    if (!on_device) return staged_query(c, (long long)n, block, in, out, queue);
    for (long long at = 0; at < (long long)n; at += block)
        if (queue(std::min(block, (long long)n - at), in + at, out + at) != VRT_OK) return VRT_E_DEVICE;
    return VRT_OK;
}
}  // extern "C++"
int vrt_cast_rays(vrt_ctx* c, int64_t n, const vrt_ray* rays, vrt_ray_hit* hits, int on_device) {
    if (!c || !rays || !hits) return fail(VRT_E_INVALID, "null argument");
    if (n < 0) return fail(VRT_E_INVALID, "n must not be negative");
    if (on_device != 0 && on_device != 1) return fail(VRT_E_INVALID, "on_device must be 0 or 1");
    if (!c->prepared) return fail(VRT_E_STATE, "vrt_cast_rays asks a prepared scene: call vrt_prepare first (also after vrt_upload_voxels)");
    if (n == 0) return VRT_OK;
    HIP_TRY(hipSetDevice(c->device));
    const QueryInputs q = query_inputs(c);
    const bool staged = plan_cast_staged((long long)n, c->knobs.cast_view);   // on the whole batch, however the host path cuts it
    auto queue = [&](long long m, const vrt_ray* d_rays, vrt_ray_hit* d_hits) -> int {
        HIP_TRY(launch_cast_rays(c->stream, c->cfg.grid_res, staged, c->ref_oob, c->n_cu, q.fp, q.sc, m, d_rays, d_hits));
        return VRT_OK;
    };
    if (on_device) return queue((long long)n, rays, hits);
    return staged_query(c, (long long)n, std::min<long long>(plan_cast_chunk(), (long long)n), rays, hits, queue);
}
static_assert(sizeof(vrt_box_sweep) == 48 && sizeof(vrt_sweep_hit) == 32, "record sizes of include/vrt_api.h");
int vrt_sweep_boxes(vrt_ctx* c, int64_t n, const vrt_box_sweep* boxes, vrt_sweep_hit* hits, int on_device) {
    if (!c || !boxes || !hits) return fail(VRT_E_INVALID, "null argument");
    if (n < 0) return fail(VRT_E_INVALID, "n must not be negative");
    if (on_device != 0 && on_device != 1) return fail(VRT_E_INVALID, "on_device must be 0 or 1");
    if (!c->prepared) return fail(VRT_E_STATE, "vrt_sweep_boxes asks a prepared scene: call vrt_prepare first (also after vrt_upload_voxels)");
    if (n == 0) return VRT_OK;
    if (!on_device)
        for (int64_t k = 0; k < n; k++) if (boxes[k].reserved != 0u) return fail(VRT_E_INVALID, "a box's `reserved` field must be 0");
    HIP_TRY(hipSetDevice(c->device));
    QueryInputs q = query_inputs(c);
    // the scene's box in either indexing mode: only cells inside the grid exist for a sweep, so no box "meets" anything outside it
    q.sc.cull = c->d_cull + (c->knobs.cull != 0 ? 0 : 8);
    auto queue = [&](long long m, const vrt_box_sweep* d_boxes, vrt_sweep_hit* d_hits) -> int {
        HIP_TRY(launch_sweep_boxes(c->stream, c->cfg.grid_res, c->n_cu, q.fp.floor_height, q.sc, m, d_boxes, d_hits));
        return VRT_OK;
    };
    if (on_device) return queue((long long)n, boxes, hits);
    return staged_query(c, (long long)n, std::min<long long>(plan_sweep_chunk(), (long long)n), boxes, hits, queue);
}
int vrt_trace_radiance(vrt_ctx* c, int64_t n, const vrt_path_ray* rays, int n_samples, uint32_t first_frame, vrt_radiance* out, int on_device) {
    return sampled_query<RadianceQuery>(c, "vrt_trace_radiance", "ray", n, rays, n_samples, first_frame, out, on_device);
}
int vrt_gather_irradiance(vrt_ctx* c, int64_t n, const vrt_sensor* sensors, int n_samples, uint32_t first_frame, vrt_irradiance* out, int on_device) {
    return sampled_query<SensorQuery>(c, "vrt_gather_irradiance", "sensor", n, sensors, n_samples, first_frame, out, on_device);
}
int vrt_gather_probes(vrt_ctx* c, int64_t n, const vrt_probe* probes, int n_samples, uint32_t first_frame, vrt_sh_probe* out, int on_device) {
    return sampled_query<ProbeQuery>(c, "vrt_gather_probes", "probe", n, probes, n_samples, first_frame, out, on_device);
}
int vrt_fetch_voxels(vrt_ctx* c, const int32_t lo[3], const int32_t hi[3], void* mat, void* rgb, int on_device) {
    if (!c || !lo || !hi || !mat || !rgb) return fail(VRT_E_INVALID, "null argument");
    if (on_device != 0 && on_device != 1) return fail(VRT_E_INVALID, "on_device must be 0 or 1");
    EditBox box;
    if (const int rc = scene_box(c, lo, hi, "vrt_fetch_voxels reads", box)) return rc;
    const size_t nv = (size_t)edit_box_voxels(box);
    if (nv == 0) return VRT_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (on_device) {
        HIP_TRY(launch_fetch_voxels(c->stream, c->cfg.grid_res, box, c->d_mat, c->d_rgb, (int8_t*)mat, (uint8_t*)rgb));
        return VRT_OK;
    }
    const size_t rgb_at = (nv + 255) & ~(size_t)255;
    if (grow_scratch(c, &c->d_cast_stage, &c->cast_stage_bytes, rgb_at + 3 * nv) != VRT_OK) return VRT_E_DEVICE;
    HIP_TRY(launch_fetch_voxels(c->stream, c->cfg.grid_res, box, c->d_mat, c->d_rgb, (int8_t*)c->d_cast_stage, c->d_cast_stage + rgb_at));
    HIP_TRY(hipMemcpyAsync(mat, c->d_cast_stage, nv, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(rgb, c->d_cast_stage + rgb_at, 3 * nv, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(sync_stream_only(c, c->stream));
    return VRT_OK;
}
// The distance field of the stored voxels over the box [lo, hi) (vrt_distance.h): three line passes on the context's stream, reading
// d_mat as vrt_fetch_voxels does -- so the same ordering, no enter(), no flush.  The scratch is the call's own buffer: every call runs
// on the context's stream, where stream order lets the next call reuse it, and the host path's copies out of it are waited for here.
int vrt_distance_field(vrt_ctx* c, const int32_t lo[3], const int32_t hi[3], int32_t max_d2, uint32_t flags, void* d2, void* nearest, int on_device) {
    if (!c || !lo || !hi || !d2) return fail(VRT_E_INVALID, "null argument");
    if (on_device != 0 && on_device != 1) return fail(VRT_E_INVALID, "on_device must be 0 or 1");
    const char* const bad = max_d2 < 0 || max_d2 > VRT_DIST_MAX_D2 ? "max_d2 must be 0 .. VRT_DIST_MAX_D2" : (flags & ~(uint32_t)VRT_DIST_TO_EMPTY) != 0u ? "unknown flag bits" : nullptr;
    EditBox box;
    if (const int rc = scene_box(c, lo, hi, "vrt_distance_field reads", box, bad)) return rc;
    const size_t nv = (size_t)edit_box_voxels(box);
    if (nv == 0) return VRT_OK;
    HIP_TRY(hipSetDevice(c->device));
    const DistBox p = dist_plan_box(box, c->cfg.grid_res, max_d2, flags);
    const DistLayout l = plan_distance_layout((size_t)dist_len(p.grown, 0), (size_t)dist_len(p.grown, 1), (size_t)dist_len(box, 0), (size_t)dist_len(box, 1),
                                              (size_t)dist_len(box, 2), nearest != nullptr, !on_device);
    if (grow_scratch(c, &c->d_dist, &c->dist_bytes, l.bytes) != VRT_OK) return VRT_E_DEVICE;
    const DistScratch s{(int*)(c->d_dist + l.a_at), (int*)(c->d_dist + l.b_at), c->d_dist + l.cz_at, c->d_dist + l.cy_at};
    if (on_device) {
        HIP_TRY(launch_distance_field(c->stream, c->cfg.grid_res, p, c->d_mat, s, (int*)d2, (int*)nearest));
        return VRT_OK;
    }
    int* d_d2 = (int*)(c->d_dist + l.d2_at);
    int* d_nearest = nearest ? (int*)(c->d_dist + l.nearest_at) : nullptr;
    HIP_TRY(launch_distance_field(c->stream, c->cfg.grid_res, p, c->d_mat, s, d_d2, d_nearest));
    HIP_TRY(hipMemcpyAsync(d2, d_d2, 4 * nv, hipMemcpyDeviceToHost, c->stream));
    if (nearest) HIP_TRY(hipMemcpyAsync(nearest, d_nearest, 4 * nv, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(sync_stream_only(c, c->stream));
    return VRT_OK;
}
// The connected components of the box's members (vrt_label.h): three launches on the context's stream, reading d_mat as
// vrt_distance_field does -- so the same ordering, no enter(), no flush.  The union-find works in the labels themselves; the context's
// own buffer holds the counter words the last launch adds to and, on the host path, the staged labels (plan_label_layout).  Stream order
// lets the next call reuse it; the host path's copies out of it are waited for here, the device path's copy of the record is queued.
static_assert(sizeof(vrt_label_result) == 16, "record size of include/vrt_api.h");
int vrt_label_components(vrt_ctx* c, const int32_t lo[3], const int32_t hi[3], uint32_t flags, void* labels, vrt_label_result* result, int on_device) {
    if (!c || !lo || !hi || !labels) return fail(VRT_E_INVALID, "null argument");
    if (on_device != 0 && on_device != 1) return fail(VRT_E_INVALID, "on_device must be 0 or 1");
    const uint32_t both = VRT_LABEL_CONN_18 | VRT_LABEL_CONN_26;
    const char* const bad = (flags & ~(uint32_t)(VRT_LABEL_EMPTY | both)) != 0u ? "unknown flag bits" : (flags & both) == both ? "VRT_LABEL_CONN_18 and VRT_LABEL_CONN_26 exclude one another" : nullptr;
    EditBox box;
    if (const int rc = scene_box(c, lo, hi, "vrt_label_components reads", box, bad)) return rc;
    const size_t nv = (size_t)edit_box_voxels(box);
    if (nv == 0) {   // no label to write; the record is zeroed where it lives
        if (result && !on_device) memset(result, 0, sizeof(*result));
        if (result && on_device) {
            HIP_TRY(hipSetDevice(c->device));
            HIP_TRY(hipMemsetAsync(result, 0, sizeof(*result), c->stream));
        }
        return VRT_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    const LabelBox p = label_plan_box(box, c->cfg.grid_res, flags);
    const LabelLayout l = plan_label_layout(nv, !on_device);
    if (grow_scratch(c, &c->d_label, &c->label_bytes, l.bytes) != VRT_OK) return VRT_E_DEVICE;
    vrt_label_result* const counters = (vrt_label_result*)(c->d_label + l.result_at);
    if (on_device) {
        HIP_TRY(launch_label_components(c->stream, p, c->d_mat, (int*)labels, counters));
        if (result) HIP_TRY(hipMemcpyAsync(result, counters, sizeof(*result), hipMemcpyDeviceToDevice, c->stream));
        return VRT_OK;
    }
    int* const d_labels = (int*)(c->d_label + l.labels_at);
    HIP_TRY(launch_label_components(c->stream, p, c->d_mat, d_labels, counters));
    HIP_TRY(hipMemcpyAsync(labels, d_labels, 4 * nv, hipMemcpyDeviceToHost, c->stream));
    vrt_label_result r;   // (on this stack frame: the wait below covers it)
    if (result) HIP_TRY(hipMemcpyAsync(&r, counters, sizeof(r), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(sync_stream_only(c, c->stream));
    if (result) *result = r;
    return VRT_OK;
}
// ---- editing the scene with triangles: vrt_voxelize_triangles, vrt_fill_triangles ---------------------------------------------------------
// Both turn the caller's triangles into box arrays on the device and hand those to finish_edit like any other box -- ordered and
// synchronised exactly as vrt_update_voxels.  Batch by batch a raster pass writes the head region of the context's scratch (d_vox, cut up
// by plan_tri_layout), a resolve pass turns that into the box arrays.  The host path stages plan_voxelize_chunk() triangles at a time in
// the query staging buffer; the device path works on the caller's array, plan_voxelize_batch() triangles a batch.
static_assert(sizeof(vrt_triangle) == 48 && sizeof(vrt_voxelize_result) == 40 && sizeof(VoxResult) == 40 && sizeof(VoxEntry) == 16, "record sizes of include/vrt_api.h");
extern "C++" {   // (a template below)
// What a triangle edit E supplies (tri_edit<E>): `what`, the entry point's name and verb for its messages; head_bytes, the size of its head
// region; batch, its set-up and raster launches over m staged or caller-owned triangles numbered from `at`; resolve, its resolve launch;
// resolves_chunks, whether the host path resolves after every chunk, while the chunk's triangles are still staged.
// vrt_voxelize_triangles (vrt_voxelize.h): ownership of the box's voxels, one word each, is settled batch by batch
// (launch_voxelize_batch) and resolved into box arrays (launch_voxelize_resolve) -- on the host path chunk by chunk, since an owner's
// payload is read from its triangle; the device path resolves once, over the caller's array.
struct VoxelizeEdit {
    static constexpr const char* what = "vrt_voxelize_triangles edits";
    static constexpr bool resolves_chunks = true;
    static size_t head_bytes(const EditBox&, size_t nv) { return 4 * nv; }
    int batch(vrt_ctx* c, const EditBox& box, long long at, long long m, const vrt_triangle* d_tris, const TriScratch& s) const {
        HIP_TRY(launch_voxelize_batch(c->stream, c->cfg.grid_res, c->n_cu, box, (unsigned long long)at, m, d_tris, s));
        return VRT_OK;
    }
    int resolve(vrt_ctx* c, const EditBox& box, long long base, const vrt_triangle* d_tris, bool final, const TriScratch& s) const {
        HIP_TRY(launch_voxelize_resolve(c->stream, c->cfg.grid_res, box, (unsigned long long)base, d_tris, final, c->d_mat, c->d_rgb, s));
        return VRT_OK;
    }
};
// vrt_fill_triangles (vrt_fill.h): every batch toggles one bit per owned column in a bitmap of the box (launch_fill_batch), one resolve
// turns the bitmap into box arrays of `voxel` (launch_fill_resolve).  XOR commutes, so the host path's chunks need no resolve of their
// own: they are staged one after the other and toggle into the same bitmap, and the one resolve reads no triangle.
struct FillEdit {
    uint32_t voxel;
    static constexpr const char* what = "vrt_fill_triangles edits";
    static constexpr bool resolves_chunks = false;
    static size_t head_bytes(const EditBox& box, size_t) { return 4 * (size_t)fill_words(box); }
    int batch(vrt_ctx* c, const EditBox& box, long long, long long m, const vrt_triangle* d_tris, const TriScratch& s) const {
        HIP_TRY(launch_fill_batch(c->stream, c->cfg.grid_res, c->n_cu, box, m, d_tris, s));
        return VRT_OK;
    }
    int resolve(vrt_ctx* c, const EditBox& box, long long, const vrt_triangle*, bool, const TriScratch& s) const {
        HIP_TRY(launch_fill_resolve(c->stream, c->cfg.grid_res, box, voxel, c->d_mat, c->d_rgb, s));
        return VRT_OK;
    }
};
template <class E>
static int tri_edit(vrt_ctx* c, const E& e, int64_t n, const vrt_triangle* tris, const int32_t lo[3], const int32_t hi[3], vrt_voxelize_result* result, int on_device) {
    if (!c || !tris || !lo || !hi) return fail(VRT_E_INVALID, "null argument");
    if (n < 0 || n >= 4294967295LL) return fail(VRT_E_INVALID, "n must be 0 .. 2^32 - 2");
    if (on_device != 0 && on_device != 1) return fail(VRT_E_INVALID, "on_device must be 0 or 1");
    EditBox box;
    if (const int rc = scene_box(c, lo, hi, E::what, box)) return rc;
    if (!on_device)
        for (int64_t k = 0; k < n; k++) if (tris[k].reserved0 != 0u || tris[k].reserved1 != 0u) return fail(VRT_E_INVALID, "a triangle's reserved words must be 0");
    if (result) memset(result, 0, sizeof(*result));
    const size_t nv = (size_t)edit_box_voxels(box);
    if (nv == 0 || n == 0) return VRT_OK;
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    const long long batch = std::min<long long>((long long)n, on_device ? plan_voxelize_batch() : plan_voxelize_chunk());
    const size_t head_bytes = E::head_bytes(box, nv);
    const TriLayout l = plan_tri_layout(head_bytes, nv, (size_t)batch);
    if (grow_scratch(c, &c->d_vox, &c->vox_bytes, l.bytes) != VRT_OK) return VRT_E_DEVICE;
    unsigned long long* const heads = (unsigned long long*)(c->d_vox + l.heads_at);
    const TriScratch s{(uint32_t*)c->d_vox, (int8_t*)(c->d_vox + l.mat_at), c->d_vox + l.rgb_at, (VoxEntry*)(c->d_vox + l.entries_at), heads, (VoxResult*)(heads + 8)};
    if (!on_device && grow_scratch(c, &c->d_cast_stage, &c->cast_stage_bytes, (size_t)batch * sizeof(vrt_triangle)) != VRT_OK) return VRT_E_DEVICE;
    c->main_dirty = true;
    HIP_TRY(launch_tri_begin(c->stream, head_bytes, s));
    for (long long at = 0; at < (long long)n; at += batch) {   // (stream order lets batch k + 1 reuse what batch k has read)
        const long long m = std::min(batch, (long long)n - at);
        const vrt_triangle* d_tris = tris + at;
        if (!on_device) {
            HIP_TRY(hipMemcpyAsync(c->d_cast_stage, tris + at, (size_t)m * sizeof(vrt_triangle), hipMemcpyHostToDevice, c->stream));
            d_tris = (const vrt_triangle*)c->d_cast_stage;
        }
        if (e.batch(c, box, at, m, d_tris, s) != VRT_OK) return VRT_E_DEVICE;
        if (!on_device && E::resolves_chunks && e.resolve(c, box, at, d_tris, at + m >= (long long)n, s) != VRT_OK) return VRT_E_DEVICE;
    }
    if ((on_device || !E::resolves_chunks) && e.resolve(c, box, 0, tris, true, s) != VRT_OK) return VRT_E_DEVICE;
    VoxResult r;   // (the resolve's record, final here; finish_edit's one synchronisation waits for the copy)
    if (result) HIP_TRY(hipMemcpyAsync(&r, s.res, sizeof(r), hipMemcpyDeviceToHost, c->stream));
    const int rc = finish_edit(c, box, s.box_mat, s.box_rgb);   // (the wait also ends the loan of the host array)
    if (rc == VRT_OK && result) {
        result->voxels = (int64_t)r.voxels;
        result->invalid = (int64_t)r.invalid;
        if (r.voxels != 0ULL) for (int a = 0; a < 3; a++) { result->lo[a] = r.lo[a]; result->hi[a] = r.hi[a] + 1; }
    }
    return rc;
}
}  // extern "C++"
int vrt_voxelize_triangles(vrt_ctx* c, int64_t n, const vrt_triangle* tris, const int32_t lo[3], const int32_t hi[3], vrt_voxelize_result* result, int on_device) {
    return tri_edit(c, VoxelizeEdit{}, n, tris, lo, hi, result, on_device);
}
int vrt_fill_triangles(vrt_ctx* c, int64_t n, const vrt_triangle* tris, const int32_t lo[3], const int32_t hi[3], uint32_t voxel, vrt_voxelize_result* result,
                       int on_device) {
    return tri_edit(c, FillEdit{voxel}, n, tris, lo, hi, result, on_device);
}

}  // extern "C"
