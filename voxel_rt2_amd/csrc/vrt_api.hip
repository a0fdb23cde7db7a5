// vrt_api.hip -- the C ABI of include/vrt_api.h: context creation and teardown, uploads, the sky entry points, the fetches, the probes,
// the stats.
// (The context itself: vrt_ctx.h.  vrt_accumulate and everything that sequences launches: vrt_pipeline.hip; the calls on a prepared scene --
// the box edit, the queries, vrt_fetch_voxels, the distance field, the triangle edits: vrt_scene_ops.hip.  Both #included below.)
//
// Replaces the host side of the reference's Renderer (renderer/pathtracer.py:28-136 field
// allocation, 139-150 / 246-287 setters, 314-329 prepare + sky steps, 664-668 reset, 1310-1323
// accumulate / fetch_image).  One context = one HIP device, one stream; all per-pixel buffers
// cover the context's rows plus a halo (row-tile sharding across GPUs renders the halo rows
// redundantly instead of exchanging them: per-pixel random streams make them bit-identical).
#include "vrt_ctx.h"
#include "vrt_probe.h"
#include "vrt_shade_probe.h"

// The row ranges this context produces: one, or with vrt_set_row_stripes its stripes.
static std::vector<std::pair<int, int>> owned_ranges(const vrt_ctx* c) {
    std::vector<std::pair<int, int>> r;
    if (c->stripe_rows == 0) { r.emplace_back(c->own0, c->own1); return r; }
    const int period = c->stripe_rows * c->stripe_parts;
    for (int s0 = c->stripe_part * c->stripe_rows; s0 < c->cfg.height; s0 += period)
        r.emplace_back(s0, s0 + c->stripe_rows < c->cfg.height ? s0 + c->stripe_rows : c->cfg.height);
    return r;
}
static size_t owned_rows(const vrt_ctx* c) {
    size_t n = 0;
    for (const auto& r : owned_ranges(c)) n += (size_t)(r.second - r.first);
    return n;
}
static FrameParams make_frame_params(const vrt_ctx* c) {
    FrameParams fp;
    memset(&fp, 0, sizeof(fp));
    memcpy(fp.view.m, c->cam.view, 64);
    memcpy(fp.proj.m, c->cam.proj, 64);
    memcpy(fp.view_inv.m, c->cam.view_inv, 64);
    memcpy(fp.proj_inv.m, c->cam.proj_inv, 64);
    fp.camera_pos = mk3(c->cam.pos[0], c->cam.pos[1], c->cam.pos[2]);
    const int W = c->cfg.width, H = c->cfg.height;
    fp.inv_res = mk2((float)(1.0 / (double)W), (float)(1.0 / (double)H));
    // TAA jitter: two draws of random stream 3 per set_proj_mat call (pathtracer.py:264-265)
    dm_rng rng = dm_rng_init(c->cfg.seed, c->cam.jitter_index, 0u, 3u);
    float r0 = dm_rng_f32(&rng), r1 = dm_rng_f32(&rng);
    fp.taa_jitter = mk2((r0 * 2.0f - 1.0f) * fp.inv_res.x, (r1 * 2.0f - 1.0f) * fp.inv_res.y);
    fp.W = W; fp.H = H;
    fp.row0 = c->buf0; fp.row1 = c->buf1;
    fp.camera_is_moving = c->cam.camera_is_moving;
    fp.render_scale = c->cam.render_scale;
    fp.max_accum_frames = c->cam.max_accum_frames;
    fp.light_dir = mk3(c->scene.light_direction[0], c->scene.light_direction[1], c->scene.light_direction[2]);
    fp.light_color = mk3(c->scene.light_color[0], c->scene.light_color[1], c->scene.light_color[2]);
    fp.light_cos_max = c->scene.light_cos_theta_max;
    fp.light_weight = c->scene.light_weight;
    fp.light_cone_pdf = cone_pdf_inside(fp.light_cos_max);
    fp.floor_height = c->scene.floor_height;
    fp.floor_color = mk3(c->scene.floor_color[0], c->scene.floor_color[1], c->scene.floor_color[2]);
    fp.floor_material = c->scene.floor_material;
    fp.background = mk3(c->scene.background_color[0], c->scene.background_color[1], c->scene.background_color[2]);
    fp.use_sky = c->scene.use_physical_sky;
    fp.voxel_edges = c->cfg.voxel_edges;
    fp.exposure = c->cfg.exposure;
    fp.max_depth = c->cfg.max_depth;
    fp.seed = c->cfg.seed;
    fp.frame = c->frame;
    if (c->stripe_rows) {
        fp.stripe_rows = c->stripe_rows;
        fp.stripe_period = c->stripe_rows * c->stripe_parts;
        fp.stripe_first = c->stripe_part * c->stripe_rows;
        fp.stripe_tile_rows = (int)owned_ranges(c).size() * (c->stripe_rows / 8 + 2);
    }
    return fp;
}
// What plan_render_variant (vrt_plan.h) decides on, as the context stands, for a launch of `fused` samples.
static RenderInputs render_inputs(const vrt_ctx* c, int fused) {
    const float* lc = c->scene.light_color;
    const bool emits = (lc[0] != 0.0f || lc[1] != 0.0f || lc[2] != 0.0f) && c->scene.light_weight != 0.0f;
    return RenderInputs{c->cfg.width, c->cfg.height, c->cfg.max_depth, c->knobs.render, c->knobs.cull, c->cfg.use_restir != 0,
                        c->instrumented, c->count_as_timed, c->ref_oob, c->cull_active, c->dense_grid, emits, fused};
}
static RenderVariant render_variant(const vrt_ctx* c, int fused) { return plan_render_variant(render_inputs(c, fused)); }
static SceneData make_scene_data(const vrt_ctx* c) {
    SceneData sc;
    sc.pyr.l0 = c->d_l0; sc.pyr.l1 = c->d_l1; sc.pyr.l2 = c->d_l2; sc.pyr.l3 = c->d_l3;
    sc.pyr.l0c = c->d_l0c; sc.pyr.l0c_base = c->d_l0c_base; sc.pyr.l0c_count = c->d_l0c_base + 512;
    sc.pyr.ref_oob = c->ref_oob ? 1 : 0;
    sc.grid = c->d_grid;
    sc.mats = c->d_mats;
    sc.mats_x = c->d_mats_x;
    sc.sky.scattering = c->d_sky_scat;
    sc.sky.transmittance = c->d_sky_trans;
    sc.sky.res = c->cfg.sky_res;
    sc.sky.fres = c->cfg.sky_res > 0 ? (float)(1.0 / (double)c->cfg.sky_res) : 0.0f;
    sc.counters = c->d_counters;
    sc.cull = c->d_cull + (render_variant(c, 1).cull ? 0 : 8);   // (cull does not depend on the fused count)
    return sc;
}
static SkyPrecompute make_sky(const vrt_ctx* c) {
    SkyPrecompute sp;
    sp.scattering = c->d_sky_scat; sp.transmittance = c->d_sky_trans; sp.trans_lut = c->d_trans_lut;
    sp.cloud_tex = c->d_cloud_tex; sp.cloud_ambient = c->d_cloud_ambient;
    sp.res = c->cfg.sky_res;
    sp.fres = (float)(1.0 / (double)c->cfg.sky_res);
    sp.use_clouds = c->scene.use_clouds;
    sp.seed = c->cfg.seed;
    return sp;
}
static void sun_of(const vrt_ctx* c, f3& dir, f3& col, float& cosm) {
    dir = mk3(c->scene.light_direction[0], c->scene.light_direction[1], c->scene.light_direction[2]);
    col = mk3(c->scene.light_color[0], c->scene.light_color[1], c->scene.light_color[2]) * c->scene.light_weight;
    cosm = c->scene.light_cos_theta_max;
}

#include "vrt_pipeline.hip"
#include "vrt_scene_ops.hip"

extern "C" {

const char* vrt_last_error(void) { return g_err.c_str(); }
#ifndef VRT_BUILD_ID
#define VRT_BUILD_ID "unknown"
#endif
const char* vrt_build_id(void) { return VRT_BUILD_ID; }

vrt_ctx* vrt_create(const vrt_config* cfg) {
    if (!cfg) { fail(VRT_E_INVALID, "null config"); return nullptr; }
    if (cfg->grid_res != 128 && cfg->grid_res != 256) { fail(VRT_E_INVALID, "grid_res must be 128 (pathtracer.py:83) or 256"); return nullptr; }
    if (cfg->width <= 0 || cfg->height <= 0 || cfg->width > 16384 || cfg->height > 16384) { fail(VRT_E_INVALID, "bad image size"); return nullptr; }
    if (cfg->max_depth < 1 || cfg->max_depth > 64) { fail(VRT_E_INVALID, "max_depth must be in 1..64"); return nullptr; }
    if (cfg->sky_res < 0 || cfg->sky_res > 8192 || (cfg->sky_res > 0 && cfg->sky_res < 4)) { fail(VRT_E_INVALID, "sky_res must be 0 or 4..8192"); return nullptr; }
    if (cfg->dx != 2.0f / (float)cfg->grid_res) { fail(VRT_E_INVALID, "dx must be 2 / grid_res: 1/64 at 128 (scene.py:11), 1/128 at 256 -- the grid spans the world box [-1, 1]^3"); return nullptr; }
    int own0 = 0, own1 = cfg->height;
    if (cfg->row_end > cfg->row_begin) {
        if (cfg->row_begin < 0 || cfg->row_end > cfg->height) { fail(VRT_E_INVALID, "row range outside the image"); return nullptr; }
        own0 = cfg->row_begin; own1 = cfg->row_end;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { fail(VRT_E_DEVICE, "no HIP device: libvrt_hip has no CPU path"); return nullptr; }
    if (cfg->device < 0 || cfg->device >= ndev) { fail(VRT_E_INVALID, "device ordinal out of range"); return nullptr; }
    hipDeviceProp_t prop;
    if (hipSetDevice(cfg->device) != hipSuccess || hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) {
        fail(VRT_E_DEVICE, "cannot select HIP device");
        return nullptr;
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fail(VRT_E_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
        return nullptr;
    }
    vrt_ctx* c = new vrt_ctx();
    c->cfg = *cfg;
    c->knobs = read_knobs();
    c->device = cfg->device;
    c->n_cu = prop.multiProcessorCount;
    c->own0 = own0; c->own1 = own1;
    c->halo = cfg->use_restir ? 26 : 2;  // bilinear + prepass taps; + spatial reuse radius 24 (pathtracer.py:1313)
    c->buf0 = own0 - c->halo < 0 ? 0 : own0 - c->halo;
    c->buf1 = own1 + c->halo > cfg->height ? cfg->height : own1 + c->halo;
    c->npix = (size_t)(c->buf1 - c->buf0) * cfg->width;
    bool ok = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess;
    const size_t G = (size_t)cfg->grid_res, nvox = G * G * G, n = c->npix;
    const size_t nw0 = nvox / 64, nw1 = nw0 / 64, nw2 = nw1 / 64;  // words of the brick levels
    ok = ok && dalloc(c, &c->d_mat, nvox) == hipSuccess && dalloc(c, &c->d_rgb, nvox * 3) == hipSuccess && dalloc(c, &c->d_grid, nvox) == hipSuccess;
    ok = ok && dalloc(c, &c->d_l0, nw0) == hipSuccess && dalloc(c, &c->d_l1, nw1) == hipSuccess && dalloc(c, &c->d_l2, nw2) == hipSuccess &&
         dalloc(c, &c->d_l3, 1) == hipSuccess && dalloc(c, &c->d_cull, 16) == hipSuccess && dalloc(c, &c->d_l0c, 32768) == hipSuccess && dalloc(c, &c->d_l0c_base, 513) == hipSuccess;
    ok = ok && dalloc(c, &c->d_mats, 128 * 14) == hipSuccess && dalloc(c, &c->d_counters, 1) == hipSuccess && dalloc(c, &c->d_work, VRT_WORK_SETS * VRT_WORK_HEADS * VRT_WORK_HEAD_STRIDE) == hipSuccess;
    ok = ok && dalloc(c, &c->d_cbuf[0], n) == hipSuccess && dalloc(c, &c->d_cbuf[1], n) == hipSuccess && dalloc(c, &c->sets[0].spec_planes, n * VRT_MAX_FUSED) == hipSuccess && dalloc(c, &c->sets[0].gb_pos, n) == hipSuccess;
    ok = ok && dalloc(c, &c->sets[0].gb_mat, n) == hipSuccess && dalloc(c, &c->sets[0].refl_planes, n * VRT_MAX_FUSED) == hipSuccess;
    ok = ok && dalloc(c, &c->d_gb_refl_f, n) == hipSuccess && dalloc(c, &c->d_ldr, n) == hipSuccess;
    for (int s = 0; s < VRT_GB_ROT && ok; s++) ok = ok && dalloc(c, &c->d_gb_normal[s], n) == hipSuccess && dalloc(c, &c->d_gb_depth[s], n) == hipSuccess;
    for (int s = 0; s < 2 && ok; s++) {
        ok = ok && dalloc(c, &c->d_hist_d[s], n) == hipSuccess && dalloc(c, &c->d_hist_s[s], n) == hipSuccess;
    }
    if (cfg->use_restir) {
        // VRT_MAX_FUSED planes of input reservoirs, the LAST being the slot the reference knows (as with the specular planes):
        // a fused launch ends on it, so a later pass that renders part of the frame finds the last sample's reservoirs there
        ok = ok && dalloc(c, &c->d_res_planes, n * VRT_MAX_FUSED) == hipSuccess && dalloc(c, &c->d_res[1], n) == hipSuccess;
        if (ok) c->d_res[0] = c->d_res_planes + (size_t)(VRT_MAX_FUSED - 1) * n;
    }
    if (cfg->use_restir) ok = ok && dalloc(c, &c->d_color_d2, n) == hipSuccess && dalloc(c, &c->d_color_s2, n) == hipSuccess &&
                              dalloc(c, &c->d_gris_geo, n) == hipSuccess && dalloc(c, &c->d_gris_src, n) == hipSuccess && dalloc(c, &c->d_gris_tst, n) == hipSuccess;
    ok = ok && dalloc(c, &c->d_mats_x, 128 * 8) == hipSuccess;
    if (cfg->sky_res > 0) {
        size_t ns = (size_t)cfg->sky_res * cfg->sky_res * 3;
        ok = ok && dalloc(c, &c->d_sky_scat, ns) == hipSuccess && dalloc(c, &c->d_sky_trans, ns) == hipSuccess;
        ok = ok && dalloc(c, &c->d_trans_lut, 256 * 128 * 3) == hipSuccess && dalloc(c, &c->d_cloud_tex, 256 * 256 * 3) == hipSuccess;
        ok = ok && dalloc(c, &c->d_cloud_ambient, 4) == hipSuccess;
    }
    if (!ok) {
        fail(VRT_E_DEVICE, std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError()));
        vrt_destroy(c);
        return nullptr;
    }
    // default material table rows (materials.py:50-63) until vrt_upload_materials is called
    {
        std::vector<float> t(128 * 14);
        const float row[14] = {1, 1, 1, 0, 0, 0.04f, 0, 0.9f, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < 128; i++) memcpy(&t[14 * i], row, sizeof(row));
        hipMemcpy(c->d_mats, t.data(), t.size() * 4, hipMemcpyHostToDevice);
        launch_mat_derived(c->stream, c->d_mats, c->d_mats_x);
    }
    c->last_gb_normal = c->d_gb_normal[VRT_GB_ROT - 1]; c->last_gb_depth = c->d_gb_depth[VRT_GB_ROT - 1];
    memset(&c->scene, 0, sizeof(c->scene));
    c->scene.floor_color[0] = c->scene.floor_color[1] = c->scene.floor_color[2] = 1.0f;  // pathtracer.py:91-93
    c->scene.floor_material = 1;
    c->scene.light_cos_theta_max = 1.0f;
    return c;
}

void vrt_destroy(vrt_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    release_gate(c);   // nothing may be left waiting at a gate
    if (c->stream && flush_deferred(c, false) != VRT_OK) { (void)hipGetLastError(); c->deferred.clear(); }
    drain_all(c);
    resolve_events(c);
#if defined(VRT_DEV_KNOBS)   // development build: what the A/B runs and tests/test_gpu_prepass.py read (the shipped library reports nothing)
    if (getenv("VRT_PRIMARY_REPORT")) {
        unsigned long long r[2] = {0ULL, 0ULL};
        if (c->d_pv_report && hipMemcpy(r, c->d_pv_report, sizeof(r), hipMemcpyDeviceToHost) != hipSuccess) (void)hipGetLastError();
        std::string grown;   // per lane that has a queue: how often it was reallocated for a larger launch (lane_primary_queue)
        for (const Lane& l : c->lanes) if (l.pv_counts) grown += (grown.empty() ? "" : ",") + std::to_string(l.pv_regrown);
        fprintf(stderr, "vrt: primary vertices served %u of %u render launches, paths finished %llu sent on %llu, queues regrown [%s]\n", c->primary_queued, c->passes_n[0], r[0], r[1],
                grown.c_str());
    }
    if (getenv("VRT_PREPASS_REPORT")) fprintf(stderr, "vrt: pre-passes queued %u told %u of %u render launches\n", c->prepass_queued, c->prepass_told, c->passes_n[0]);
#endif
    for (PlaneSet& p : c->sets) {
        if (p.ev_r) hipEventDestroy(p.ev_r);
        if (p.ev_t) hipEventDestroy(p.ev_t);
    }
    for (Lane& l : c->lanes) if (l.stream) hipStreamDestroy(l.stream);
    if (c->ev_main) hipEventDestroy(c->ev_main);
    for (int s = 0; s < VRT_FETCH_SLOTS; s++) if (c->ev_fetch[s]) hipEventDestroy(c->ev_fetch[s]);
    for (int s = 0; s < 2; s++) if (c->ev_cbuf_read[s]) hipEventDestroy(c->ev_cbuf_read[s]);
    if (c->ev_fetch_src) hipEventDestroy(c->ev_fetch_src);
    if (c->fetch_stream) hipStreamDestroy(c->fetch_stream);
    for (void* p : c->device_allocs) hipFree(p);   // every buffer, the sets' and lanes' included (dalloc, dmalloc)
    if (c->stream && c->owns_stream) hipStreamDestroy(c->stream);
    delete c;
}

int vrt_upload_voxels(vrt_ctx* c, const int8_t* mat, const uint8_t* rgb) {
    if (!c || !mat || !rgb) return fail(VRT_E_INVALID, "null argument");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    const size_t nvox = (size_t)c->cfg.grid_res * c->cfg.grid_res * c->cfg.grid_res;
    HIP_TRY(hipMemcpyAsync(c->d_mat, mat, nvox, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_rgb, rgb, nvox * 3, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(sync_guarded(c, c->stream));  // host buffers are only borrowed for the call
    c->prepared = false;
    c->main_dirty = true;
    return VRT_OK;
}
int vrt_upload_materials(vrt_ctx* c, const float* table) {
    if (!c || !table) return fail(VRT_E_INVALID, "null argument");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    c->main_dirty = true;
    HIP_TRY(hipMemcpyAsync(c->d_mats, table, 128 * 14 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_mat_derived(c->stream, c->d_mats, c->d_mats_x));
    HIP_TRY(sync_guarded(c, c->stream));
    return VRT_OK;
}
int vrt_upload_cloud_texture(vrt_ctx* c, const uint8_t* rgb) {
    if (!c || !rgb) return fail(VRT_E_INVALID, "null argument");
    if (c->cfg.sky_res <= 0) return fail(VRT_E_STATE, "context was created without sky tables (sky_res = 0)");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    c->main_dirty = true;
    HIP_TRY(hipMemcpyAsync(c->d_cloud_tex, rgb, 256 * 256 * 3, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(sync_guarded(c, c->stream));
    return VRT_OK;
}
int vrt_set_scene(vrt_ctx* c, const vrt_scene_params* s) {
    if (!c || !s) return fail(VRT_E_INVALID, "null argument");
    if (s->use_physical_sky && c->cfg.sky_res <= 0) return fail(VRT_E_INVALID, "use_physical_sky needs sky_res > 0 at vrt_create");
    c->scene = *s;
    c->have_scene = true;
    return VRT_OK;
}
int vrt_set_camera(vrt_ctx* c, const vrt_camera* cam) {
    if (!c || !cam) return fail(VRT_E_INVALID, "null argument");
    if (!(cam->render_scale > 0.0f) || cam->render_scale > 1.0f) return fail(VRT_E_INVALID, "render_scale must be in (0, 1]");
    if (cam->camera_is_moving && (c->own0 != 0 || c->own1 != c->cfg.height || c->stripe_rows) && !c->d_hx_hist_d)
        return fail(VRT_E_INVALID, "row-sharded contexts support the static camera only (history resampling crosses tiles)");
    c->cam = *cam;
    c->have_cam = true;
    return VRT_OK;
}
int vrt_reserve_cus(vrt_ctx* c, int n_cus) {
    if (!c || n_cus < 0) return fail(VRT_E_INVALID, "bad argument");
    if (n_cus > c->n_cu - 8) n_cus = c->n_cu - 8 > 0 ? c->n_cu - 8 : 0;
    HIP_TRY(hipSetDevice(c->device));
    c->reserved_cus = n_cus;
    c->render_blocks = 0;   // the grid is sized again at the next vrt_accumulate
    return VRT_OK;
}
int vrt_set_row_stripes(vrt_ctx* c, int stripe_rows, int n_parts, int part) {
    if (!c) return fail(VRT_E_INVALID, "null context");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    if (stripe_rows == 0) { c->stripe_rows = c->stripe_parts = c->stripe_part = 0; return VRT_OK; }
    if (stripe_rows < 8 || stripe_rows % 8 != 0 || n_parts < 1 || part < 0 || part >= n_parts) return fail(VRT_E_INVALID, "stripe_rows must be a multiple of 8, 0 <= part < n_parts");
    if (c->own0 != 0 || c->own1 != c->cfg.height) return fail(VRT_E_INVALID, "row stripes are a property of a whole-frame context (row_begin = row_end = 0)");
    if (c->cfg.use_restir) return fail(VRT_E_INVALID, "row stripes with ReSTIR would render a 24-row halo around every stripe: use contiguous row tiles");
    if (c->have_cam && c->cam.camera_is_moving) return fail(VRT_E_INVALID, "row stripes support the static camera only");
    if (c->hx_on) return fail(VRT_E_INVALID, "row stripes support the static camera only: no history exchange");
    if (c->frame != 0) return fail(VRT_E_STATE, "set the stripes before the first vrt_accumulate");
    c->stripe_rows = stripe_rows; c->stripe_parts = n_parts; c->stripe_part = part;
    return VRT_OK;
}
// ---- history exchange: the moving camera on row tiles ------------------------------------------------------------------------
// The moving-camera pass resamples the previous frame's histories, depth and normals at each pixel's reprojected position, which
// can be any row of the frame (pathtracer.py:993-1000, 1092-1183).  A row tile that opts in keeps all four as frame-sized planes:
// every vrt_accumulate call stores the tile's own rows there, the caller imports the other tiles' rows between calls.
static bool is_row_tile(const vrt_ctx* c) { return c->own0 != 0 || c->own1 != c->cfg.height; }
static void free_history_planes(vrt_ctx* c) {
    (void)dfree(c, &c->d_hx_hist_d); (void)dfree(c, &c->d_hx_hist_s); (void)dfree(c, &c->d_hx_depth); (void)dfree(c, &c->d_hx_normal);
    c->hx_row_epoch.clear();
}
int vrt_set_history_exchange(vrt_ctx* c, int on) {
    if (!c) return fail(VRT_E_INVALID, "null context");
    if (c->stripe_rows) return fail(VRT_E_INVALID, "row stripes support the static camera only: no history exchange");
    if (c->frame != 0) return fail(VRT_E_STATE, "set the history exchange before the first vrt_accumulate");
    if (!on && c->have_cam && c->cam.camera_is_moving && is_row_tile(c))
        return fail(VRT_E_INVALID, "the moving camera on a row tile needs the history exchange: set a static camera first");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    c->hx_on = on != 0;
    if (!c->hx_on || !is_row_tile(c)) { free_history_planes(c); return VRT_OK; }   // a whole-frame context has nothing to import
    if (c->d_hx_hist_d) return VRT_OK;
    const size_t n = (size_t)c->cfg.width * c->cfg.height;
    if (dalloc(c, &c->d_hx_hist_d, n) != hipSuccess || dalloc(c, &c->d_hx_hist_s, n) != hipSuccess || dalloc(c, &c->d_hx_depth, n) != hipSuccess ||
        dalloc(c, &c->d_hx_normal, n) != hipSuccess) {
        (void)hipGetLastError();
        free_history_planes(c);
        c->hx_on = false;
        return fail(VRT_E_DEVICE, "no device memory for the whole-frame history planes");
    }
    c->hx_row_epoch.assign((size_t)c->cfg.height, 0u);
    c->hx_epoch = 0;
    return VRT_OK;
}
// Rows [row0, row1) of the temporal state <-> caller-owned device memory: four planes back to back, each [row1 - row0][W]
// (diffuse history f32x4, specular history f32x4, g-buffer depth f32, g-buffer normal u32): 40 bytes a pixel.  Export
// (to_library = 0): rows of the context's own, as the most recent vrt_accumulate left them.  Import (1): rows outside them,
// into the whole-frame planes of a row tile with history exchange.  Queued on the context's stream.
int vrt_history_rows_io(vrt_ctx* c, int row0, int row1, void* device_ptr, int to_library) {
    if (!c || !device_ptr) return fail(VRT_E_INVALID, "null argument");
    if (c->stripe_rows) return fail(VRT_E_INVALID, "row stripes support the static camera only: no history exchange");
    if (row0 < 0 || row1 > c->cfg.height || row1 <= row0) return fail(VRT_E_INVALID, "row range outside the image");
    if (!to_library && (row0 < c->own0 || row1 > c->own1)) return fail(VRT_E_INVALID, "export: rows must lie inside the context's own rows");
    if (to_library && row0 < c->own1 && row1 > c->own0) return fail(VRT_E_INVALID, "import: rows must lie outside the context's own rows");
    if (to_library && !c->d_hx_hist_d) return fail(VRT_E_STATE, "import needs vrt_set_history_exchange on a row tile");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    const size_t W = c->cfg.width, rows = (size_t)(row1 - row0);
    char* rec = (char*)device_ptr;
    char* const planes[4] = {rec, rec + rows * W * 16, rec + rows * W * 32, rec + rows * W * 36};
    const size_t elem[4] = {16, 16, 4, 4};
    c->main_dirty = true;
    if (to_library) {
        void* const dst[4] = {c->d_hx_hist_d, c->d_hx_hist_s, c->d_hx_depth, c->d_hx_normal};
        for (int k = 0; k < 4; k++)
            HIP_TRY(hipMemcpyAsync((char*)dst[k] + (size_t)row0 * W * elem[k], planes[k], rows * W * elem[k], hipMemcpyDeviceToDevice, c->stream));
        for (int r = row0; r < row1; r++) c->hx_row_epoch[(size_t)r] = c->hx_epoch;
    } else {
        const void* const src[4] = {c->d_hist_d[c->hist_in], c->d_hist_s[c->hist_in], c->last_gb_depth, c->last_gb_normal};
        for (int k = 0; k < 4; k++)
            HIP_TRY(hipMemcpyAsync(planes[k], (const char*)src[k] + (size_t)(row0 - c->buf0) * W * elem[k], rows * W * elem[k], hipMemcpyDeviceToDevice, c->stream));
    }
    return VRT_OK;
}

int vrt_set_instrumented(vrt_ctx* c, int on) {
    if (!c) return fail(VRT_E_INVALID, "null context");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    c->instrumented = on != 0;
    c->count_as_timed = on == 2;
    c->render_blocks = 0;
    return VRT_OK;
}

int vrt_set_reference_indexing(vrt_ctx* c, int on) {
    if (!c) return fail(VRT_E_INVALID, "null context");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    c->ref_oob = on != 0;
    c->render_blocks = 0;   // other kernel instantiations (the instrumented ones carry the code): the grid is sized again
    return VRT_OK;
}

int vrt_prepare(vrt_ctx* c) {
    if (!c) return fail(VRT_E_INVALID, "null context");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    c->main_dirty = true;
    HIP_TRY(launch_prepare(c->stream, c->cfg.grid_res, c->d_mat, c->d_rgb, c->d_grid, c->d_l0, c->d_l1, c->d_l2, c->d_l3, c->d_l0c, c->d_l0c_base, c->d_cull));
    {
        const float off[8] = {-1e30f, -1e30f, -1e30f, 1e30f, 1e30f, 1e30f, 0.0f, 0.0f};   // nothing is culled
        HIP_TRY(hipMemcpyAsync(c->d_cull + 8, off, sizeof(off), hipMemcpyHostToDevice, c->stream));
        float box[8];
        HIP_TRY(hipMemcpyAsync(box, c->d_cull, sizeof(box), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));   // (source and destination are on this stack frame)
        note_cull_record(c, box);
    }
    if (c->scene.use_physical_sky == 1) {
        SkyPrecompute sp = make_sky(c);
        f3 sd, sc_;
        float cm;
        sun_of(c, sd, sc_, cm);
        size_t ns = (size_t)c->cfg.sky_res * c->cfg.sky_res * 3 * sizeof(float);
        HIP_TRY(launch_sky_prepare(c->stream, sp, sd, sc_, cm));
        HIP_TRY(hipMemsetAsync(c->d_sky_scat, 0, ns, c->stream));   // pathtracer.py:322-323
        HIP_TRY(hipMemsetAsync(c->d_sky_trans, 0, ns, c->stream));
        c->cloud_pass = 0;
    }
    c->prepared = true;
    return VRT_OK;
}
int vrt_sky_accumulate_clouds(vrt_ctx* c, int max_samples) {
    if (!c || max_samples <= 0) return fail(VRT_E_INVALID, "bad argument");
    if (!c->prepared || c->scene.use_physical_sky != 1) return fail(VRT_E_STATE, "needs vrt_prepare with use_physical_sky");
    HIP_TRY(hipSetDevice(c->device));
    f3 sd, sc_;
    float cm;
    sun_of(c, sd, sc_, cm);
    c->main_dirty = true;
    if (settle_ctx_stream(c) != VRT_OK) return VRT_E_DEVICE;   // (behind the render launches that read the tables)
    HIP_TRY(launch_sky_clouds(c->stream, make_sky(c), sd, sc_, cm, max_samples, c->cloud_pass, 0, c->cfg.sky_res));
    c->cloud_pass++;
    return VRT_OK;
}
// One cloud pass over the table columns of slice `slice_idx` of `max_slices` only (the split of vrt_sky_compute_slice,
// atmos.py:162).  A texel's passes depend on no other texel, so ranks that each own a slice run this max_samples times,
// then vrt_sky_compute_slice on their slice, and exchange columns (vrt_sky_table_io): voxel_rt2_amd/parallel.py.
int vrt_sky_accumulate_clouds_slice(vrt_ctx* c, int max_samples, int slice_idx, int max_slices) {
    if (!c || max_samples <= 0 || max_slices <= 0 || slice_idx < 0 || slice_idx >= max_slices) return fail(VRT_E_INVALID, "bad argument");
    if (!c->prepared || c->scene.use_physical_sky != 1) return fail(VRT_E_STATE, "needs vrt_prepare with use_physical_sky");
    HIP_TRY(hipSetDevice(c->device));
    f3 sd, sc_;
    float cm;
    sun_of(c, sd, sc_, cm);
    if (c->cfg.sky_res % max_slices != 0) return fail(VRT_E_INVALID, "sky_res is not a multiple of max_slices: trailing table columns would belong to no slice");
    const int w = c->cfg.sky_res / max_slices;
    c->main_dirty = true;
    if (settle_ctx_stream(c) != VRT_OK) return VRT_E_DEVICE;   // (behind the render launches that read the tables)
    HIP_TRY(launch_sky_clouds(c->stream, make_sky(c), sd, sc_, cm, max_samples, c->cloud_pass, w * slice_idx, w * (slice_idx + 1)));
    c->cloud_pass++;
    return VRT_OK;
}
// Copy table columns [u0, u1) between the library's sky tables and caller-owned DEVICE memory (f32[u1-u0][R][3], the table's
// own layout: a column slice is one contiguous block).  which = VRT_BUF_SKY_SCATTERING / VRT_BUF_SKY_TRANSMITTANCE;
// to_library = 0 reads, 1 writes.  Queued on the context's stream.
int vrt_sky_table_io(vrt_ctx* c, int which, int u0, int u1, void* device_ptr, int to_library) {
    if (!c || !device_ptr) return fail(VRT_E_INVALID, "null argument");
    if (c->cfg.sky_res <= 0) return fail(VRT_E_STATE, "no sky tables");
    if (which != VRT_BUF_SKY_SCATTERING && which != VRT_BUF_SKY_TRANSMITTANCE) return fail(VRT_E_INVALID, "not a sky table");
    if (u0 < 0 || u1 > c->cfg.sky_res || u1 <= u0) return fail(VRT_E_INVALID, "column range outside the table");
    HIP_TRY(hipSetDevice(c->device));
    float* table = which == VRT_BUF_SKY_SCATTERING ? c->d_sky_scat : c->d_sky_trans;
    const size_t col = (size_t)c->cfg.sky_res * 3 * sizeof(float);
    char* lib = (char*)table + (size_t)u0 * col;
    const size_t bytes = (size_t)(u1 - u0) * col;
    c->main_dirty = true;
    if (settle_ctx_stream(c) != VRT_OK) return VRT_E_DEVICE;
    if (to_library) HIP_TRY(hipMemcpyAsync(lib, device_ptr, bytes, hipMemcpyDeviceToDevice, c->stream));
    else HIP_TRY(hipMemcpyAsync(device_ptr, lib, bytes, hipMemcpyDeviceToDevice, c->stream));
    return VRT_OK;
}
int vrt_sky_compute_slice(vrt_ctx* c, int slice_idx, int max_slices) {
    if (!c || max_slices <= 0 || slice_idx < 0 || slice_idx >= max_slices) return fail(VRT_E_INVALID, "bad slice");
    if (!c->prepared || c->scene.use_physical_sky != 1) return fail(VRT_E_STATE, "needs vrt_prepare with use_physical_sky");
    HIP_TRY(hipSetDevice(c->device));
    f3 sd, sc_;
    float cm;
    sun_of(c, sd, sc_, cm);
    int w = c->cfg.sky_res / max_slices;  // atmos.py:162: floor division -- trailing columns (3840 / 32 has none) belong to no slice, as in the reference
    if (w == 0) return VRT_OK;   // fewer columns than slices: every slice is empty
    c->main_dirty = true;
    if (settle_ctx_stream(c) != VRT_OK) return VRT_E_DEVICE;
    HIP_TRY(launch_sky_slice(c->stream, make_sky(c), sd, sc_, cm, w * slice_idx, w * (slice_idx + 1)));
    return VRT_OK;
}

int vrt_reset(vrt_ctx* c) {
    if (!c) return fail(VRT_E_INVALID, "null context");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    for (int s = 0; s < 2; s++) {
        HIP_TRY(hipMemsetAsync(c->d_hist_d[s], 0, c->npix * sizeof(f4), c->stream));
        HIP_TRY(hipMemsetAsync(c->d_hist_s[s], 0, c->npix * sizeof(f4), c->stream));
    }
    if (c->d_hx_hist_d) {   // the whole frame's histories, as every rank's reset_framebuffer in the same step (imported g-buffer rows stay)
        const size_t n = (size_t)c->cfg.width * c->cfg.height;
        HIP_TRY(hipMemsetAsync(c->d_hx_hist_d, 0, n * sizeof(f4), c->stream));
        HIP_TRY(hipMemsetAsync(c->d_hx_hist_s, 0, n * sizeof(f4), c->stream));
    }
    c->acc_valid = false;   // nothing accumulated: vrt_denoise has no frame to work on
    return VRT_OK;
}
int vrt_end_frame(vrt_ctx* c) {
    if (!c) return fail(VRT_E_INVALID, "null context");
    memcpy(c->prev_view.m, c->cam.view, 64);
    memcpy(c->prev_proj.m, c->cam.proj, 64);
    c->have_prev = true;
    return VRT_OK;
}
int vrt_sync(vrt_ctx* c) {
    if (!c) return fail(VRT_E_INVALID, "null context");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    HIP_TRY(sync_guarded(c, c->stream));  // every render launch on the render streams has its temporal pass here
    return VRT_OK;
}

// copy rows [own0, own1) of a per-pixel device buffer into a full-image host array (other rows zero)
static int fetch_rows(vrt_ctx* c, const void* dbuf, size_t elem, void* out) {
    HIP_TRY(hipSetDevice(c->device));
    const size_t W = c->cfg.width;
    if (c->own0 != 0 || c->own1 != c->cfg.height || c->stripe_rows) memset(out, 0, (size_t)c->cfg.height * W * elem);   // a shard: the other rows are zero
    for (const auto& rr : owned_ranges(c)) {
        const char* src = (const char*)dbuf + (size_t)(rr.first - c->buf0) * W * elem;
        char* dst = (char*)out + (size_t)rr.first * W * elem;
        HIP_TRY(hipMemcpyAsync(dst, src, (size_t)(rr.second - rr.first) * W * elem, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(sync_guarded(c, c->stream));
    return VRT_OK;
}
int vrt_fetch_hdr(vrt_ctx* c, float* out) {
    if (!c || !out) return fail(VRT_E_INVALID, "null argument");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    return fetch_rows(c, c->d_cbuf[c->cidx], sizeof(f3), out);
}
int vrt_fetch_hdr_device(vrt_ctx* c, void* device_ptr) {
    if (!c || !device_ptr) return fail(VRT_E_INVALID, "null argument");
    if (vrt_fetch_hdr_device_async(c, device_ptr) != VRT_OK) return VRT_E_DEVICE;
    HIP_TRY(sync_guarded(c, c->stream));
    return VRT_OK;
}
int vrt_fetch_hdr_device_async(vrt_ctx* c, void* device_ptr) {
    if (!c || !device_ptr) return fail(VRT_E_INVALID, "null argument");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    const size_t W = c->cfg.width;
    size_t done = 0;   // (a striped context's rows: one stripe after the other)
    for (const auto& rr : owned_ranges(c)) {
        const char* src = (const char*)c->d_cbuf[c->cidx] + (size_t)(rr.first - c->buf0) * W * sizeof(f3);
        HIP_TRY(hipMemcpyAsync((char*)device_ptr + done * W * sizeof(f3), src, (size_t)(rr.second - rr.first) * W * sizeof(f3), hipMemcpyDeviceToDevice, c->stream));
        done += (size_t)(rr.second - rr.first);
    }
    return VRT_OK;
}
int vrt_set_stream(vrt_ctx* c, void* hip_stream) {
    if (!c) return fail(VRT_E_INVALID, "null context");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    HIP_TRY(sync_guarded(c, c->stream));
    resolve_events(c);
    for (PlaneSet& p : c->sets) p.ev_t_valid = false;  // everything recorded on the old stream has completed
    if (c->ctx_lane) {   // the stream is a render lane: the other lanes are drained too (as where the pipeline changes its shape), the lane goes on on the new stream
        drain_all(c);
        forget_passes(c);
        c->lanes[c->n_streams].last_seq = 0u;
    }
    c->main_dirty = true;
    c->main_touched = true;
    if (c->owns_stream && c->stream) hipStreamDestroy(c->stream);
    if (hip_stream) { c->stream = (hipStream_t)hip_stream; c->owns_stream = false; }
    else { HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->owns_stream = true; }
    return VRT_OK;
}
int vrt_fetch_ldr(vrt_ctx* c, float* out) {
    if (!c || !out) return fail(VRT_E_INVALID, "null argument");
    if (!c->have_cam) return fail(VRT_E_STATE, "vrt_set_camera has not been called");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    if (c->ev_fetch_src) {   // asynchronous fetches share d_ldr: theirs first
        HIP_TRY(hipEventRecord(c->ev_fetch_src, c->fetch_stream));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_fetch_src, 0));
    }
    FrameParams fp = make_frame_params(c);
    HIP_TRY(launch_tonemap(c->stream, fp, c->d_cbuf[c->cidx], c->d_ldr, c->own0, c->own1));
    return fetch_rows(c, c->d_ldr, sizeof(f4), out);
}

// ---- presenting every frame without emptying the pipeline ---------------------------------------------------------------
// The reference presents each frame (scene.py:255-262: accumulate, fetch_image, copy_prev_matrices).  vrt_fetch_hdr / _ldr
// are blocking copies into pageable memory on the context's stream: the caller waits for every launch queued so far and the
// next launch starts on an idle chip.  The asynchronous forms queue tonemap and copy on a stream of their own behind the
// passes queued so far and return; the caller goes on queueing frames and collects the image with vrt_fetch_wait(slot).
// `out` should be page-locked (vrt_host_alloc): the copy then runs beside the following launches.  The frame is whole for
// an unsharded context; a shard's rows land in their place and the other rows of `out` are left alone.
static int ensure_fetch_stream(vrt_ctx* c) {
    if (c->fetch_stream) return VRT_OK;
    HIP_TRY(hipStreamCreateWithFlags(&c->fetch_stream, hipStreamNonBlocking));
    for (int i = 0; i < VRT_FETCH_SLOTS; i++) HIP_TRY(hipEventCreateWithFlags(&c->ev_fetch[i], hipEventDisableTiming));
    for (int i = 0; i < 2; i++) HIP_TRY(hipEventCreateWithFlags(&c->ev_cbuf_read[i], hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_fetch_src, hipEventDisableTiming));
    return VRT_OK;
}
static int fetch_async(vrt_ctx* c, void* out, int slot, int what /* 0 HDR, 1 LDR f32 x 4, 2 LDR 8 bit x 4 */) {
    const bool ldr = what != 0;
    if (!c || !out || slot < 0 || slot >= VRT_FETCH_SLOTS) return fail(VRT_E_INVALID, "bad argument (slot must be 0..3)");
    if (ldr && !c->have_cam) return fail(VRT_E_STATE, "vrt_set_camera has not been called");
    if (c->fetch_valid[slot]) return fail(VRT_E_STATE, "this slot's previous fetch has not been collected (vrt_fetch_wait)");
    if (c->stripe_rows) return fail(VRT_E_STATE, "asynchronous fetches are not available on a context with row stripes");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    if (what == 2 && !c->d_ldr8 && dalloc(c, &c->d_ldr8, c->npix) != hipSuccess) { (void)dfree(c, &c->d_ldr8); return fail(VRT_E_DEVICE, "no memory for the 8-bit image"); }
    if (ensure_fetch_stream(c) != VRT_OK) return VRT_E_DEVICE;
    const size_t W = c->cfg.width, rows = (size_t)(c->own1 - c->own0), off = (size_t)(c->own0 - c->buf0) * W;
    const int b = c->cidx;
    HIP_TRY(hipEventRecord(c->ev_fetch_src, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->fetch_stream, c->ev_fetch_src, 0));
    if (what == 2) {
        HIP_TRY(launch_tonemap8(c->fetch_stream, make_frame_params(c), c->d_cbuf[b], c->d_ldr8, c->own0, c->own1));
        HIP_TRY(hipEventRecord(c->ev_cbuf_read[b], c->fetch_stream));   // the HDR buffer is free again once the tonemap has read it
        HIP_TRY(hipMemcpyAsync((char*)out + (size_t)c->own0 * W * 4, (const char*)c->d_ldr8 + off * 4, rows * W * 4, hipMemcpyDeviceToHost, c->fetch_stream));
    } else if (ldr) {
        HIP_TRY(launch_tonemap(c->fetch_stream, make_frame_params(c), c->d_cbuf[b], c->d_ldr, c->own0, c->own1));
        HIP_TRY(hipEventRecord(c->ev_cbuf_read[b], c->fetch_stream));
        HIP_TRY(hipMemcpyAsync((char*)out + (size_t)c->own0 * W * sizeof(f4), (const char*)c->d_ldr + off * sizeof(f4), rows * W * sizeof(f4), hipMemcpyDeviceToHost, c->fetch_stream));
    } else {
        HIP_TRY(hipMemcpyAsync((char*)out + (size_t)c->own0 * W * sizeof(f3), (const char*)c->d_cbuf[b] + off * sizeof(f3), rows * W * sizeof(f3), hipMemcpyDeviceToHost, c->fetch_stream));
        HIP_TRY(hipEventRecord(c->ev_cbuf_read[b], c->fetch_stream));
    }
    c->cbuf_read_pending[b] = true;
    HIP_TRY(hipEventRecord(c->ev_fetch[slot], c->fetch_stream));
    c->fetch_valid[slot] = true;
    return VRT_OK;
}
int vrt_fetch_hdr_async(vrt_ctx* c, float* out, int slot) { return fetch_async(c, out, slot, 0); }
int vrt_fetch_ldr_async(vrt_ctx* c, float* out, int slot) { return fetch_async(c, out, slot, 1); }
int vrt_fetch_ldr8_async(vrt_ctx* c, uint8_t* out, int slot) { return fetch_async(c, out, slot, 2); }
int vrt_fetch_wait(vrt_ctx* c, int slot) {
    if (!c || slot < 0 || slot >= VRT_FETCH_SLOTS) return fail(VRT_E_INVALID, "bad argument (slot must be 0..3)");
    if (!c->fetch_valid[slot]) return VRT_OK;
    HIP_TRY(hipSetDevice(c->device));
    // (the copy waits for launches that may be held at the dispatch gate: same bounded wait as every other synchronisation)
    wait_bounded(c, [&] { return hipEventQuery(c->ev_fetch[slot]); }, [](double) { std::this_thread::yield(); });
    HIP_TRY(hipEventSynchronize(c->ev_fetch[slot]));
    c->fetch_valid[slot] = false;
    return VRT_OK;
}
int vrt_host_alloc(vrt_ctx* c, uint64_t bytes, void** out) {
    if (!c || !out || bytes == 0) return fail(VRT_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipHostMalloc(out, (size_t)bytes, hipHostMallocDefault));
    return VRT_OK;
}
int vrt_host_free(vrt_ctx* c, void* p) {
    if (!c) return fail(VRT_E_INVALID, "null context");
    if (!p) return VRT_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipHostFree(p));
    return VRT_OK;
}
// The tile a multi-GPU rank hands to the gather, written by the temporal pass itself (12 bytes more per pixel of a pass that
// moves ~110) instead of a device-to-device copy behind it: the last pass of every vrt_accumulate call also stores its HDR
// rows [row_begin, row_end) in device_ptrs[k % n], k = the number of such tiles written so far (vrt_hdr_targets_written);
// the pass is queued on the context's stream by the call itself, so work the caller queues on that stream afterwards (an
// event for the gather's stream) is ordered behind the tile.  The caller keeps a tile untouched until its gather has read
// it.  n = 0 ends it.
int vrt_set_hdr_targets(vrt_ctx* c, void* const* device_ptrs, int n) {
    if (!c || n < 0 || (n > 0 && !device_ptrs)) return fail(VRT_E_INVALID, "bad argument");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    c->hdr_targets.assign(device_ptrs, device_ptrs + n);
    c->hdr_targets_written = c->hdr_targets_committed = 0;
    return VRT_OK;
}
int vrt_hdr_targets_written(vrt_ctx* c, uint64_t* count) {
    if (!c || !count) return fail(VRT_E_INVALID, "null argument");
    *count = c->hdr_targets_written;
    return VRT_OK;
}
int vrt_fetch_buffer(vrt_ctx* c, int which, void* out) {
    if (!c || !out) return fail(VRT_E_INVALID, "null argument");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    // the g-buffer written by the most recent accumulate (whichever schedule rendered it)
    const PlaneSet& last = c->sets[c->last_set];
    switch (which) {
        case VRT_BUF_GBUF_DEPTH: return fetch_rows(c, c->last_gb_depth, 4, out);
        case VRT_BUF_GBUF_NORMAL: return fetch_rows(c, c->last_gb_normal, 4, out);
        case VRT_BUF_GBUF_POSITION: return fetch_rows(c, last.gb_pos, 12, out);
        case VRT_BUF_GBUF_MAT: return fetch_rows(c, last.gb_mat, 4, out);
        case VRT_BUF_GBUF_REFL_DEPTH: return fetch_rows(c, c->d_gb_refl_f, 4, out);
        case VRT_BUF_HISTORY_DIFFUSE: return fetch_rows(c, c->d_hist_d[c->hist_in], 16, out);
        case VRT_BUF_HISTORY_SPECULAR: return fetch_rows(c, c->d_hist_s[c->hist_in], 16, out);
        default: break;
    }
    if (which == VRT_BUF_SKY_SCATTERING || which == VRT_BUF_SKY_TRANSMITTANCE) {
        if (c->cfg.sky_res <= 0) return fail(VRT_E_STATE, "no sky tables");
        size_t ns = (size_t)c->cfg.sky_res * c->cfg.sky_res * 3 * sizeof(float);
        HIP_TRY(hipMemcpyAsync(out, which == VRT_BUF_SKY_SCATTERING ? c->d_sky_scat : c->d_sky_trans, ns, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(sync_guarded(c, c->stream));
        return VRT_OK;
    }
    if (which == VRT_BUF_TRANS_LUT) {
        if (c->cfg.sky_res <= 0) return fail(VRT_E_STATE, "no sky tables");
        HIP_TRY(hipMemcpyAsync(out, c->d_trans_lut, 256 * 128 * 3 * 2, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(sync_guarded(c, c->stream));
        return VRT_OK;
    }
    return fail(VRT_E_INVALID, "unknown buffer id");
}
// ---- vrt_denoise: a spatial filter behind the frame (vrt_denoise.h) -------------------------------------------------------------------
// Reads what vrt_fetch_buffer / vrt_fetch_hdr would return now and writes its own scratch and `out`: no history, g-buffer, HDR buffer,
// counter or statistic.  Ordered as those fetches are: the pending accumulation first (enter), the work on the context's stream.  The
// histories, the HDR buffers and the rotating normal planes are next written by passes on that stream or by launches that wait for such
// a pass, so stream order keeps them behind the call.  NOT so the position and material planes of the last launch's copy: the launch
// that takes the copy again waits for the pass that last read it (PlaneSet::ev_t), which was queued BEFORE this call.  Only the prepare
// kernel reads them, so the call records that event again behind it: the copy's next writer then waits for the prepare kernel too.
// main_dirty / main_touched stay as a fetch leaves them.
static bool denoise_value_ok(float x) { return x >= 0.0f && x <= 3.402823466e+38f; }   // finite and not negative (a NaN fails both)
int vrt_denoise(vrt_ctx* c, const vrt_denoise_params* params, void* out, int on_device) {
    if (!c || !out) return fail(VRT_E_INVALID, "null argument");
    if (on_device != 0 && on_device != 1) return fail(VRT_E_INVALID, "on_device must be 0 or 1");
    const vrt_denoise_params p = params ? *params : vrt_denoise_params{5, 0.25f, 0.5f, 64.0f};
    if (p.iterations < 1 || p.iterations > VRT_DENOISE_MAX_ITERATIONS) return fail(VRT_E_INVALID, "iterations must be 1 .. 6");
    if (!denoise_value_ok(p.plane_tolerance) || !denoise_value_ok(p.sigma_l) || !denoise_value_ok(p.full_at))
        return fail(VRT_E_INVALID, "plane_tolerance, sigma_l and full_at must be finite and not negative");
    if (!c->acc_valid) return fail(VRT_E_STATE, "vrt_denoise works on an accumulated frame: call vrt_accumulate first (also after vrt_reset)");
    if (is_row_tile(c) || c->stripe_rows || c->hx_on)
        return fail(VRT_E_STATE, "vrt_denoise needs the whole frame: not on a row tile, with row stripes or with the history exchange (the filter reaches 62 rows)");
    if (c->acc_scale != 1.0f) return fail(VRT_E_STATE, "vrt_denoise needs a frame rendered at render scale 1");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    const size_t n = c->npix;   // (the whole frame: buf0 = 0, buf1 = height)
    if (!c->dn.guide) {
        bool ok = dmalloc(c, &c->dn.guide, n * sizeof(DenoiseGuide)) == hipSuccess && dmalloc(c, &c->dn.mat, n * sizeof(uint32_t)) == hipSuccess;
        for (int k = 0; k < 3 && ok; k++) ok = dmalloc(c, &c->dn.d[k], n * sizeof(f4)) == hipSuccess && dmalloc(c, &c->dn.s[k], n * sizeof(f4)) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            (void)dfree(c, &c->dn.guide); (void)dfree(c, &c->dn.mat);
            for (int k = 0; k < 3; k++) { (void)dfree(c, &c->dn.d[k]); (void)dfree(c, &c->dn.s[k]); }
            return fail(VRT_E_DEVICE, "no device memory for the denoiser's planes");
        }
    }
    if (!on_device && !c->d_dn_out) HIP_TRY(dmalloc(c, &c->d_dn_out, n * sizeof(f3)));
    f3* const d_out = on_device ? (f3*)out : c->d_dn_out;
    const PlaneSet& last = c->sets[c->last_set];
    const DenoiseSource src{last.gb_pos, c->last_gb_normal, last.gb_mat, c->d_hist_d[c->hist_in], c->d_hist_s[c->hist_in], c->d_cbuf[c->cidx]};
    const DenoiseSettings set{p.iterations, p.plane_tolerance * c->cfg.dx, p.sigma_l, p.full_at, c->acc_moving};
    HIP_TRY(launch_denoise_prepare(c->stream, c->cfg.width, c->cfg.height, set.moving, src, c->dn, d_out));
    if (last.ev_t) {   // (the overlapped pipeline's copies: a launch on the context's own stream is behind the call as it is)
        PlaneSet& l = c->sets[c->last_set];
        HIP_TRY(hipEventRecord(l.ev_t, c->stream));
        l.ev_t_valid = true; l.ev_t_of = c->last_set;
    }
    HIP_TRY(launch_denoise_filter(c->stream, c->cfg.width, c->cfg.height, set, c->dn, d_out));
    if (on_device) return VRT_OK;
    HIP_TRY(hipMemcpyAsync(out, d_out, n * sizeof(f3), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(sync_guarded(c, c->stream));   // (also ends the loan of the host array)
    return VRT_OK;
}
// Launches of half the slots on two streams of the pipeline's own: the shape whose flags give bit 24 to the context's lane (include/vrt_api.h).
static bool lean_shape(const vrt_ctx* c) { return c->overlap_ready && c->n_streams == 2 && c->grid_div == 2; }
int vrt_get_stats(vrt_ctx* c, vrt_stats* out) {
    if (!c || !out) return fail(VRT_E_INVALID, "null argument");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    HIP_TRY(sync_guarded(c, c->stream));
    resolve_events(c);
    Counters h;
    HIP_TRY(hipMemcpy(&h, c->d_counters, sizeof(h), hipMemcpyDeviceToHost));
    c->stats.rays = h.rays; c->stats.dda_iters = h.iters; c->stats.occupancy_queries = h.queries;
    c->stats.closest_hits = h.closest_hits; c->stats.sky_lookups = h.sky_lookups;
    {   // every pass counted, the timed ones' mean for all of them
        auto scaled = [&](int k) { return c->timed_n[k] ? c->timed_ms[k] * ((double)c->passes_n[k] / (double)c->timed_n[k]) : 0.0; };
        c->stats.render_ms = scaled(0); c->stats.temporal_ms = scaled(1); c->stats.gris_ms = scaled(2);
        c->stats.render_launches = c->passes_n[0]; c->stats.temporal_launches = c->passes_n[1]; c->stats.gris_launches = c->passes_n[2];
    }
    c->stats.pipeline_flags = (c->overlap_ready ? 1u : 0u) | (c->drain_signal ? 2u : 0u) | (((uint32_t)c->gate_releases & 0xFFFFu) << 8) |
                              (lean_shape(c) ? ((c->mode_switches < 127u ? c->mode_switches : 127u) << 25) | (c->ctx_lane ? 1u << 24 : 0u)
                                             : (c->mode_switches < 255u ? c->mode_switches : 255u) << 24) |
                              (c->overlap_ready ? ((uint32_t)(c->n_streams == 3 ? 2 : c->n_streams >> 1) << 2) | ((uint32_t)c->grid_div << 5) : 0u);
    *out = c->stats;
    return VRT_OK;
}
int vrt_reset_stats(vrt_ctx* c) {
    if (!c) return fail(VRT_E_INVALID, "null context");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    HIP_TRY(sync_guarded(c, c->stream));
    resolve_events(c);
    HIP_TRY(hipMemsetAsync(c->d_counters, 0, sizeof(Counters), c->stream));   // on the stream the counting launches follow on
    c->main_dirty = true;
    memset(&c->stats, 0, sizeof(c->stats));
    for (int k = 0; k < 3; k++) { c->timed_ms[k] = 0.0; c->timed_n[k] = c->passes_n[k] = 0u; }
    c->since_reset = 0u;
    return VRT_OK;
}
// Test hook: rows of arguments through single functions of the sky precompute (vrt_sky_kernels.hip, k_sky_probe).
int vrt_sky_probe(vrt_ctx* c, int op, int n, const float* in, int in_stride, float* out, int out_stride, const uint16_t* trans_lut, const float* cloud_ambient) {
    if (!c || !in || !out || n <= 0 || in_stride <= 0 || out_stride <= 0 || op < 0 || op > 9) return fail(VRT_E_INVALID, "bad argument");
    if (c->cfg.sky_res <= 0) return fail(VRT_E_STATE, "context was created without sky tables (sky_res = 0)");
    HIP_TRY(hipSetDevice(c->device));
    c->main_dirty = true;
    if (settle_ctx_stream(c) != VRT_OK) return VRT_E_DEVICE;
    if (trans_lut) HIP_TRY(hipMemcpyAsync(c->d_trans_lut, trans_lut, 256 * 128 * 3 * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    float *d_in = nullptr, *d_out = nullptr;
    HIP_TRY(hipMalloc((void**)&d_in, (size_t)n * in_stride * sizeof(float)));
    if (hipMalloc((void**)&d_out, (size_t)n * out_stride * sizeof(float)) != hipSuccess) { hipFree(d_in); return fail(VRT_E_DEVICE, "no memory for the probe"); }
    const f3 amb = cloud_ambient ? mk3(cloud_ambient[0], cloud_ambient[1], cloud_ambient[2]) : mk3(0.0f);
    hipError_t e = hipMemcpyAsync(d_in, in, (size_t)n * in_stride * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_out, 0, (size_t)n * out_stride * sizeof(float), c->stream);
    if (e == hipSuccess) e = launch_sky_probe(c->stream, make_sky(c), op, n, d_in, in_stride, d_out, out_stride, amb);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, (size_t)n * out_stride * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    hipFree(d_in); hipFree(d_out);
    if (e != hipSuccess) return fail(VRT_E_DEVICE, std::string("sky probe: ") + hipGetErrorString(e));
    return VRT_OK;
}
// Test hook: rays through the closest-hit walk on the context's own pyramid (vrt_probe.h, k_trace_probe).
int vrt_trace_probe(vrt_ctx* c, int mode, int n, const float* origin_dir, void* out) {
    if (!c || !origin_dir || !out || n <= 0 || mode < 0 || (mode & ~(3 | PROBE_CULL_BOX)) || (mode & 3) >= PROBE_WALK_COUNT) return fail(VRT_E_INVALID, "bad argument");
    if (!c->prepared) return fail(VRT_E_STATE, "needs vrt_prepare");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    float* d_in = nullptr;
    ProbeOut* d_out = nullptr;
    HIP_TRY(hipMalloc((void**)&d_in, (size_t)n * 6 * sizeof(float)));
    if (hipMalloc((void**)&d_out, (size_t)n * sizeof(ProbeOut)) != hipSuccess) { hipFree(d_in); return fail(VRT_E_DEVICE, "no memory for the probe"); }
    // cull = (mode & PROBE_CULL_BOX) && !ref_oob: the MODE asks for the box (cull_active), whatever the counters (instrumented) and VRT_CULL say
    RenderInputs in = render_inputs(c, 1);
    in.cull_active = (mode & PROBE_CULL_BOX) != 0; in.instrumented = false; in.knob_cull = -1;
    const float* cull = c->d_cull + (plan_render_variant(in).cull ? 0 : 8);
    hipError_t e = hipMemcpyAsync(d_in, origin_dir, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_out, 0, (size_t)n * sizeof(ProbeOut), c->stream);
    if (e == hipSuccess) e = launch_trace_probe(c->stream, c->cfg.grid_res, mode & 3, make_scene_data(c).pyr, cull, n, d_in, d_out);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, (size_t)n * sizeof(ProbeOut), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = sync_guarded(c, c->stream);
    hipFree(d_in); hipFree(d_out);
    if (e != hipSuccess) return fail(VRT_E_DEVICE, std::string("trace probe: ") + hipGetErrorString(e));
    return VRT_OK;
}
// Test hook: rows of arguments through single shading functions on the context's materials, scene and camera (vrt_shade_probe.h, k_shade_probe).
int vrt_shade_probe(vrt_ctx* c, int op, int n, const float* in, int in_stride, float* out, int out_stride) {
    if (!c || !in || !out || n <= 0 || op < 0 || op >= SHADE_OP_COUNT || in_stride < shade_probe_in_width(op) || out_stride < shade_probe_out_width(op))
        return fail(VRT_E_INVALID, "bad argument");
    if (!c->prepared) return fail(VRT_E_STATE, "needs vrt_prepare");
    if (enter(c) != VRT_OK) return VRT_E_DEVICE;
    float *d_in = nullptr, *d_out = nullptr, *d_lane = nullptr;
    const size_t n_in = (size_t)n * in_stride, n_out = (size_t)n * out_stride, n_lane = op == SHADE_SHIFT ? (size_t)n * VRT_SHADE_LANE_TABLE : 0;
    hipError_t e = hipMalloc((void**)&d_in, n_in * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&d_out, n_out * sizeof(float));
    if (e == hipSuccess && n_lane) e = hipMalloc((void**)&d_lane, n_lane * sizeof(float));
    if (e == hipSuccess) e = hipMemcpyAsync(d_in, in, n_in * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_out, 0, n_out * sizeof(float), c->stream);
    if (e == hipSuccess && n_lane) e = hipMemsetAsync(d_lane, 0, n_lane * sizeof(float), c->stream);
    if (e == hipSuccess) e = launch_shade_probe(c->stream, make_frame_params(c), make_scene_data(c), c->d_mats_x, op, n, d_in, in_stride, d_out, out_stride, d_lane);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, n_out * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = sync_guarded(c, c->stream);
    hipFree(d_in); hipFree(d_out); hipFree(d_lane);
    if (e != hipSuccess) return fail(VRT_E_DEVICE, std::string("shade probe: ") + hipGetErrorString(e));
    return VRT_OK;
}
// diagnostic builds (-DVRT_DIAG_REGIONS) only: 32 x {wave entries, active lanes} per instrumented code region
int vrt_diag_regions(vrt_ctx* c, unsigned long long* out64, int reset) {
    if (!c || !out64) return fail(VRT_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, 64 * sizeof(unsigned long long)));
    hipError_t e = launch_diag_read(c->stream, d, reset);
    if (e != hipSuccess) { hipFree(d); return fail(VRT_E_STATE, "library was not built with VRT_DIAG_REGIONS"); }
    HIP_TRY(sync_guarded(c, c->stream));
    HIP_TRY(hipMemcpy(out64, d, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    hipFree(d);
    return VRT_OK;
}
// runs op over n floats on the device: checks the numeric contract of vrt_detmath.h on gfx950
int vrt_detmath_probe(int device, int op, int n, const float* a, const float* b, float* out) {
    if (n <= 0 || !a || !b || !out) return fail(VRT_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(device));
    float *da = nullptr, *db = nullptr, *dout = nullptr;
    HIP_TRY(hipMalloc((void**)&da, n * 4));
    HIP_TRY(hipMalloc((void**)&db, n * 4));
    HIP_TRY(hipMalloc((void**)&dout, n * 4));
    HIP_TRY(hipMemcpy(da, a, n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(db, b, n * 4, hipMemcpyHostToDevice));
    HIP_TRY(launch_detmath_probe(0, op, n, da, db, dout));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout, n * 4, hipMemcpyDeviceToHost));
    hipFree(da); hipFree(db); hipFree(dout);
    return VRT_OK;
}

}  // extern "C"
