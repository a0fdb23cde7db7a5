// vrt_ctx.h -- private to vrt_api.hip's translation unit: the context, error reporting, device allocation, and the waits that know
// about the dispatch gate.  (vrt_api.hip: the entry points; vrt_pipeline.hip: launch sequencing; vrt_plan.h: its decisions;
// vrt_scene_ops.hip: the calls on a prepared scene.)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include <algorithm>
#include "../../include/vrt_api.h"
#include "vrt_kernels.h"
#include "vrt_plan.h"

static_assert(VRT_MAX_DEFER == VRT_MAX_GROUP, "VRT_DEFER may ask for as many launches as k_temporal_group takes");
#define VRT_GB_ROT (VRT_MAX_SETS + 1)   // rotating g-buffer normal / depth copies: copy j is read by temporal passes j and j + 1, and the
                                       // launch that writes it again only waits for the pass VRT_MAX_SETS launches back
#define VRT_WORK_SETS 16  // rotating sets of work heads (vrt_kernels.hip: a launch zeroes the set eight launches ahead)
#define VRT_FETCH_SLOTS 4 // asynchronous fetches the caller may have outstanding (vrt_fetch_*_async)

using namespace vrt;

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#if defined(VRT_HOST_PROFILE)
// Diagnostic build (tools/probe_host_cost.py): host time of every HIP_TRY call site, printed when the library is unloaded.
#include <map>
static double prof_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static std::map<std::string, std::pair<double, long>> g_prof;
static struct ProfDump {
    ~ProfDump() {
        std::vector<std::pair<double, std::string>> rows;
        for (auto& kv : g_prof) rows.push_back({kv.second.first, kv.first});
        std::sort(rows.begin(), rows.end());
        for (auto it = rows.rbegin(); it != rows.rend() && it - rows.rbegin() < 25; ++it)
            fprintf(stderr, "[host] %9.1f ms %8ld calls %7.2f us  %s\n", it->first * 1e3, g_prof[it->second].second, it->first * 1e6 / (double)g_prof[it->second].second, it->second.substr(0, 110).c_str());
    }
} g_prof_dump;
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        const double t0_ = prof_now();                                                                  \
        hipError_t e_ = (expr);                                                                         \
        auto& p_ = g_prof[#expr]; p_.first += prof_now() - t0_; p_.second++;                            \
        if (e_ != hipSuccess)                                                                           \
            return fail(VRT_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));               \
    } while (0)
#else
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(VRT_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));               \
    } while (0)
#endif

struct EventPair { hipEvent_t a, b; int kind; unsigned weight; };  // kind 0 render, 1 temporal, 2 gris; weight: passes the kernel between them stands for

// One copy of everything a render launch writes and its temporal pass reads, with the events that order the two.  Set 0 is what a
// launch that is not overlapped uses (the buffers the reference knows); overlapped launches rotate through n_sets of them.
struct PlaneSet {
    f3* multi_d = nullptr;         // diffuse colour planes of the samples fused into one launch (set 0: allocated on first use)
    // specular colour and raw reflection depth: VRT_MAX_FUSED planes each, the LAST plane being the buffer the reference knows
    // (color_buffer_specular, gbuff_depth_reflection); a fused launch ends on it, so whatever later reads stale pixels (moving
    // camera at half render scale) finds the last sample there, as in the reference
    f3* spec_planes = nullptr;
    float* refl_planes = nullptr;
    f3* gb_pos = nullptr;
    uint32_t* gb_mat = nullptr;
    hipEvent_t ev_r = nullptr;     // the render launch that wrote this copy
    hipEvent_t ev_t = nullptr;     // the pass recorded for this copy
    bool ev_t_valid = false;
    int ev_t_of = 0;               // the set whose ev_t stands for the pass that last read this one (a grouped pass records one event)
};
// One render stream and what only one launch at a time may use.  Lane 0's scratch and camera-ray table also serve the launches
// that are not overlapped (on the context's stream).
struct Lane {
    hipStream_t stream = nullptr;
    uint32_t* pool_scratch = nullptr;
    PrimaryRecord* prim_cache = nullptr;   // camera-ray records of fused launches (allocated on first use)
    uint32_t* pv_counts = nullptr;         // the queue k_primary_vertex leaves this lane's launch (vrt_primary.h; allocated on first use,
    uint32_t* pv_entries = nullptr;        // grown when a launch needs more): counter lines, continuation records, leftover items
    uint32_t* pv_leftovers = nullptr;
    size_t pv_entry_words = 0, pv_left_words = 0;   // words allocated
#if defined(VRT_DEV_KNOBS)
    unsigned pv_regrown = 0;               // times a queue this lane already had was reallocated for a larger launch (VRT_PRIMARY_REPORT)
#endif
    unsigned last_seq = 0;                 // launch_seq + 1 of the last launch queued on this stream (0: none)
    int last_set = -1;                     // the copy that launch wrote: its ev_r is the lane's latest (-1: none since the streams were drained)
};

struct vrt_ctx {
    vrt_config cfg;
    Knobs knobs;                      // environment switches as they stood when the context was created
    vrt_scene_params scene;
    vrt_camera cam;
    bool have_scene = false, have_cam = false, prepared = false, have_prev = false;
    bool instrumented = false;
    bool count_as_timed = false;      // instrumented launches keep the camera-ray reuse of the timed schedule (vrt_set_instrumented(ctx, 2))
    bool ref_oob = false;             // vrt_set_reference_indexing: cells outside the grid are read the reference's way (vrt_trace.h, ref_bit)
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = true;
    std::vector<void*> device_allocs; // every device buffer the context owns (dalloc, dmalloc): what vrt_destroy frees
    int n_cu = 0, render_blocks = 0;
    int render_blocks_d12 = 0;        // ... of the twelve-wave geometry a dense grid renders on (k_render_pool_dense12; 0: never taken)
    size_t pool_scratch_bytes = 0;    // a lane's scratch: room for either geometry
    int reserved_cus = 0;             // CUs' worth of workgroup slots the persistent render grid leaves free (vrt_reserve_cus)
    // rows
    int own0 = 0, own1 = 0;   // rows this context produces
    int stripe_rows = 0, stripe_parts = 0, stripe_part = 0;   // ... or, of them, every stripe_parts-th stripe of stripe_rows rows (vrt_set_row_stripes)
    int buf0 = 0, buf1 = 0;   // rows held in the buffers (own + halo)
    int halo = 2;
    size_t npix = 0;          // (buf1 - buf0) * W
    // scene data
    int8_t* d_mat = nullptr; uint8_t* d_rgb = nullptr; uint32_t* d_grid = nullptr;
    unsigned long long *d_l0 = nullptr, *d_l1 = nullptr, *d_l2 = nullptr, *d_l3 = nullptr, *d_l0c = nullptr;
    uint32_t* d_l0c_base = nullptr;  // [512] offsets + [1] count
    bool cull_active = false;        // the grown box leaves part of the grid out: there are rays to cull (read back by vrt_prepare)
    bool dense_grid = false;         // half of the bricks or more are non-empty (read back by vrt_prepare)
    float* d_cull = nullptr;         // [8] grown bounding box of the solid voxels + flag, [8] the same with the flag off (cull_ray, vrt_trace.h)
    uint8_t* d_edit_stage = nullptr;  // vrt_update_voxels, host path: the box arrays on their way to k_edit_store (grown on demand)
    size_t edit_stage_bytes = 0;
    uint8_t* d_cast_stage = nullptr;  // vrt_cast_rays / vrt_fetch_voxels, host path: rays in and records out, or the box arrays on their way out (grown on demand)
    size_t cast_stage_bytes = 0;
    uint8_t* d_vox = nullptr;         // vrt_voxelize_triangles / vrt_fill_triangles: the head region (ownership words or toggle words), box arrays, item list, heads and result record (plan_tri_layout; grown on demand)
    size_t vox_bytes = 0;
    uint8_t* d_dist = nullptr;        // vrt_distance_field: the passes' values and chosen coordinates, and on the host path the staged results (plan_distance_layout; grown on demand)
    size_t dist_bytes = 0;
    uint8_t* d_label = nullptr;       // vrt_label_components: the counter words and on the host path the staged labels (plan_label_layout; grown on demand)
    size_t label_bytes = 0;
    uint8_t* d_move = nullptr;        // vrt_move_voxels: the snapshot words, the box arrays of the larger box, the record and on the host path the staged selection (move_layout; grown on demand)
    size_t move_bytes = 0;
    uint8_t* d_radiance_plane = nullptr;   // vrt_trace_radiance, vrt_gather_irradiance, vrt_gather_probes: a work counter (256 bytes) and the scratch plane of VRT_RADIANCE_ITEMS item values (allocated on first use)
    float* d_mats = nullptr;
    Counters* d_counters = nullptr;
    unsigned* d_work = nullptr;
    // sky
    float *d_sky_scat = nullptr, *d_sky_trans = nullptr, *d_cloud_ambient = nullptr;
    uint16_t* d_trans_lut = nullptr;
    uint8_t* d_cloud_tex = nullptr;
    uint32_t cloud_pass = 0;
    // per-pixel
    f3 *d_cbuf[2] = {nullptr, nullptr};  // color_buffer: [cidx] = HDR of the last pass = render target of the next (pathtracer.py:39)
    int cidx = 0;
    f3 *d_color_d2 = nullptr, *d_color_s2 = nullptr;
    uint32_t* d_gb_normal[VRT_GB_ROT] = {};  // rotating: [cur] is written by the next launch, [prev_gb] by the last
    float* d_gb_depth[VRT_GB_ROT] = {};
    float* d_gb_refl_f = nullptr;
    f4 *d_hist_d[2] = {nullptr, nullptr}, *d_hist_s[2] = {nullptr, nullptr};
    int hist_in = 0;  // history ping-pong
    f4* d_ldr = nullptr;
    uint32_t* d_ldr8 = nullptr;   // rgba8 image of vrt_fetch_ldr8_async (allocated on first use)
    ReservoirRec* d_res[2] = {nullptr, nullptr};
    ReservoirRec* d_res_planes = nullptr;   // input reservoirs: VRT_MAX_FUSED planes, d_res[0] is the last of them
    GrisGeo* d_gris_geo = nullptr;   // per-pixel records of k_gris's prepare pass (vrt_restir.h)
    GrisSrc* d_gris_src = nullptr;
    GrisTest* d_gris_tst = nullptr;
    float* d_mats_x = nullptr;       // [128][8] mat_derive() of every material row
    int cur = 0;      // g-buffer rotation: render writes [cur], temporal reads [prev_gb] as "prev"
    int prev_gb = VRT_GB_ROT - 1;  // the copy the most recent launch wrote
    const uint32_t* last_gb_normal = nullptr;   // g-buffer normal / depth of the most recent render launch (either schedule)
    const float* last_gb_depth = nullptr;
    mat4 prev_view{}, prev_proj{};
    uint32_t frame = 0;
    unsigned primary_queued = 0;      // launches whose primary vertices were shaded ahead of them (plan_primary)
    unsigned long long* d_pv_report = nullptr;   // development builds with VRT_PRIMARY_REPORT: paths finished ahead of the pool, paths sent on
    unsigned prepass_queued = 0, prepass_told = 0;   // pre-passes queued so far, and those the launch was told of (plan_prepass)
    LaunchSeq launch_seq;     // .next: render launches so far (selects which work counters a launch uses, and its records' tag); .reserved: a pre-pass holds that number (vrt_plan.h)

    // ---- the launch pipeline (vrt_pipeline.hip) ----
    // Overlapped launches (vrt_accumulate): n_sets copies of everything a render launch writes and its temporal pass reads,
    // n_streams render streams and the events that order them, so that the next launches start while launch k drains and temporal
    // pass k runs beside them.
    PlaneSet sets[VRT_MAX_SETS];
    Lane lanes[VRT_MAX_STREAMS];
    hipEvent_t ev_main = nullptr;
    int n_streams = 2;   // the shape in use (plan_pipeline_shape, ensure_overlap)
    int grid_div = 1;
    bool pass_on_render = false;
    // The context's stream as render lane number n_streams (PipelineShape::ctx_lane): lanes[n_streams] holds that lane's scratch and
    // camera-ray table and NO stream -- lane_stream() answers with the context's, whichever the caller has set (vrt_set_stream).
    bool ctx_lane = false;
    bool pass_on_last = false;   // grouped passes run on the lane of the group's last launch (PipelineShape::pass_on_last)
    // Passes and launches on the OTHER lanes that the context's stream has not been made to wait for: with ctx_lane a wait queued
    // with every pass would hold the stream's own next launch behind it, so the waits are queued where somebody is about to look at
    // the stream or to queue work on it (settle_ctx_stream: flush_deferred's callers, the sky entry points, abort_pipeline).
    bool ctx_unsettled = false;
    int defer_k = 1;
    int n_sets = 3;      // copies in use: lanes + defer_k
    bool overlap_ready = false, overlap_failed = false;
    unsigned mode_switches = 0;   // times the pipeline was drained to change its depth (ensure_overlap)
    // A render launch queued behind another on another render stream would be dispatched at once and sit in the
    // queue until workgroups retire -- which the profiler and the events count as its run time.  Instead the kernel
    // raises this word (HSA signal memory, host visible) to launch_seq + 1 when it starts to drain, and the stream of the
    // launch that will take its workgroup slots (the next one; the one after with half-size launches) waits for that
    // value (hipStreamWaitValue32) before the dispatch.  The gate only TIMES dispatches
    // (ordering is by events), so raising the word early is always safe: release_gate() does it from the host on
    // error paths and when a synchronisation overstays (gate_watchdog_ms).  A stream wait is itself a queue operation:
    // under a tool that runs one queue operation at a time (rocprofv3 --pmc) a wait that is dispatched ahead of the
    // launch it waits for blocks that launch for ever (tools/probes/probe_gate.cpp reproduces it: the wait completes
    // by itself in 0.3 ms, never under --pmc, and a host store releases it) -- ensure_overlap() tests for exactly
    // that once and leaves the gate out where the test fails.
    uint32_t* drain_signal = nullptr;
    bool drain_signalled = false;  // the most recent render launch was given the signal
    bool prev_launch_full = true;  // ... and took every workgroup slot (the next dispatch waits for ITS drain, whatever the pipeline's depth)
    unsigned last_full_seq = 0;    // launch_seq + 1 of the most recent launch that took every workgroup slot (0: none)
    unsigned gate_releases = 0;    // host releases so far (error paths, watchdog): diagnostic
    // Deferred accumulation: with a static camera the passes of K consecutive overlapped launches run as ONE kernel
    // (k_temporal_group) once the K-th is queued, or earlier when somebody is about to look (flush_deferred).  A launch's
    // planes stay occupied until then: n_sets = n_streams + K copies.
    struct Deferred { TemporalSlice slice; int set; int lane; bool timed; };
    std::vector<Deferred> deferred;
    // Where a grouped pass runs: on the context's stream, or (pass_on_last: the shape with ctx_lane, and the A/B shapes of
    // VRT_PASS_STREAM=1) on the lane of the group's last launch -- behind it in stream order, behind the others by their events,
    // passes following one another by last_pass_ev; the context's stream then only WAITS for the pass's event (queue_group; with
    // ctx_lane: settle_ctx_stream), so that whatever is queued on it next, by the library or the caller, comes behind it.
    hipEvent_t last_pass_ev = nullptr;   // event of the most recent pass queued on a render stream (nullptr: none since the streams were drained)
    int last_pass_lane = -1;
    bool main_touched = true;   // the context's stream was given work since the last pass on a render stream: that pass's successor waits for it
    bool main_dirty = true;     // work other than accumulate passes was queued on the main stream since the last overlapped launch
    unsigned pipe_seq = 0;      // overlapped launches so far
    int last_set = 0;           // copy the most recent render launch wrote
    int last_render_set = -1;   // copy whose ev_r the most recent overlapped launch recorded (-1: none yet)
    // Device time per kind of pass (0 render, 1 accumulation, 2 spatial reuse): every pass is counted, the ones that carry timers
    // are summed (small launches: one in eight, plan_timer_period) and vrt_get_stats scales the sum to all of them.
    double timed_ms[3] = {0.0, 0.0, 0.0};
    uint32_t timed_n[3] = {0u, 0u, 0u}, passes_n[3] = {0u, 0u, 0u};
    unsigned since_reset = 0;     // render launches since vrt_reset_stats: the first one carries timers
    std::vector<EventPair> pending;
    vrt_stats stats{};

    // HDR tiles handed over device to device (vrt_set_hdr_targets): pass k also writes its HDR rows to ring[k % n]
    std::vector<void*> hdr_targets;
    unsigned long long hdr_targets_written = 0;
    unsigned long long hdr_targets_committed = 0;   // ... by calls that returned VRT_OK (abort_pipeline rolls back to it)
    // asynchronous fetches (vrt_fetch_*_async)
    hipStream_t fetch_stream = nullptr;
    hipEvent_t ev_fetch[VRT_FETCH_SLOTS] = {}, ev_fetch_src = nullptr, ev_cbuf_read[2] = {};
    bool fetch_valid[VRT_FETCH_SLOTS] = {}, cbuf_read_pending[2] = {};
    // vrt_denoise: what the most recent vrt_accumulate rendered with (the camera may have been set again since), and the pass's scratch
    // planes (allocated on first use)
    bool acc_valid = false;           // a vrt_accumulate has rendered since vrt_create / the last vrt_reset
    int acc_moving = 0;               // its camera_is_moving
    float acc_scale = 1.0f;           // its render_scale
    DenoiseScratch dn{};
    f3* d_dn_out = nullptr;           // the host path's result on its way out
    // History exchange (vrt_set_history_exchange): a row tile's whole-frame copy of the previous frame's temporal state, which the
    // moving-camera pass resamples from.  Own rows are stored by every vrt_accumulate call, the other rows imported by the caller
    // (vrt_history_rows_io); hx_row_epoch[r] = hx_epoch when row r was imported after the most recent call.
    bool hx_on = false;               // opted in (also on a whole-frame context, where it changes nothing)
    f4 *d_hx_hist_d = nullptr, *d_hx_hist_s = nullptr;   // [H][W], allocated on a row tile only
    float* d_hx_depth = nullptr;
    uint32_t* d_hx_normal = nullptr;
    std::vector<unsigned> hx_row_epoch;
    unsigned hx_epoch = 0;            // vrt_accumulate calls since the opt-in
};

// Device memory is the context's from the moment it exists: vrt_destroy frees whatever is registered, dfree what is given up earlier.
template <class T>
static hipError_t dmalloc(vrt_ctx* c, T** p, size_t bytes) {   // uninitialised
    const hipError_t e = hipMalloc((void**)p, bytes);
    if (e == hipSuccess) c->device_allocs.push_back(*p);
    else *p = nullptr;
    return e;
}
template <class T>
static hipError_t dalloc(vrt_ctx* c, T** p, size_t n) {   // n zeroed elements
    hipError_t e = dmalloc(c, p, n * sizeof(T));
    // hipMemset fills on the NULL stream and may return before the fill has run; the context's streams are non-blocking, so
    // nothing orders a launch queued next (a buffer allocated on its first use: the fused samples' planes) after that fill --
    // it zeroed the first tiles a render launch had just written (seen once the allocator handed back recycled memory:
    // tests/test_gpu_parity.py::test_row_shards_equal_full_frame after the large frames of test_gpu_fullsize.py).  Wait for it.
    if (e == hipSuccess) e = hipMemset(*p, 0, n * sizeof(T));
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    return e;
}
template <class T>
static hipError_t dfree(vrt_ctx* c, T** p) {
    if (!*p) return hipSuccess;
    auto& v = c->device_allocs;
    v.erase(std::remove(v.begin(), v.end(), (void*)*p), v.end());
    const hipError_t e = hipFree(*p);
    *p = nullptr;
    return e;
}

// Queues the accumulation of every render launch whose pass was deferred (vrt_pipeline.hip).  Everything that observes or changes
// what a pass per launch would have produced calls it first.
static int flush_deferred(vrt_ctx* c, bool split_tail = true);
// Lanes of the pipeline in use, and the stream of each.
static int n_lanes(const vrt_ctx* c) { return c->n_streams + (c->ctx_lane ? 1 : 0); }
static hipStream_t lane_stream(const vrt_ctx* c, int lane) { return c->ctx_lane && lane == c->n_streams ? c->stream : c->lanes[lane].stream; }
// The context's stream comes behind every pass and every render launch queued on another lane so far (vrt_ctx::ctx_unsettled).
static int settle_ctx_stream(vrt_ctx* c) {
    if (!c->ctx_unsettled) return VRT_OK;
    if (c->last_pass_ev && lane_stream(c, c->last_pass_lane) != c->stream) HIP_TRY(hipStreamWaitEvent(c->stream, c->last_pass_ev, 0));
    for (int s = 0; s < c->n_streams; s++)   // (launches whose pass is not queued yet: what a caller's upload must not overtake)
        if (c->lanes[s].last_set >= 0) HIP_TRY(hipStreamWaitEvent(c->stream, c->sets[c->lanes[s].last_set].ev_r, 0));
    c->ctx_unsettled = false;
    return VRT_OK;
}
// The preamble of the entry points that look at, or queue work behind, what vrt_accumulate has produced.
static int enter(vrt_ctx* c) {
    HIP_TRY(hipSetDevice(c->device));
    return flush_deferred(c);
}

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Host store to the gate word: every launch queued so far counts as draining.  launch_seq is at least what any launch in
// flight will raise the word to, and later launches raise it further (atomic max), so no wait can be lost.
static void release_gate(vrt_ctx* c) {
    if (!c->drain_signal) return;
    __atomic_store_n(c->drain_signal, (uint32_t)c->launch_seq.next, __ATOMIC_RELEASE);
    c->gate_releases++;
}
// Before a blocking wait for work that may sit behind a gated launch: polls `query` (hipErrorNotReady: not yet) for at most the
// watchdog's time, then releases the gate from the host (harmless when the launches are merely long; the way out when a dispatch
// never comes).  idle(seconds waited so far) is how the caller passes the time between two polls.
template <class Query, class Idle>
static void wait_bounded(vrt_ctx* c, Query query, Idle idle) {
    if (!c->drain_signal || !c->drain_signalled) return;
    const double t0 = now_s();
    while (query() == hipErrorNotReady) {
        const double waited = now_s() - t0;
        if (waited > c->knobs.gate_watchdog_s) { release_gate(c); break; }
        idle(waited);
    }
    (void)hipGetLastError();
}
// The same wait without the flush: for the entry points that read scene data only (vrt_cast_rays, vrt_fetch_voxels) and so leave the
// pending accumulation where it is.
static hipError_t sync_stream_only(vrt_ctx* c, hipStream_t st) {
    wait_bounded(c, [&] { return hipStreamQuery(st); }, [](double) { std::this_thread::yield(); });
    return hipStreamSynchronize(st);
}
// hipStreamSynchronize with that bound on how long a gated launch may hold the stream.
static hipError_t sync_guarded(vrt_ctx* c, hipStream_t st) {
    if (st == c->stream && flush_deferred(c) != VRT_OK) return hipErrorUnknown;   // (the passes the caller is about to wait for)
    wait_bounded(c, [&] { return hipStreamQuery(st); }, [](double waited) {
        // a frame is a millisecond: yield for the first of it (a 50 us sleep overshoots by 50-150 us with the kernel's timer
        // slack, 5-15 % of a fetch-every-frame loop), sleep only through launches that are really long
        if (waited < 2e-3) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(50));
    });
    return hipStreamSynchronize(st);
}
// Host wait for everything queued on the context's streams.
static void drain_all(vrt_ctx* c) {
    for (Lane& l : c->lanes) if (l.stream) (void)hipStreamSynchronize(l.stream);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->fetch_stream) (void)hipStreamSynchronize(c->fetch_stream);
}
