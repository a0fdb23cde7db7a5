// vrt_plan.h -- the launch pipeline's decisions as plain functions over plain values: the environment switches, which render kernel a launch takes, the
// pipeline's shape, how many samples a launch fuses, which launches carry timers, what a dispatch waits for, which copy and stream a launch takes.
// Nothing here knows HIP or vrt_ctx: vrt_pipeline.hip calls these between its HIP calls, tests/emul/plan_emul.cpp calls them on a
// machine without a GPU (tests/test_pipeline_plan_host.py).
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>

#define VRT_MAX_FUSED 4   // samples of one vrt_accumulate(n) call rendered by a single launch
#define VRT_MAX_STREAMS 8 // render launches in flight at most (a stream, a pool scratch and a camera-ray table each): 2, 4 or 8 are used
#define VRT_MAX_SETS 12   // copies of what a render launch writes: streams + 1 are used, or streams + K
                          // where the accumulation of K launches is deferred into one pass (flush_deferred)
#ifndef VRT_DEFER_4DEEP
#define VRT_DEFER_4DEEP 4 // K of the four-deep pipeline (launches of up to 12 M items).  The two-deep one (4K frames: a set is 1 GB there)
#endif                    // and the eight-deep one (not measured with K > 1) accumulate every launch in a pass of its own
#define VRT_MAX_DEFER 8   // largest K a switch may ask for: VRT_MAX_GROUP of vrt_temporal.h (vrt_ctx.h asserts that they agree)
#define VRT_LEAN_STREAMS 2
#ifndef VRT_PRIMARY_DEFAULT
#define VRT_PRIMARY_DEFAULT 1   // Knobs::primary of the shipped library
#endif

// Environment switches, read ONCE when a context is created (never on the launch path).
// The shipped library knows four: VRT_RENDER=pool|fused (which of the two schedules of the same per-path code renders),
// VRT_OVERLAP=0 (isolated launches: what the --pmc passes and the tile balancing of bench.py measure on),
// VRT_GATE_WATCHDOG_MS (how long a synchronisation waits at a gated launch before the host releases the gate) and the HIP
// runtime's own GPU_MAX_HW_QUEUES (how deep a pipeline the runtime's queues carry).
// A build with -DVRT_DEV_KNOBS (build_variants/libvrt_dev.so: `python -m voxel_rt2_amd.build --variant dev -DVRT_DEV_KNOBS`,
// loaded by tests/test_gpu_pipeline.py and the A/B runs of tools/) adds the development switches: the fault-injection hook
// VRT_TEST_FAIL_LAUNCH and the A/B switches VRT_CULL, VRT_DENSE, VRT_DEEP_ITEMS, VRT_DEEPER_ITEMS, VRT_STREAMS, VRT_GRID_DIV,
// VRT_DRAIN_GATE, VRT_FUSE, VRT_FUSE_RESTIR, VRT_OVERLAP_SINGLE, VRT_FULL_BELOW, VRT_CHUNK, VRT_DEFER, VRT_PASS_STREAM, VRT_CTX_LANE, VRT_CAST_VIEW,
// VRT_PREPASS, VRT_PRIMARY, VRT_PRIMARY_CAP; and a second test hook, VRT_TEST_SPOIL_RECORDS=N: every N-th camera-ray record of a pre-pass is made to
// fail its check before anything reads it (k_spoil_primary_records, vrt_kernels.hip), so that the routes for missing and stale records run.
struct Knobs {
    int render = -1;               // -1: the library's choice, 0: fused, 1: pool; -2: a value VRT_RENDER does not know
    bool overlap = true;
    double gate_watchdog_s = 2.0;
    int hw_queues = 4;
    // development switches: the defaults below are what the shipped library always runs with
    int cull = -1, dense = -1;     // -1: decided from the scene (vrt_prepare)
    long long deep_items = (long long)12 << 20, deeper_items = (long long)9 << 19;
    int streams = 0, grid_div = 0; // 0: decided from the frame size (plan_pipeline_shape)
    int pass_stream = -1;          // -1: decided with the pipeline's shape (plan_pipeline_shape), 0: grouped passes on the context's stream, 1: on a render stream
    int ctx_lane = -1;             // -1: decided with the pipeline's shape, 0 / 1: the context's stream is not / is a render lane (where launches can be deferred)
    bool drain_gate = true, fuse_restir = true, overlap_single = true;
    int max_fused = VRT_MAX_FUSED, full_below = 2, chunk = 0, fail_launch = -1, gate_extra = 0, time_every = 0;
    int defer4 = VRT_DEFER_4DEEP, defer8 = 1;   // render launches whose accumulation runs as one pass, per pipeline depth (VRT_DEFER: both)
    int cast_view = -1;            // -1: by the batch size (plan_cast_staged), 0: k_cast_rays on the pyramid in global memory, 1: coarse levels staged in LDS
    int primary = VRT_PRIMARY_DEFAULT;   // plan_primary: 0: no launch has its primary vertices shaded ahead of it, 1: those the rule names
    long long primary_cap = 0;     // plan_primary_caps: continuation records of a launch's queue, all heads together (0: the rule's)
    int prepass = 1;               // plan_prepass: 0: no launch has a pre-pass, 1: those the rule names, 2: the same, queued, but the launch is not told (A/B: what co-residency costs)
#if defined(VRT_DEV_KNOBS)
    int spoil_records = 0;         // VRT_TEST_SPOIL_RECORDS: 0: off, N >= 1: the records whose index is launch number mod N (mod N) are spoiled behind every pre-pass
#endif
};
static Knobs read_knobs() {
    Knobs k;
    if (const char* e = getenv("VRT_RENDER")) k.render = strcmp(e, "fused") == 0 ? 0 : strcmp(e, "pool") == 0 ? 1 : -2;
    if (const char* e = getenv("VRT_OVERLAP")) k.overlap = atoi(e) != 0;
    if (const char* e = getenv("VRT_GATE_WATCHDOG_MS")) { const double v = atof(e); if (v > 0.0) k.gate_watchdog_s = v * 1e-3; }
    if (const char* e = getenv("GPU_MAX_HW_QUEUES")) k.hw_queues = atoi(e);
#if defined(VRT_DEV_KNOBS)
    if (const char* e = getenv("VRT_TEST_FAIL_LAUNCH")) k.fail_launch = atoi(e);
    if (const char* e = getenv("VRT_TEST_SPOIL_RECORDS")) { const int v = atoi(e); if (v >= 1) k.spoil_records = v; }
    if (const char* e = getenv("VRT_CULL")) k.cull = atoi(e) != 0;
    if (const char* e = getenv("VRT_DENSE")) k.dense = atoi(e) != 0;
    if (const char* e = getenv("VRT_DEEP_ITEMS")) k.deep_items = atoll(e);
    if (const char* e = getenv("VRT_DEEPER_ITEMS")) k.deeper_items = atoll(e);
    if (const char* e = getenv("VRT_STREAMS")) { const int v = atoi(e); if (v == 2 || v == 3 || v == 4 || v == 8) k.streams = v; }
    if (const char* e = getenv("VRT_PASS_STREAM")) { const int v = atoi(e); if (v == 0 || v == 1) k.pass_stream = v; }
    if (const char* e = getenv("VRT_CTX_LANE")) { const int v = atoi(e); if (v == 0 || v == 1) k.ctx_lane = v; }
    if (const char* e = getenv("VRT_GRID_DIV")) { const int v = atoi(e); if (v >= 1 && v <= 4) k.grid_div = v; }
    if (const char* e = getenv("VRT_DRAIN_GATE")) k.drain_gate = atoi(e) != 0;
    if (const char* e = getenv("VRT_FUSE")) { const int v = atoi(e); if (v >= 1 && v <= VRT_MAX_FUSED) k.max_fused = v; }
    if (const char* e = getenv("VRT_FUSE_RESTIR")) k.fuse_restir = atoi(e) != 0;
    if (const char* e = getenv("VRT_OVERLAP_SINGLE")) k.overlap_single = atoi(e) != 0;
    if (const char* e = getenv("VRT_TIME_EVERY")) { const int v = atoi(e); if (v >= 1 && v <= 1024) k.time_every = v; }   // 0 (default): by launch size
    if (const char* e = getenv("VRT_GATE_EXTRA")) { const int v = atoi(e); if (v >= 0 && v <= 4) k.gate_extra = v; }
    if (const char* e = getenv("VRT_FULL_BELOW")) { const int v = atoi(e); if (v >= 0 && v <= 3) k.full_below = v; }   // 0: no overlapped launch takes every slot, whatever the host's timing (tests)
    if (const char* e = getenv("VRT_DEFER")) { const int v = atoi(e); if (v >= 0 && v <= VRT_MAX_DEFER) k.defer4 = k.defer8 = v < 1 ? 1 : v; }   // 0, 1: a pass per launch
    if (const char* e = getenv("VRT_CHUNK")) { const int v = atoi(e); if (v >= 64 && v <= 4096) k.chunk = v / 64 * 64; }
    if (const char* e = getenv("VRT_PRIMARY")) { const int v = atoi(e); if (v == 0 || v == 1) k.primary = v; }
    if (const char* e = getenv("VRT_PRIMARY_CAP")) { const long long v = atoll(e); if (v >= 8) k.primary_cap = v; }
    if (const char* e = getenv("VRT_PREPASS")) { const int v = atoi(e); if (v >= 0 && v <= 2) k.prepass = v; }
    if (const char* e = getenv("VRT_CAST_VIEW")) k.cast_view = strcmp(e, "staged") == 0 ? 1 : strcmp(e, "global") == 0 ? 0 : -1;
#endif
    return k;
}

// Which instantiation of the render kernel a launch takes, decided HERE and nowhere else.  vrt_api.hip fills the inputs from the context
// (render_inputs); vrt_kernels.hip maps the result to a kernel: k_render<G, restir, instr> on the fused schedule; on the pooled one
// (pool_kernel) k_render_pool_restir<G, instr, cull>, else with dense12 k_render_pool_dense12<G, instr, cull>, else
// k_render_pool<G, instr, black_sun, cull>.
struct RenderInputs {
    int width, height, max_depth, knob_render, knob_cull;     // (Knobs::render, Knobs::cull)
    bool use_restir, instrumented, count_as_timed, ref_oob;   // vrt_set_instrumented, vrt_set_reference_indexing
    bool cull_active, dense_grid, light_emits;                // the scene's (vrt_prepare); a colour component of the light is non-zero and so is its weight
    int fused;                                                // samples the launch renders (plan_fused_count)
};
struct RenderVariant {
    bool pooled, restir;  // the pooled schedule (vrt_pool.h), not the fused one (vrt_path.h); ReSTIR runs on either
    bool instr;           // counts the reference's work; also the instantiations that carry the reference's out-of-grid reading
    bool cull;            // rays that cannot hit a voxel are not walked (cull_ray, vrt_trace.h): sc.cull is the scene's box, not the open one
    bool black_sun;       // scene.py's default light: the light sample is compiled out of the shading stage
    bool dense12;         // the twelve-wave geometry of a dense grid under an emitting sun; also `heavy` of plan_pipeline_shape
    bool share_primary;   // fused samples share their camera rays through a per-pixel table (vrt_pool.h)
};
static inline RenderVariant plan_render_variant(const RenderInputs& in) {
    RenderVariant v;
    // the pooled kernel packs pixel coordinates in 12 bits and the depth in 4; VRT_RENDER=fused: A/B measurements, tests
    v.pooled = in.width <= 4096 && in.height <= 4096 && in.max_depth <= 15 && in.knob_render != 0;
    v.restir = in.use_restir;
    v.instr = in.instrumented || in.ref_oob;
    // launches that count the reference's work walk every ray, as the reference and the oracle do; with the reference's indexing a
    // ray clear of every solid voxel can still "hit" outside the grid: every ray is walked; VRT_CULL=0 for A/B runs
    v.cull = in.cull_active && !(in.instrumented && !in.count_as_timed) && !in.ref_oob && in.knob_cull != 0;
    v.black_sun = !in.light_emits;
    v.dense12 = v.pooled && !v.restir && in.dense_grid && !v.black_sun;   // (with a black sun SHADE walks next to no shadow rays)
    v.share_primary = v.pooled && in.fused > 1 && (!v.instr || in.count_as_timed);   // (counting the reference's work: every camera ray is walked)
    return v;
}

// Whether a launch is preceded by the pre-pass that leaves its camera-ray records (k_primary_records, vrt_kernels.hip), and whether
// the launch is told so.  The pre-pass is a lean kernel for the wave slot that two pooled waves of 208 registers leave empty on a
// SIMD; it is queued on the launch's own lane, where it runs while the launches of the other lanes hold the heavy slots.  So only
// launches that have such neighbours and such a slot: overlapped ones of half the slots (grid_div 2: the four-deep pipeline and the
// queue-lean shapes, with or without the context's stream as a lane) that do not find the pipeline empty (`lone`: they take every
// slot), whose samples share the record table, and not the twelve-wave geometry (its three waves leave no registers).  Launches
// that count the reference's work walk every camera ray themselves.  Everything else -- lone launches, the two-deep 4K mode, the
// eight-deep small-launch mode, ReSTIR, one-sample calls -- is queued as it was.  knob: Knobs::prepass.
struct Prepass { bool queue, tell; };
static inline Prepass plan_prepass(const RenderVariant& v, bool overlapped, bool lone, int grid_div, int knob) {
    Prepass p;
    p.queue = knob != 0 && overlapped && !lone && grid_div == 2 && v.pooled && v.share_primary && !v.instr && !v.dense12 && !v.restir;
    p.tell = p.queue && knob != 2;
    return p;
}
// Whether a launch's primary vertices are shaded ahead of it (k_primary_vertex, vrt_kernels.hip; vrt_primary.h) and the launch resumes
// its paths from the queue that kernel leaves (the QUEUED instantiation): exactly the launches that have a pre-pass and are told of it
// -- the kernel reads the pre-pass's records.  (It does not share the pre-pass's wave slot: at 160 registers it fits beside one pooled
// wave of a SIMD, not two, and runs where a draining launch has freed slots.)  knob: Knobs::primary.
static inline bool plan_primary(const Prepass& pre, int knob) { return knob != 0 && pre.queue && pre.tell; }
// The queue of such a launch over `tiles` 8x8 tiles of n_samples samples, per work head (8 of them; tile t appends to head t % 8).
// left_cap: every item of the head's tiles -- a leftover can always be written, so no path is dropped.  cap: continuation records; a
// path that finds them used up becomes a leftover and is begun by the pool from depth 0, the same bits.  Three eighths of the
// items: of the path-samples a tenth (sun-lit) to a quarter (S1) go on in the small frames of tests/test_gpu_primary_vertex.py and
// 20.7 % on the 1080p headline (the development build's report over a bench run) -- a quarter would leave a head
// with a few more continuing paths than the average nothing to spare; the overflow route is exact but costs the pool a depth-0 turn.
// 64 bytes a record under a black sun, 96 under an emitting one: a 1080p launch of four samples holds 3.1 M records -- 199 MB
// (299 MB) a lane -- and 33 MB of leftover words.  A queue that has to grow (a later launch with
// more tiles or samples) is reallocated behind a host wait for the lane's stream: once, on the launch path.
// knob_cap: Knobs::primary_cap, records of all heads together (tests force 64).
struct PrimaryCaps { unsigned cap, left_cap; };
static inline PrimaryCaps plan_primary_caps(unsigned tiles, int n_samples, long long knob_cap) {
    PrimaryCaps c;
    c.left_cap = ((tiles + 7u) / 8u) * 64u * (unsigned)n_samples;
    c.cap = knob_cap > 0 ? (unsigned)(knob_cap / 8) : (unsigned)((3ull * c.left_cap + 7ull) / 8ull);
    if (c.cap > c.left_cap) c.cap = c.left_cap;
    return c;
}
// What is queued on an overlapped launch's lane ahead of the launch itself, in order.  The pre-pass first (it waits for nothing but the
// lane's previous launch); the wait for the pass that last read the copy the launch writes; then, with plan_primary, the zeroing of
// the queue's counts and k_primary_vertex, which writes that copy and is no pooled launch, so not the gate's business; the dispatch gate last, right in front of
// the pooled launch.  wait_pass: such a pass is on record; wait_gate: plan_gate_wait.
enum LaneOp { LANE_OP_PREPASS = 0, LANE_OP_WAIT_PASS, LANE_OP_ZERO_QUEUE, LANE_OP_PRIMARY_VERTEX, LANE_OP_WAIT_GATE, LANE_OP_COUNT };
static inline int plan_lane_ops(const Prepass& pre, bool primary, bool wait_pass, bool wait_gate, LaneOp* ops) {
    int n = 0;
    if (pre.queue) ops[n++] = LANE_OP_PREPASS;
    if (wait_pass) ops[n++] = LANE_OP_WAIT_PASS;
    if (primary && pre.queue && pre.tell) { ops[n++] = LANE_OP_ZERO_QUEUE; ops[n++] = LANE_OP_PRIMARY_VERTEX; }
    if (wait_gate) ops[n++] = LANE_OP_WAIT_GATE;
    return n;
}
// The launch numbers.  A launch takes the next number when it is queued (plan_seq_take); its records carry the number as their tag
// (+ 1), and a tag must never come to mean two launches -- a launch with another camera would take the first one's records for its
// own.  A pre-pass is queued AHEAD of its launch and is handed the number the launch will take (plan_seq_reserve); if the launch is
// then not queued after all (a queue operation between the two failed: abort_pipeline), plan_seq_abort burns the number.
struct LaunchSeq { unsigned next = 0; bool reserved = false; };
static inline unsigned plan_seq_reserve(LaunchSeq& s) { s.reserved = true; return s.next; }
static inline unsigned plan_seq_take(LaunchSeq& s) { s.reserved = false; return s.next++; }
static inline void plan_seq_abort(LaunchSeq& s) { if (s.reserved) { s.next++; s.reserved = false; } }

// How deep a launch of `items` work items (pixels x fused samples) wants the pipeline.  A launch lasts at least as long as its
// deepest path takes alone (about 0.2 ms at 8 bounces), whatever its size, and a workgroup slot its wave has left stays empty
// until the NEXT launch may start.
// A launch of every slot can only be followed when it starts to drain (two in flight).  Launches of half the slots each follow
// one another at half that distance -- two run at full strength while a third drains and a fourth waits its turn.  Measured
// (profiles/r02_pipeline_depth.txt): 1080p x 4 samples +3.7 %, half of it +5 %, an eighth (one rank's rows of an 8-GPU
// run) +24 %; thirds and quarters of the slots are worse again; a 4K frame (33 M items a launch) loses 0-7 % and keeps
// the two-deep pipeline.
// Deeper still for the smaller launches -- one rank's rows of an 8-GPU split of 1080p are 1 M items: eight launches of a
// quarter of the slots each (+7.5 % on those rows; with the timers thinned out, below: +2 % on half a frame of 4.1 M items,
// +17 % on its cheap upper 480 rows, -2 % on a whole frame, -9 % on the sun-lit one: the limit is 4.5 M items).  Each render stream wants a
// hardware queue of its own (two streams on one queue serialise), so only where the runtime was started with sixteen
// (GPU_MAX_HW_QUEUES, which voxel_rt2_amd/_lib.py sets unless the user has).
// VRT_DEEP_ITEMS / VRT_DEEPER_ITEMS (development build): largest launch (pixels x fused samples) of each kind; VRT_STREAMS /
// VRT_GRID_DIV override.
// The queue-lean shape.  The four-deep pipeline keeps five streams busy (four render streams and the context's, which carries the
// grouped passes) beside the runtime's null stream.  A runtime with four hardware queues places them on three: two render
// streams share one queue and the context's stream shares another with a third (profiles/r06_a_queues_q4.txt: the queue ids of
// the kernel trace), and a launch then sits behind the stream wait or the pass of a stream it has nothing to do with (-7 %
// against sixteen queues).  With fewer queues than streams the same launches -- half the slots each, two running at any time, one
// pass per K launches -- go to TWO render streams: launch k follows launch k - 2 in stream order, which says what the dispatch
// gate would (plan_gate_wait leaves the stream wait out), and two render streams and the context's stream have a queue each.
// Launch k then starts when launch k - 2 has completed, not when it begins to drain: 3.3 % slower than four streams where the
// queues are there (sixteen: 8 923-8 958 against 9 205-9 259), 4.5 % faster where they are not (four: 8 913-8 955 against
// 8 547-8 572).  Three render streams lose a quarter at four queues with the pass on either stream (two of them share a queue:
// 6 650-6 750), the pass on a render stream loses 2.6 % with two (it holds that stream's next launch back: 8 715-8 720) and
// changes nothing with four (profiles/r06_a_shapes.txt).
// The context's stream as a third lane.  In the queue-lean shape the context's stream has a queue to itself and carries one pass per
// K launches.  ctx_lane makes it the lane behind the library's own streams: launches take turns over n_streams + 1 lanes on as many
// queues, launch k waits for launch k - 2's drain signal (the dispatch gate, as with four streams) instead of its completion, and the
// grouped pass runs on the lane of the group's last launch, whose next launch is a whole round away.  Only where every launch is
// deferred (a pass per launch would put every pass in front of the context's stream's own launches), and not beside a forced shape
// (VRT_STREAMS, VRT_GRID_DIV, VRT_PASS_STREAM measure the shapes above as they were measured); VRT_CTX_LANE=0|1 overrides both
// for A/B runs, VRT_PASS_STREAM=0 then keeps every pass on the context's stream.
struct PipelineShape {
    int n_streams;         // depth of the launch pipeline: 2, 4 with launches of half the workgroup slots each, or 8 with quarters
    int grid_div;          // an overlapped launch takes render_blocks / grid_div workgroups
    bool pass_on_render;   // grouped passes run on a render stream (development switch VRT_PASS_STREAM=1: measured, not faster in any shape)
    int defer_k;           // K: render launches whose accumulation runs as one pass (1: every launch has a pass of its own)
    bool ctx_lane;         // the context's stream is render lane number n_streams: n_streams + 1 lanes, n_streams streams of the pipeline's own
    bool pass_on_last;     // grouped passes run on the lane of the group's last launch: pass_on_render, or ctx_lane unless VRT_PASS_STREAM=0
};
static inline PipelineShape plan_pipeline_shape(size_t items, bool heavy, int hw_queues, bool can_defer, const Knobs& knobs) {
    // (heavy: the dense-grid kernel -- six rays a path instead of two: an item is about twice the work, a rank's 4.1 M items of an
    // 8-way split of a dense 4K frame lose 10 % in the eight-deep pipeline that the same number of S1's items gain 2-17 % from)
    const bool deep = items <= (size_t)knobs.deep_items;                                                       // 12 M
    const bool deeper = deep && items * (heavy ? 2u : 1u) <= (size_t)knobs.deeper_items && hw_queues >= 16;    // 4.5 M
    const bool lean = deep && !deeper && hw_queues < 4 + 2;   // (the render streams, the context's stream, the null stream)
    PipelineShape sh;
    sh.n_streams = deeper ? 8 : deep ? (lean ? VRT_LEAN_STREAMS : 4) : 2;
    sh.grid_div = deeper ? 4 : deep ? 2 : 1;
    sh.pass_on_render = false;
    if (knobs.streams) sh.n_streams = knobs.streams;
    if (knobs.grid_div) sh.grid_div = knobs.grid_div;
    if (knobs.pass_stream >= 0) sh.pass_on_render = knobs.pass_stream != 0;
    // K of the mode: contexts whose launches are never deferred (can_defer) do not pay for the copies
    const int ns = sh.n_streams;
    int k = !can_defer ? 1 : (ns == 4 || (ns < 4 && sh.grid_div == 2)) ? knobs.defer4 : ns == 8 ? knobs.defer8 : 1;
    if (k > VRT_MAX_SETS - ns) k = VRT_MAX_SETS - ns;
    sh.defer_k = k < 1 ? 1 : k;
    sh.ctx_lane = lean && can_defer && !knobs.streams && !knobs.grid_div && knobs.pass_stream < 0;
    if (knobs.ctx_lane >= 0) sh.ctx_lane = knobs.ctx_lane != 0 && can_defer;
    if (sh.defer_k < 2 || ns + 1 > VRT_MAX_STREAMS) sh.ctx_lane = false;
    if (sh.ctx_lane && sh.defer_k > VRT_MAX_SETS - ns - 1) sh.defer_k = VRT_MAX_SETS - ns - 1;
    sh.pass_on_last = sh.pass_on_render || (sh.ctx_lane && knobs.pass_stream != 0);
    return sh;
}

// Samples the next launch of a vrt_accumulate(n) call renders, `left` of them still to go.
static inline int plan_fused_count(int left, bool can_fuse, int max_fused) {
    return (can_fuse && left > 1) ? (left < max_fused ? left : max_fused) : 1;
}

// Timers (two events around each kernel, vrt_stats' device times) cost a short step its rate: the barrier packets they put
// around the kernel sit in the chain from one launch's drain to the next one's first wave -- a fixed 30-40 us of a step,
// 3-25 % of the steps of 0.15-0.3 ms that a rank's rows of an 8-GPU split or the reference's one-sample calls take, nothing
// of a 1 ms step.  What a step will take is not known when it is queued, its size is: launches of the deep pipelines (up to 12 M
// work items, ReSTIR off) carry timers one time in eight; vrt_get_stats scales the timed launches' sum to all of them.
static inline unsigned plan_timer_period(int time_every, bool restir, size_t items, long long deep_items) {
    return time_every > 0 ? (unsigned)time_every : ((!restir && items <= (size_t)deep_items) ? 8u : 1u);
}

// The value of the drain signal that launch number `launch_seq` is dispatched at.  Dispatch when the launch whose workgroup slots
// this one will take starts to drain: the one before it, or with launches of half the slots the one before that (the signal
// carries the number + 1 of the latest launch draining) -- unless the one before it took EVERY slot (a lone launch): then that
// one has to drain first; and never for a launch OLDER than the last one that took every slot: until that one drains there is no
// slot at all.  0: nothing to wait for.
static inline unsigned plan_gate_target(unsigned launch_seq, bool prev_launch_full, int grid_div, int gate_extra, unsigned last_full_seq) {
    const unsigned back = prev_launch_full ? 1u : (unsigned)(grid_div + gate_extra);
    const unsigned target = launch_seq + 1u > back ? launch_seq + 1u - back : 0u;
    return target < last_full_seq ? last_full_seq : target;
}
// Whether the stream wait for `target` is queued at all.  (A launch already on this stream that is the target or newer has raised
// the word by the time this one's turn comes: stream order says what the wait would.)
static inline bool plan_gate_wait(unsigned target, unsigned lane_last_seq, bool gate_present, bool signalled) {
    return gate_present && signalled && target > 0u && lane_last_seq < target;
}

// Workgroups of a launch that shares the chip with others: its part of the slots, in whole rounds of the 8 XCDs.
static inline int plan_partial_blocks(int all_blocks, int grid_div) { return (all_blocks / grid_div + 7) & ~7; }

// Which copy overlapped launch number `pipe_seq` writes, and which render stream (and pool scratch) it goes to: consecutive
// launches take turns.
static inline int plan_set_of(unsigned pipe_seq, int n_sets) { return (int)(pipe_seq % (unsigned)n_sets); }
static inline int plan_lane_of(unsigned pipe_seq, int n_lanes) { return (int)(pipe_seq % (unsigned)n_lanes); }

// ---- vrt_cast_rays (its two rules of thumb also serve the sampled queries, below) ------------------------------------------------
// Which view of the pyramid a batch of n rays is walked on: the coarse levels staged in LDS once per workgroup (k_render's
// LdsPyramid), or everything through global memory.  Staging is 4 KiB + 64 B a workgroup at 128^3 and 32.5 KiB at 256^3: a cost per
// WORKGROUP, which a grid sized from the CU count pays a bounded number of times, but which a pick of one ray or a fan of a few
// hundred pays in full for next to no walking.  VRT_CAST_STAGED_MIN is meant to be where the two curves of tools/cast_rate.py cross on s1;
// that tool has not run on an MI355X yet, so 4096 -- sixteen workgroups' worth of rays -- is PROVISIONAL.  Results do
// not depend on it (both instantiations give the same bytes: tests/test_gpu_cast_rays.py).  `knob`: Knobs::cast_view.
#ifndef VRT_CAST_STAGED_MIN
#define VRT_CAST_STAGED_MIN 4096
#endif
static inline bool plan_cast_staged(long long n, int knob) { return knob >= 0 ? knob != 0 : n >= VRT_CAST_STAGED_MIN; }
// Rays a host-path call stages at a time (80 bytes of device memory a ray: the batch size is limited by the caller's memory only).
static inline long long plan_cast_chunk() { return 1 << 18; }
// Workgroups of a launch over n rays, 256 rays a workgroup per turn of its loop: no more than fit on the chip at once.
static inline int plan_cast_blocks(long long n, int n_cu, int blocks_per_cu) {
    const long long want = (n + 255) / 256, fit = (long long)n_cu * (blocks_per_cu > 0 ? blocks_per_cu : 1);
    return (int)(want < fit ? want : fit);
}

// ---- vrt_sweep_boxes ------------------------------------------------------------------------------------------------------------------
// Boxes a host-path call stages at a time (80 bytes of device memory a box, as a ray: the batch size is limited by the caller's memory only).
static inline long long plan_sweep_chunk() { return 1 << 18; }
// Workgroups of a launch over n boxes: a wave of 64 lanes a box, so four boxes a workgroup of 256 per turn of its loop, and no more
// workgroups than fit on the chip at once (plan_cast_blocks' rule with 4 in the place of 256).
#define VRT_SWEEP_BOXES_PER_BLOCK 4
static inline int plan_sweep_blocks(long long n, int n_cu, int blocks_per_cu) {
    const long long want = (n + VRT_SWEEP_BOXES_PER_BLOCK - 1) / VRT_SWEEP_BOXES_PER_BLOCK, fit = (long long)n_cu * (blocks_per_cu > 0 ? blocks_per_cu : 1);
    return (int)(want < fit ? want : fit);
}

// ---- vrt_voxelize_triangles ----------------------------------------------------------------------------------------------------------
// Triangles a host-path call stages at a time (48 bytes of device memory each), and triangles one set-up + rasterise pair of launches
// takes on either path (16 bytes of item-list entry each): n is limited by the caller's memory only.
static inline long long plan_voxelize_chunk() { return 1 << 18; }
static inline long long plan_voxelize_batch() { return 1 << 20; }
// Items (16^3 cells of a triangle, vrt_voxelize.h) a wave reserves per atomic on the work head: few enough that the 4096 items of a
// grid-spanning triangle spread over 1024 waves (an item through the triangle's plane is some twenty bricks of 64 voxel tests: a grab
// of them is the tail a lone large triangle adds to a call), enough that the search for an item's triangle is paid once per four items.
#define VRT_VOX_ITEMS_PER_GRAB 4
// Workgroups of the rasterise launch: a persistent grid of four waves a workgroup, eight workgroups a CU -- the item count is known
// on the device only, and a wave that finds the head exhausted ends at once.
static inline int plan_voxelize_blocks(int n_cu) { return (n_cu > 0 ? n_cu : 1) * 8; }
// The context's triangle-edit scratch (vrt_ctx::d_vox), cut up for a box of nv voxels, a head region of head_bytes and batches of at most
// `batch` triangles.  The head is what the call's raster kernel writes: vrt_voxelize_triangles' ownership words (4 * nv bytes) or
// vrt_fill_triangles' toggle words (4 * fill_words: one bit a voxel, a column rounded up to whole 32-bit words).  Behind it the box
// arrays handed to launch_edit (head and materials padded to 256 bytes), the item-list entries (16 bytes a triangle, on a multiple of
// 16), and 256 bytes for the two heads and the result record.  (The surface pass used to put box_mat at 4 * nv unrounded, and both
// calls the entries on a multiple of 256: this moves the regions by at most 255 bytes, never makes the buffer more than 255 bytes
// larger, and changes no result -- nothing but these offsets says where a region is.)
struct TriLayout { size_t mat_at, rgb_at, entries_at, heads_at, bytes; };
static inline TriLayout plan_tri_layout(size_t head_bytes, size_t nv, size_t batch) {
    const auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    TriLayout l;
    l.mat_at = up(head_bytes);
    l.rgb_at = l.mat_at + up(nv);
    l.entries_at = (l.rgb_at + 3 * nv + 15) & ~(size_t)15;
    l.heads_at = l.entries_at + 16 * batch;
    l.bytes = l.heads_at + 256;
    return l;
}

// ---- vrt_fill_triangles -----------------------------------------------------------------------------------------------------------------
// Chunks and batches are vrt_voxelize_triangles' (plan_voxelize_chunk, plan_voxelize_batch), and so is the persistent grid
// (plan_voxelize_blocks): the item count is known on the device only.  An item here is a tile of 16 x 16 columns (vrt_fill.h), four
// column tests and at most four divisions a lane -- an order of magnitude lighter than the surface pass's 16^3 cell, so the tail a
// grab leaves on one wave matters less and the search for an item's triangle more: a grid-spanning triangle's 256 items are 32 grabs.
#define VRT_FILL_ITEMS_PER_GRAB 8

// ---- vrt_distance_field (vrt_distance.h) ------------------------------------------------------------------------------------------------
// Tile shapes.  Pass z: a workgroup of 256 threads stages VRT_DIST_Z_LINES whole lines (consecutive in memory: z fastest, then y) in LDS,
// padded to 257 words a line, and a thread works output elements 256 apart.  Passes y and x: a workgroup stages a tile of
// VRT_DIST_LANES adjacent lines -- adjacent in memory, so every row of the tile is one coalesced segment -- as [entry][lane], at most
// 256 x 32 x 4 = 32 KB; its 256 threads are VRT_DIST_LANES lanes x VRT_DIST_GROUPS groups, a group working every eighth output entry.
#define VRT_DIST_Z_LINES 8
#define VRT_DIST_Z_PITCH 257
#define VRT_DIST_LANES 32
#define VRT_DIST_GROUPS 8
// The scratch of one call, cut up: A int32[gx][gy][bz] (pass z's result), B int32[gx][by][bz] (pass y's); with `nearest` the chosen
// coordinates cz uint8[gx][gy][bz] and cy uint8[gx][by][bz]; on the host path the staged results d2 and nearest int32[bx][by][bz].
// gx, gy: the grown box's extent; bx, by, bz: the box's.  At most 10 bytes per voxel of the grown box plus 8 per voxel of the box.
struct DistLayout { size_t a_at, b_at, cz_at, cy_at, d2_at, nearest_at, bytes; };
static inline DistLayout plan_distance_layout(size_t gx, size_t gy, size_t bx, size_t by, size_t bz, bool nearest, bool staged) {
    const auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    DistLayout l;
    l.a_at = 0;
    l.b_at = up(l.a_at + 4 * gx * gy * bz);
    l.cz_at = up(l.b_at + 4 * gx * by * bz);
    l.cy_at = up(l.cz_at + (nearest ? gx * gy * bz : 0));
    l.d2_at = up(l.cy_at + (nearest ? gx * by * bz : 0));
    l.nearest_at = up(l.d2_at + (staged ? 4 * bx * by * bz : 0));
    l.bytes = up(l.nearest_at + (staged && nearest ? 4 * bx * by * bz : 0)) + 256;
    return l;
}

// ---- vrt_label_components (vrt_label.h) -------------------------------------------------------------------------------------------------
// The tile a workgroup of k_label_tile solves in LDS, cut from the box's own corner: memory is z-fastest, so the long edge is z and a
// wave's 64 lanes sit on 64 consecutive z -- one coalesced 64-byte segment of material bytes, 64 consecutive LDS words.  8 x 8 x 64
// cells are 16 KB of int32: three workgroups a CU's LDS, and a quarter of a tile's cells lie on a face the seam pass must visit.
#define VRT_LABEL_TX 8
#define VRT_LABEL_TY 8
#define VRT_LABEL_TZ 64
#define VRT_LABEL_TILE (VRT_LABEL_TX * VRT_LABEL_TY * VRT_LABEL_TZ)
// The scratch of one call: the union-find works in the output array itself, so the context holds the counter words only -- laid out
// as the 16-byte result record (members, roots, 0), which k_label_finish adds to -- and on the host path the staged labels
// int32[bx][by][bz] behind them: 4 bytes per box cell plus the record.
struct LabelLayout { size_t result_at, labels_at, bytes; };
static inline LabelLayout plan_label_layout(size_t nv, bool staged) {
    LabelLayout l;
    l.result_at = 0;
    l.labels_at = 256;
    l.bytes = l.labels_at + (staged ? (4 * nv + 255) & ~(size_t)255 : 0);
    return l;
}

// ---- the sampled queries: vrt_trace_radiance, vrt_gather_irradiance, vrt_gather_probes (vrt_query.h) ----------------------------------------------------
// The work item is (record, sample) -- (ray, sample) or (sensor, sample); a finished item leaves its value in a scratch plane -- 12 bytes
// an item for a radiance, a 32-byte vrt_irradiance record of four terms for a sensor -- which k_fold_query sums per record in sample
// order.  The plane is bounded: a call is cut into blocks of records, and a block's samples into chunks of WHOLE samples (every record of
// the block, samples [s0, s0 + count)), so that no launch has more items than the query's cap -- 12 MiB of scratch, whatever n and
// n_samples are.  The sums are carried in `out` from chunk to chunk in sample order (query_fold, vrt_query.h), so the cut cannot change a
// bit of the result (tests/test_radiance_host.py, tests/test_sensor_host.py and their GPU twins).  The sensors' cap is the same BYTES as
// the radiances' (the two queries run on one stream and share the allocation): 12 MiB / 32 = 393 216 items a launch.
// Which view of the pyramid a launch of `items` items walks on is plan_cast_staged's rule on the number of items (a path is several
// walks, so staging pays no later than it does for single rays); its workgroups are plan_cast_blocks' over the items.
#define VRT_RADIANCE_ITEMS (1 << 20)
#define VRT_SENSOR_ITEM_BYTES 32
#define VRT_SENSOR_ITEMS ((VRT_RADIANCE_ITEMS * 12) / VRT_SENSOR_ITEM_BYTES)
// The probes' item is the 48-byte ProbeItem (vrt_probe_sh.h) -- the fold forms the 27 products, the plane does not hold them -- so the same
// bytes hold 12 MiB / 48 = 2^18 items: exactly one sample of a full block (plan_query_rays), which is the least plan_query_chunk needs.
#define VRT_PROBE_ITEM_BYTES 48
#define VRT_PROBE_ITEMS ((VRT_RADIANCE_ITEMS * 12) / VRT_PROBE_ITEM_BYTES)
// Records of a block (also what a host-path call stages at a time: 48 bytes of device memory a ray, 64 a sensor): one sample of a block
// fits either plane.
static inline long long plan_query_rays(long long n) { return n < (1 << 18) ? n : (1 << 18); }
// Whole samples of a chunk over a block of n records (1 <= n <= plan_query_rays' bound) under a cap of `cap` items a launch, n_samples to
// do in all: at least 1.
static inline int plan_query_chunk(long long cap, long long n, int n_samples) {
    const long long fit = cap / (n > 0 ? n : 1);
    return (int)(fit < 1 ? 1 : fit < n_samples ? fit : n_samples);
}
// The two queries' own names for the rules above, as the host emulations' exported entry points are defined (radiance_emul_chunk,
// sensor_emul_rays and the like: tests/emul/).
static inline long long plan_radiance_rays(long long n) { return plan_query_rays(n); }
static inline int plan_radiance_chunk(long long n_rays, int n_samples) { return plan_query_chunk(VRT_RADIANCE_ITEMS, n_rays, n_samples); }
static inline bool plan_radiance_staged(long long items, int knob) { return plan_cast_staged(items, knob); }
static inline long long plan_sensor_rays(long long n) { return plan_query_rays(n); }
static inline int plan_sensor_chunk(long long n_sensors, int n_samples) { return plan_query_chunk(VRT_SENSOR_ITEMS, n_sensors, n_samples); }
static inline long long plan_probe_rays(long long n) { return plan_query_rays(n); }
static inline int plan_probe_chunk(long long n_probes, int n_samples) { return plan_query_chunk(VRT_PROBE_ITEMS, n_probes, n_samples); }
