// vrt_pipeline.hip -- launch sequencing: vrt_accumulate, the overlapped render pipeline, deferred accumulation, the timers.
// A part of vrt_api.hip's translation unit (#included there behind the context and the helpers both use, not compiled by itself),
// so that everything here stays static.  The decisions are vrt_plan.h's; this file queues what they say.

// ---- device timers -----------------------------------------------------------------------------------------------------------
static void account(vrt_ctx* c, const EventPair& ev) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) { c->timed_ms[ev.kind] += ms; c->timed_n[ev.kind] += ev.weight; }
    hipEventDestroy(ev.a);
    hipEventDestroy(ev.b);
}
static void resolve_events(vrt_ctx* c) {   // waits for every launch timed so far
    for (auto& ev : c->pending)
        if (hipEventSynchronize(ev.b) == hipSuccess) account(c, ev);
        else { hipEventDestroy(ev.a); hipEventDestroy(ev.b); }
    c->pending.clear();
}
// On the launch path: the timers of launches that HAVE completed are read and freed, nothing is waited for (a wait here would
// empty the launch pipeline every hundred calls); a caller that never synchronises is held to 4096 outstanding timers.
static void resolve_completed(vrt_ctx* c) {
    if (c->pending.size() > 4096) { resolve_events(c); return; }
    size_t done = 0;
    while (done < c->pending.size() && hipEventQuery(c->pending[done].b) == hipSuccess) { account(c, c->pending[done]); done++; }
    (void)hipGetLastError();   // (hipErrorNotReady is the expected answer at the first launch still running)
    c->pending.erase(c->pending.begin(), c->pending.begin() + (long)done);
}
// The timer bracket of one kernel: timer_begin before it is queued on `st`, timer_end behind it.  Nothing happens unless `timed`.
struct Timer { hipEvent_t b = nullptr; hipStream_t st = nullptr; };
static int timer_begin(vrt_ctx* c, Timer* t, bool timed, int kind, hipStream_t st, unsigned weight = 1u) {
    *t = Timer{};
    if (!timed) return VRT_OK;
    hipEvent_t a = nullptr;
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&t->b));
    c->pending.push_back(EventPair{a, t->b, kind, weight});
    t->st = st;
    HIP_TRY(hipEventRecord(a, st));
    return VRT_OK;
}
static int timer_end(const Timer& t) {
    if (t.b) HIP_TRY(hipEventRecord(t.b, t.st));
    return VRT_OK;
}

// ---- the overlapped pipeline: streams, copies, the dispatch gate -------------------------------------------------------------
// True when a stream wait queued BEFORE the operation that satisfies it (on another render stream) completes: the
// order in which a launch and the wait of its successor can reach the hardware.  Under a tool that serialises queue
// operations it does not -- then the word is released from the host and the caller leaves the gate out.
static bool gate_self_test(vrt_ctx* c) {
    hipStream_t s0 = c->lanes[0].stream, s1 = c->lanes[1].stream;
    if (hipStreamWaitValue32(s1, c->drain_signal, 1u, hipStreamWaitValueGte, 0xFFFFFFFFu) != hipSuccess) { (void)hipGetLastError(); return false; }
    bool wrote = hipStreamWriteValue32(s0, c->drain_signal, 1u, 0) == hipSuccess;
    bool by_itself = false;
    const double t0 = now_s();
    while (wrote && now_s() - t0 < 0.1) {
        if (hipStreamQuery(s1) == hipSuccess) { by_itself = true; break; }
        std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
    (void)hipGetLastError();
    if (!by_itself) __atomic_store_n(c->drain_signal, 1u, __ATOMIC_RELEASE);
    (void)hipStreamSynchronize(s1);
    (void)hipStreamSynchronize(s0);
    __atomic_store_n(c->drain_signal, 0u, __ATOMIC_RELEASE);
    (void)hipGetLastError();
    return by_itself;
}

// Streams, copies and events for a pipeline `want` launches deep (what a shallower one already has is kept; every buffer is
// looked at by itself, so an attempt that failed half way is completed, not allocated over).
static bool grow_pipeline(vrt_ctx* c, int want, int want_sets, bool ctx_lane) {
    const size_t n = c->npix;
    bool ok = true;
    for (int s = 1; s < want_sets && ok; s++) {
        PlaneSet& p = c->sets[s];
        ok = (p.multi_d || dalloc(c, &p.multi_d, n * VRT_MAX_FUSED) == hipSuccess) && (p.spec_planes || dalloc(c, &p.spec_planes, n * VRT_MAX_FUSED) == hipSuccess) &&
             (p.refl_planes || dalloc(c, &p.refl_planes, n * VRT_MAX_FUSED) == hipSuccess) && (p.gb_pos || dalloc(c, &p.gb_pos, n) == hipSuccess) &&
             (p.gb_mat || dalloc(c, &p.gb_mat, n) == hipSuccess);
    }
    for (int s = 0; s < want && ok; s++) {   // stream s and, beyond the first, a pool scratch of its own
        Lane& l = c->lanes[s];
        if (l.stream) continue;
        ok = (s == 0 || l.pool_scratch || dmalloc(c, &l.pool_scratch, c->pool_scratch_bytes) == hipSuccess) &&
             hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking) == hipSuccess;
    }
    if (ctx_lane && ok) {   // the lane of the context's stream: a scratch of its own, no stream (lane_stream)
        Lane& l = c->lanes[want];
        ok = l.pool_scratch || dmalloc(c, &l.pool_scratch, c->pool_scratch_bytes) == hipSuccess;
    }
    for (int s = 0; s < want_sets && ok; s++) {
        PlaneSet& p = c->sets[s];
        ok = (p.ev_r || hipEventCreateWithFlags(&p.ev_r, hipEventDisableTiming) == hipSuccess) &&
             (p.ev_t || hipEventCreateWithFlags(&p.ev_t, hipEventDisableTiming) == hipSuccess);
    }
    if (!ok) (void)hipGetLastError();
    return ok;
}
// Whether this context's overlapped launches may have their accumulation deferred: not with a tile ring (a call must queue its own
// tile), a history exchange or row stripes.  (Overlapped launches are static-camera, render scale 1, ReSTIR off already.)
static bool can_defer(const vrt_ctx* c) { return c->hdr_targets.empty() && !c->hx_on && c->stripe_rows == 0; }
static void forget_passes(vrt_ctx* c) {   // every stream was drained: no pass is left to wait for
    for (PlaneSet& p : c->sets) p.ev_t_valid = false;
    for (Lane& l : c->lanes) l.last_set = -1;
    c->last_pass_ev = nullptr;
    c->ctx_unsettled = false;
}
// The pipeline for a launch of `items` work items; false (and never tried again) if its streams and copies cannot be had.  The
// depth follows the launch: a context whose caller changes habit (one sample per call, then four) is drained once and goes on in
// the other mode -- the set numbering and the gate distance of the two modes do not mix.
static bool ensure_overlap(vrt_ctx* c, size_t items, bool heavy) {
    if (c->overlap_failed) return false;
    PipelineShape sh = plan_pipeline_shape(items, heavy, c->knobs.hw_queues, can_defer(c), c->knobs);
    const bool first = !c->overlap_ready;
    if (!first && sh.n_streams == c->n_streams && sh.grid_div == c->grid_div && sh.pass_on_render == c->pass_on_render && sh.ctx_lane == c->ctx_lane &&
        sh.pass_on_last == c->pass_on_last) return true;
    bool ok = grow_pipeline(c, sh.n_streams, sh.n_streams + (sh.ctx_lane ? 1 : 0) + sh.defer_k, sh.ctx_lane);
    if (first) {
        if (!ok && sh.defer_k > 1) {   // no memory for the deferred launches' copies: a pass per launch, on the context's stream (which is no lane then)
            sh.defer_k = 1; sh.ctx_lane = false; sh.pass_on_last = sh.pass_on_render;
            c->knobs.ctx_lane = 0;   // (nor is the lane asked for again: the shape of later launches compares equal to this one)
            ok = grow_pipeline(c, sh.n_streams, sh.n_streams + 1, false);
        }
    } else {
        if (!ok) return true;   // no memory for the other mode: this one goes on
        if (sync_guarded(c, c->stream) != hipSuccess) return true;   // (with the deferred passes of the mode that ends)
        drain_all(c);
        if (sync_guarded(c, c->stream) != hipSuccess) return true;   // (the temporal passes behind those launches)
        (void)hipGetLastError();
        forget_passes(c);
        c->mode_switches++;
    }
    c->n_streams = sh.n_streams;
    c->grid_div = sh.grid_div;
    c->pass_on_render = sh.pass_on_render;
    c->ctx_lane = sh.ctx_lane;
    c->pass_on_last = sh.pass_on_last;
    if (sh.ctx_lane) c->lanes[sh.n_streams].last_seq = 0u;   // (nothing of this mode is on the context's stream yet)
    c->n_sets = sh.n_streams + (sh.ctx_lane ? 1 : 0) + sh.defer_k;
    c->defer_k = sh.defer_k;
    if (!first) return true;
    ok = ok && hipEventCreateWithFlags(&c->ev_main, hipEventDisableTiming) == hipSuccess;
    int can_wait = 0;
    const bool want_gate = ok && c->knobs.drain_gate;   // off: launches overlap all the same, only queue earlier
    c->drain_signal = nullptr;
    if (want_gate && hipDeviceGetAttribute(&can_wait, hipDeviceAttributeCanUseStreamWaitValue, c->device) == hipSuccess && can_wait &&
        hipExtMallocWithFlags((void**)&c->drain_signal, 8, hipMallocSignalMemory) == hipSuccess) {
        c->device_allocs.push_back(c->drain_signal);
        hipPointerAttribute_t at;
        bool usable = hipPointerGetAttributes(&at, c->drain_signal) == hipSuccess && at.hostPointer == (void*)c->drain_signal;  // the host must be able to release it
        if (usable) { __atomic_store_n(c->drain_signal, 0u, __ATOMIC_RELEASE); usable = gate_self_test(c); }
        if (!usable) { (void)hipGetLastError(); (void)dfree(c, &c->drain_signal); }
    }
    (void)hipGetLastError();
    if (!ok) { c->overlap_failed = true; return false; }
    c->overlap_ready = true;
    return true;
}

// After a failed queue operation inside vrt_accumulate: nothing may be left waiting for a launch that did not happen, and
// the context must be usable again.  The rotation state (buffer roles, frame index, pipeline slot) only advances at the end
// of an iteration whose launches were all queued, so a context without ReSTIR on the overlapped or plain schedule is back at
// the pass before the failed one.  NOT so the accumulated history of a fused ReSTIR call: its per-sample reuse and
// accumulation passes ping-pong the histories in place, so the passes queued before the failure have advanced them while
// the roles were rolled back -- after a failed call on a ReSTIR context the caller must vrt_reset().
static void abort_pipeline(vrt_ctx* c) {
    const std::string keep = g_err;
    plan_seq_abort(c->launch_seq);   // a pre-pass queued for a launch that did not follow: its tag is never handed out again
    release_gate(c);
    c->drain_signalled = false;
    // the launches that WERE queued are accumulated all the same (the failed one has left no slice behind)
    if (flush_deferred(c, false) != VRT_OK) { (void)hipGetLastError(); c->deferred.clear(); }
    drain_all(c);   // (asynchronous fetches queued before the failure have completed too)
    c->cbuf_read_pending[0] = c->cbuf_read_pending[1] = false;
    c->hdr_targets_written = c->hdr_targets_committed;   // a tile handed out for a pass that was never queued is handed out again
    (void)hipGetLastError();
    resolve_events(c);
    // the work heads rotate with the launch number and each launch zeroes the set eight launches ahead: a launch that did not
    // run leaves a used set behind -- nothing is in flight now, so all of them start clean
    (void)hipMemset(c->d_work, 0, VRT_WORK_SETS * VRT_WORK_HEADS * VRT_WORK_HEAD_STRIDE * sizeof(unsigned));
    (void)hipStreamSynchronize(nullptr);   // (the fill runs on the NULL stream: see dalloc)
    (void)hipGetLastError();
    forget_passes(c);
    c->main_dirty = true;
    c->render_blocks = 0;   // residency and scratch are looked at again
    g_err = keep;
}

// ---- deferred accumulation ---------------------------------------------------------------------------------------------------
// rows of the HDR frame a pass also writes to the caller's ring (vrt_set_hdr_targets)
static f3* next_hdr_target(vrt_ctx* c) {
    if (c->hdr_targets.empty()) return nullptr;
    return (f3*)c->hdr_targets[(size_t)(c->hdr_targets_written++ % c->hdr_targets.size())];
}
static int wait_cbuf_readers(vrt_ctx* c, int b, hipStream_t st = nullptr) {   // an asynchronous fetch may still be reading the HDR buffer a pass (on st) is about to write
    if (c->cbuf_read_pending[b]) { HIP_TRY(hipStreamWaitEvent(st ? st : c->stream, c->ev_cbuf_read[b], 0)); c->cbuf_read_pending[b] = false; }
    return VRT_OK;
}

// One k_temporal_group over deferred[first, first + n): behind those launches, histories and HDR roles swapped ONCE.
static int queue_group(vrt_ctx* c, size_t first, size_t n) {
    TemporalGroup tg;
    memset(&tg, 0, sizeof(tg));
    tg.W = c->cfg.width; tg.H = c->cfg.height; tg.row0 = c->buf0; tg.row1 = c->buf1;
    tg.inv_res = mk2((float)(1.0 / (double)tg.W), (float)(1.0 / (double)tg.H));   // (make_frame_params)
    tg.n_slices = (int)n;
    bool timed = false;
    // the stream the pass runs on: the context's, or the lane of the group's last launch (vrt_ctx::pass_on_last) -- which with
    // ctx_lane is the context's stream one time in n_lanes
    const int lane = c->pass_on_last ? c->deferred[first + n - 1].lane : -1;
    hipStream_t ps = lane >= 0 ? lane_stream(c, lane) : c->stream;
    if (lane >= 0) {
        if (c->main_touched) {   // histories reset, frames fetched, passes of launches that were not deferred: all on the context's stream
            if (ps != c->stream) {
                HIP_TRY(hipEventRecord(c->ev_main, c->stream));
                HIP_TRY(hipStreamWaitEvent(ps, c->ev_main, 0));
            }
            c->main_touched = false;
        }
        // the history ping-pong makes passes sequential
        if (c->last_pass_ev && c->last_pass_lane != lane) HIP_TRY(hipStreamWaitEvent(ps, c->last_pass_ev, 0));
    }
    for (size_t i = 0; i < n; i++) {
        const vrt_ctx::Deferred& d = c->deferred[first + i];
        if (d.lane != lane) HIP_TRY(hipStreamWaitEvent(ps, c->sets[d.set].ev_r, 0));   // (a launch on the pass's own stream precedes it there)
        tg.slice[i] = d.slice;
        timed = timed || d.timed;
    }
    tg.hist_d_in = c->d_hist_d[c->hist_in]; tg.hist_d_out = c->d_hist_d[c->hist_in ^ 1];
    tg.hist_s_in = c->d_hist_s[c->hist_in]; tg.hist_s_out = c->d_hist_s[c->hist_in ^ 1];
    tg.hdr = c->d_cbuf[c->cidx ^ 1];
    tg.gb_refl_filtered = c->d_gb_refl_f;
    if (wait_cbuf_readers(c, c->cidx ^ 1, ps) != VRT_OK) return VRT_E_DEVICE;
    Timer t;   // a group with a timed launch in it carries the timers, and counts for all of its passes
    if (timer_begin(c, &t, timed, 1, ps, (unsigned)n) != VRT_OK) return VRT_E_DEVICE;
    HIP_TRY(launch_temporal_group(ps, tg, c->own0, c->own1));
    if (timer_end(t) != VRT_OK) return VRT_E_DEVICE;
    const int last_set = c->deferred[first + n - 1].set;   // one event for the group: every copy it read is free behind it
    hipEvent_t done = c->sets[last_set].ev_t;
    HIP_TRY(hipEventRecord(done, ps));
    if (lane >= 0) {
        // Whatever comes next on the context's stream -- a fetch, a synchronisation, a pass of a launch that is not deferred,
        // the caller's own work -- comes behind the pass: a wait, no kernel.  Where the stream is a lane that wait is queued when
        // such work is about to come (settle_ctx_stream), not in front of the lane's next launch.
        if (c->ctx_lane) c->ctx_unsettled = c->ctx_unsettled || ps != c->stream;
        else HIP_TRY(hipStreamWaitEvent(c->stream, done, 0));
        c->last_pass_ev = done;
        c->last_pass_lane = lane;
    } else {
        c->main_touched = true;
    }
    for (size_t i = 0; i < n; i++) { PlaneSet& p = c->sets[c->deferred[first + i].set]; p.ev_t_valid = true; p.ev_t_of = last_set; }
    c->passes_n[1] += (uint32_t)n;   // accumulation passes in the reference's sense: one per render launch
    c->hist_in ^= 1;
    c->cidx ^= 1;
    return VRT_OK;
}
// split_tail: while the newest launch is still running the older ones' pass is queued by itself, to run beside that launch --
// otherwise the tail behind the last launch of a run grows from one launch's accumulation to all the pending ones'.
static int flush_deferred(vrt_ctx* c, bool split_tail) {
    const size_t m = c->deferred.size();
    // (split_tail: every caller but the K-th launch of a group is about to look at, or to queue work on, the context's stream)
    if (split_tail) c->main_touched = true;
    if (m == 0) return split_tail ? settle_ctx_stream(c) : VRT_OK;
    int rc = VRT_OK;
    bool split = false;
    if (split_tail && m > 1) {
        split = hipEventQuery(c->sets[c->deferred.back().set].ev_r) == hipErrorNotReady;
        (void)hipGetLastError();
    }
    if (split) {
        rc = queue_group(c, 0, m - 1);
        if (rc == VRT_OK) rc = queue_group(c, m - 1, 1);
    } else {
        rc = queue_group(c, 0, m);
    }
    c->deferred.clear();   // (after a failure too: the caller's abort_pipeline drains what was queued)
    if (split_tail) c->main_touched = true;   // (what the caller queues now comes BEHIND the passes above: the next pass on a lane waits for it)
    if (rc == VRT_OK && split_tail) rc = settle_ctx_stream(c);
    return rc;
}
// What this launch's own pass would have been given, as it stands now (camera, scene, planes).
static void capture_slice(vrt_ctx* c, const FrameParams& fp, const PixelBuffers& out, int g, int set, int lane, bool timed) {
    vrt_ctx::Deferred d;
    d.slice.view_inv = fp.view_inv; d.slice.proj_inv = fp.proj_inv;
    d.slice.color_d = out.color_d; d.slice.color_s = out.color_s;
    d.slice.gb_depth = out.gb_depth; d.slice.gb_refl_raw = out.gb_refl_depth;
    d.slice.max_accum_frames = fp.max_accum_frames;
    d.slice.n_samples = g; d.slice.sample_stride = out.sample_stride;
    d.set = set; d.lane = lane; d.timed = timed;
    c->deferred.push_back(d);
}

// ---- vrt_accumulate, step by step --------------------------------------------------------------------------------------------
static bool restir_on(const vrt_ctx* c) { return c->cfg.use_restir != 0; }

// The persistent render grid and its scratch, after anything that changes the kernel's residency (render_blocks == 0).
static int size_render_grid(vrt_ctx* c) {
    if (flush_deferred(c) != VRT_OK) return VRT_E_DEVICE;   // (the scratch below is freed behind the context's stream)
    // Two schedules of the same per-path code: the fused one (a lane owns a path, vrt_path.h) and the pooled one (a wave owns a pool of paths in LDS and
    // works stage by stage, vrt_pool.h).  A pooled context is sized for BOTH its workgroup geometries: grid and light change without coming here.
    // (Nor do the answers depend on the cull / black-sun sibling it is in now: launch bounds and LDS are the siblings', the register attribute holds
    // all of them to two waves per SIMD -- three on the twelve-wave geometry.)  Two query keys, not a launch's choice:
    const auto on = [c](bool d12) { RenderVariant k = render_variant(c, 1); k.dense12 = d12; return k; };
    const RenderVariant v = on(false), v_d12 = on(true);
    if (c->knobs.render == -2) return fail(VRT_E_INVALID, "VRT_RENDER must be 'fused' or 'pool'");
    int per_cu = 0;
    size_t per_block = 0, per_block12 = 0;   // scratch bytes
    if (v.pooled) HIP_TRY(query_render_pool(c->cfg.grid_res, v, &per_cu, &per_block));
    else HIP_TRY(query_render_residency(c->cfg.grid_res, v.restir, v.instr, &per_cu));
    if (per_cu < 1) per_cu = 1;
    if (per_cu > 8) per_cu = 8;
    int cus = c->n_cu - c->reserved_cus;
    if (cus < 8) cus = c->n_cu < 8 ? c->n_cu : 8;
    c->render_blocks = per_cu * cus;   // (abort_pipeline zeroes it again if an allocation below fails)
    c->render_blocks_d12 = 0;
    if (v.pooled && !v.restir) {   // the contexts whose launches take the twelve-wave geometry once grid and light call for it
        int per_cu12 = 0;
        HIP_TRY(query_render_pool(c->cfg.grid_res, v_d12, &per_cu12, &per_block12));
        c->render_blocks_d12 = (per_cu12 < 1 ? 1 : per_cu12) * cus;
    }
    c->pool_scratch_bytes = std::max(c->render_blocks * per_block, c->render_blocks_d12 * per_block12);
    if (!v.pooled) return VRT_OK;
    HIP_TRY(sync_guarded(c, c->stream));
    for (int s = 0; s < VRT_MAX_STREAMS; s++) {   // lane 0's, then that of every other stream the pipeline has, whatever the depth in use
        Lane& l = c->lanes[s];
        if (s > 0 && !(c->overlap_ready && (l.stream || l.pool_scratch))) continue;   // (the lane of the context's stream has a scratch and no stream)
        HIP_TRY(dfree(c, &l.pool_scratch));
        HIP_TRY(dmalloc(c, &l.pool_scratch, c->pool_scratch_bytes));
    }
    return VRT_OK;
}

// A launch of half the slots only pays with other launches beside it: one that finds the pipeline empty (the caller
// fetches every frame, or this is the first of a run) takes every slot like a launch that is not overlapped.
// The same holds for a pipeline that is nearly empty -- a caller that presents every frame and waits for frame k - 1
// before it queues frame k + 1 keeps one or two launches in flight, which as half-size launches leave half the chip idle:
// fewer than two launches still running means every slot.
static bool pipeline_nearly_empty(vrt_ctx* c) {
    int running = 0;
    for (unsigned back = 1; back <= 3u && back <= c->pipe_seq; back++)
        if (hipEventQuery(c->sets[plan_set_of(c->pipe_seq - back, c->n_sets)].ev_r) == hipErrorNotReady) running++;
    (void)hipGetLastError();   // (hipErrorNotReady is the expected answer)
    return running < c->knobs.full_below;
}

// The camera-ray table of `lane` (allocated on first use; null if there is no memory for it: the launch then shares nothing).
static PrimaryRecord* lane_prim_cache(vrt_ctx* c, int lane) {
    Lane& l = c->lanes[lane];
    if (!l.prim_cache && dalloc(c, &l.prim_cache, c->npix) != hipSuccess) { (void)hipGetLastError(); (void)dfree(c, &l.prim_cache); }
    return l.prim_cache;
}

// The queue of `lane` for a launch of `tiles` tiles and g samples (plan_primary_caps), allocated on first use and grown behind the
// lane's stream when a launch needs more than the last did.  False: no memory for it -- the launch is queued without.
static bool lane_primary_queue(vrt_ctx* c, int lane, const RenderVariant& v, unsigned tiles, int g, PrimaryQueue* q) {
    Lane& l = c->lanes[lane];
    const PrimaryCaps caps = plan_primary_caps(tiles, g, c->knobs.primary_cap);
    const size_t words = v.black_sun ? PrimaryContWords<true>::count : PrimaryContWords<false>::count;
    const size_t need_e = (size_t)VRT_PV_HEADS * caps.cap * words, need_l = (size_t)VRT_PV_HEADS * caps.left_cap;
    if (need_e == 0 || need_l == 0) return false;
    if (need_e > l.pv_entry_words || need_l > l.pv_left_words || !l.pv_counts) {
        if (l.pv_entries || l.pv_leftovers) { if (hipStreamSynchronize(lane_stream(c, lane)) != hipSuccess) { (void)hipGetLastError(); return false; } }
#if defined(VRT_DEV_KNOBS)
        if (l.pv_entries || l.pv_leftovers) l.pv_regrown++;   // (the first allocation is not counted: tests/test_gpu_primary_routes.py)
#endif
        (void)dfree(c, &l.pv_entries); (void)dfree(c, &l.pv_leftovers);
        l.pv_entry_words = l.pv_left_words = 0;
        bool ok = l.pv_counts || dalloc(c, &l.pv_counts, (size_t)VRT_PV_HEADS * VRT_PV_COUNT_STRIDE) == hipSuccess;
        ok = ok && dmalloc(c, &l.pv_entries, need_e * sizeof(uint32_t)) == hipSuccess && dmalloc(c, &l.pv_leftovers, need_l * sizeof(uint32_t)) == hipSuccess;
        if (!ok) { (void)hipGetLastError(); (void)dfree(c, &l.pv_entries); (void)dfree(c, &l.pv_leftovers); return false; }
        l.pv_entry_words = need_e; l.pv_left_words = need_l;
    }
#if defined(VRT_DEV_KNOBS)
    if (!c->d_pv_report && getenv("VRT_PRIMARY_REPORT") && dalloc(c, &c->d_pv_report, 2) != hipSuccess) { (void)hipGetLastError(); (void)dfree(c, &c->d_pv_report); }
#endif
    q->counts = l.pv_counts; q->entries = l.pv_entries; q->leftovers = l.pv_leftovers;
    q->cap = caps.cap; q->left_cap = caps.left_cap;
    q->report = c->d_pv_report;
    return true;
}

// An overlapped launch into copy `set` on render stream `lane` comes behind what it depends on.  pre: the launch's pre-pass
// (plan_prepass) goes in here; *served: it was queued and the launch is to be told.  out, g: what the launch writes and its samples;
// *queue: with plan_primary, the launch's primary vertices are queued here too (k_primary_vertex) and the launch is to take its
// paths from queue->.
static int order_overlapped_launch(vrt_ctx* c, int set, int lane, const Prepass& pre, const RenderVariant& v, const FrameParams& fp, const SceneData& sc, bool* served,
                                   const PixelBuffers& out, int g, PrimaryQueue* queue, bool* queued) {
    hipStream_t rs = lane_stream(c, lane);
    *served = false;
    *queued = false;
    PrimaryRecord* prim_queued = nullptr;
    if (c->main_dirty) {  // uploads / prepare / sky kernels queued on the main stream come first (where it is a lane itself: in stream order)
        HIP_TRY(hipEventRecord(c->ev_main, c->stream));
        for (int s = 0; s < c->n_streams; s++) HIP_TRY(hipStreamWaitEvent(c->lanes[s].stream, c->ev_main, 0));
        c->main_dirty = false;
    }
    // What goes on the lane ahead of the launch, in plan_lane_ops' order (vrt_plan.h).  The pre-pass reads the scene and writes the
    // lane's record table, which the lane's previous launch has done with in stream order: behind the scene and in front of every wait
    // that holds the launch itself back -- for the copy it writes, for the slots it takes -- so that it runs beside the launches of the
    // other lanes.  It carries the number the launch takes below; from here on that number belongs to this launch whether or not it
    // gets queued (plan_seq_abort).  The primary vertices write the copy's colour planes and g-buffer: behind the pass that last read
    // it, and in front of the gate -- the kernel takes no heavy slot; the queue's counts are zeroed in stream order, behind the lane's
    // previous launch, which read them.
    const PlaneSet& p = c->sets[set];
    const unsigned target = plan_gate_target(c->launch_seq.next, c->prev_launch_full, c->grid_div, c->knobs.gate_extra, c->last_full_seq);
    const bool gate = plan_gate_wait(target, c->lanes[lane].last_seq, c->drain_signal != nullptr, c->drain_signalled);
    LaneOp ops[LANE_OP_COUNT];
    const int n_ops = plan_lane_ops(pre, plan_primary(pre, c->knobs.primary), p.ev_t_valid, gate, ops);
    for (int k = 0; k < n_ops; k++) {
        switch (ops[k]) {
        case LANE_OP_PREPASS:
            if (PrimaryRecord* prim = lane_prim_cache(c, lane)) {
                HIP_TRY(launch_primary_records(rs, c->cfg.grid_res, v, fp, sc, prim, plan_seq_reserve(c->launch_seq)));
#if defined(VRT_DEV_KNOBS)
                // test hook (tests/test_gpu_primary_routes.py): with VRT_TEST_SPOIL_RECORDS=N (read at vrt_create) every N-th record of the
                // pre-pass fails its check, the pattern moving with the launch's number: behind the pre-pass, ahead of every reader
                if (c->knobs.spoil_records > 0) HIP_TRY(launch_spoil_primary_records(rs, fp, prim, (unsigned)c->knobs.spoil_records, c->launch_seq.next));
#endif
                *served = pre.tell;
                prim_queued = prim;
                c->prepass_queued++;
                if (pre.tell) c->prepass_told++;
            }
            break;
        case LANE_OP_WAIT_PASS:   // the pass that last read this copy
            HIP_TRY(hipStreamWaitEvent(rs, c->sets[p.ev_t_of].ev_t, 0));
            break;
        case LANE_OP_ZERO_QUEUE: {   // (without a record table or memory for the queue the launch is queued as one without this stage)
            const unsigned tiles = (unsigned)(((fp.W + 7) >> 3) * launch_tile_rows(fp));
            if (prim_queued && tiles > 0u && lane_primary_queue(c, lane, v, tiles, g, queue)) {
                HIP_TRY(hipMemsetAsync(queue->counts, 0, (size_t)VRT_PV_HEADS * VRT_PV_COUNT_STRIDE * sizeof(uint32_t), rs));
                *queued = true;
            }
            break;
        }
        case LANE_OP_PRIMARY_VERTEX:
            if (*queued) {
                *queued = false;   // (until the kernel is queued: a failure here leaves a launch that is not told)
                HIP_TRY(launch_primary_vertex(rs, c->cfg.grid_res, v, fp, sc, out, prim_queued, c->launch_seq.next, g, *queue));
                *queued = true;
                c->primary_queued++;
            }
            break;
        case LANE_OP_WAIT_GATE:   // the dispatch gate (vrt_ctx::drain_signal): when the launch whose workgroup slots this one will take starts to drain
            HIP_TRY(hipStreamWaitValue32(rs, c->drain_signal, target, hipStreamWaitValueGte, 0xFFFFFFFFu));
            break;
        default: break;
        }
    }
    return VRT_OK;
}

// Back to the single copy: whoever reads pixels a launch does not write (moving camera at half render scale) expects the last
// sample of the last launch in set 0.
static int restore_single_set(vrt_ctx* c) {
    const size_t last = (size_t)(VRT_MAX_FUSED - 1) * c->npix;
    const PlaneSet& from = c->sets[c->last_set];
    const PlaneSet& to = c->sets[0];
    HIP_TRY(hipMemcpyAsync(to.spec_planes + last, from.spec_planes + last, c->npix * sizeof(f3), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(to.refl_planes + last, from.refl_planes + last, c->npix * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(to.gb_pos, from.gb_pos, c->npix * sizeof(f3), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(to.gb_mat, from.gb_mat, c->npix * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    c->last_set = 0;
    return VRT_OK;
}

// What a launch of g samples into copy `set` writes.  planes: colour planes of its own, not the HDR buffer (which holds the
// previous HDR outside the render area).  g samples END on the last specular / reflection / reservoir plane (PlaneSet).
static PixelBuffers pixel_buffers_of(const vrt_ctx* c, int set, int g, bool planes) {
    const PlaneSet& p = c->sets[set];
    const size_t first_plane = (size_t)(VRT_MAX_FUSED - g) * c->npix;
    PixelBuffers out;
    out.color_d = planes ? p.multi_d : c->d_cbuf[c->cidx];
    out.color_s = p.spec_planes + first_plane;
    out.gb_refl_depth = p.refl_planes + first_plane;
    out.sample_stride = g > 1 ? (int)c->npix : 0;
    out.gb_normal = c->d_gb_normal[c->cur]; out.gb_depth = c->d_gb_depth[c->cur];
    out.gb_position = p.gb_pos; out.gb_mat = p.gb_mat;
    out.reservoir = restir_on(c) ? c->d_res[0] - (size_t)(g - 1) * c->npix : nullptr;
    return out;
}

// Sample s of a launch through spatial reuse (ReSTIR) and its accumulation pass, on the context's stream; hist / ci: the history
// and HDR roles as the passes before it in this iteration have left them.
static int queue_sample_pass(vrt_ctx* c, const FrameParams& fp, const SceneData& sc, const PixelBuffers& out, int s, int g, bool timed, int hist, int ci, bool completes_call) {
    const bool restir = restir_on(c);
    const size_t off = (size_t)s * (size_t)out.sample_stride;   // this sample's plane (ReSTIR; stride 0 with one sample)
    FrameParams fps = fp;
    fps.frame = fp.frame + (uint32_t)s;
    const f3* cd = out.color_d;
    const f3* cs = out.color_s;
    Timer t;
    if (restir) {
        GrisBuffers gb;
        gb.color_d_in = out.color_d + off; gb.color_s_in = out.color_s + off; gb.color_d_out = c->d_color_d2; gb.color_s_out = c->d_color_s2;
        gb.gb_normal = out.gb_normal; gb.gb_depth = out.gb_depth; gb.gb_mat = out.gb_mat;
        gb.res_in = out.reservoir + off; gb.res_out = c->d_res[1];
        gb.geo = c->d_gris_geo; gb.src = c->d_gris_src; gb.tst = c->d_gris_tst; gb.mats_x = c->d_mats_x;
        int g0 = c->own0 - 2 < c->buf0 ? c->buf0 : c->own0 - 2, g1 = c->own1 + 2 > c->buf1 ? c->buf1 : c->own1 + 2;
        if (timer_begin(c, &t, timed, 2, c->stream) != VRT_OK) return VRT_E_DEVICE;
        HIP_TRY(launch_gris(c->stream, c->cfg.grid_res, render_variant(c, g).instr, fps, sc, gb, g0, g1));
        c->passes_n[2]++;
        if (timer_end(t) != VRT_OK) return VRT_E_DEVICE;
        cd = c->d_color_d2;
        cs = c->d_color_s2;
    }
    TemporalBuffers tb;
    tb.color_d = cd; tb.color_s = cs;
    tb.gb_normal = out.gb_normal; tb.gb_depth = out.gb_depth; tb.gb_mat = out.gb_mat;
    tb.gb_refl_raw = out.gb_refl_depth + (restir ? off : 0); tb.gb_refl_filtered = c->d_gb_refl_f;
    tb.hist_d_in = c->d_hist_d[hist]; tb.hist_d_out = c->d_hist_d[hist ^ 1];
    tb.hist_s_in = c->d_hist_s[hist]; tb.hist_s_out = c->d_hist_s[hist ^ 1];
    // (the "previous" g-buffer of a launch's later samples is the launch's own: a launch per sample would have written it again)
    tb.prev_normal = s == 0 ? c->last_gb_normal : c->d_gb_normal[c->cur];
    tb.prev_depth = s == 0 ? c->last_gb_depth : c->d_gb_depth[c->cur];
    // a row tile's moving camera: the previous state of the whole frame (history exchange; one sample per call)
    const bool frame_prev = c->d_hx_hist_d && fps.camera_is_moving;
    if (frame_prev) {
        tb.hist_d_in = c->d_hx_hist_d; tb.hist_s_in = c->d_hx_hist_s;
        tb.prev_normal = c->d_hx_normal; tb.prev_depth = c->d_hx_depth;
    }
    tb.hdr = c->d_cbuf[ci ^ 1];
    tb.sample_stride = restir ? 0 : out.sample_stride;
    tb.prev_view = c->prev_view; tb.prev_proj = c->prev_proj;
    tb.tile = completes_call ? next_hdr_target(c) : nullptr;
    tb.tile_row0 = c->own0;
    if (wait_cbuf_readers(c, ci ^ 1) != VRT_OK) return VRT_E_DEVICE;
    if (timer_begin(c, &t, timed, 1, c->stream) != VRT_OK) return VRT_E_DEVICE;
    if (c->stripe_rows) {   // one launch over the context's own rows, stripe after stripe (the kernel maps them: k_temporal)
        const int n_own = (int)owned_ranges(c).size() * c->stripe_rows;   // (a last stripe cut short by the frame's edge is cut there)
        HIP_TRY(launch_temporal(c->stream, fps, tb, 0, n_own, g));
    } else {
        HIP_TRY(launch_temporal(c->stream, fps, tb, c->own0, c->own1, restir ? 1 : g, frame_prev));
    }
    if (timer_end(t) != VRT_OK) return VRT_E_DEVICE;
    c->passes_n[1]++;
    return VRT_OK;
}

// The roles move on once every launch of an iteration is queued (abort_pipeline relies on it).
static void commit_rotation(vrt_ctx* c, int set, bool overlapped, int hist, int ci, int g, size_t items) {
    if (overlapped) c->pipe_seq += 1;
    c->last_set = set;
    c->hist_in = hist;
    c->prev_gb = c->cur;
    c->last_gb_normal = c->d_gb_normal[c->cur]; c->last_gb_depth = c->d_gb_depth[c->cur];
    c->cur = (c->cur + 1) % VRT_GB_ROT;
    c->cidx = ci;
    c->frame += (uint32_t)g;
    c->stats.path_samples += (uint64_t)items;
}

static int accumulate_impl(vrt_ctx* c, int n_samples) {
    const bool restir = restir_on(c), pooled = render_variant(c, 1).pooled;   // (neither changes in a context's life)
    if (c->render_blocks == 0) {
        const int rc = size_render_grid(c);
        if (rc != VRT_OK) return rc;
    }
    // The samples of one call share camera, jitter and scene; with a still camera at full render scale and ReSTIR
    // off they only differ in their random streams, so up to VRT_MAX_FUSED of them go through ONE k_render launch
    // (work items = pixels x samples: 4x the parallelism per launch, one tail instead of four) into consecutive
    // colour planes, and ONE k_temporal launch advances the running means sample by sample in registers.
    // With ReSTIR on the samples fuse in the RENDER launch all the same (one reservoir plane per sample beside the colour
    // planes; the pooled kernel only): spatial reuse and accumulation then run sample by sample over the planes, as the
    // reference runs them -- the reuse pass of a sample reads nothing an earlier sample's pass wrote.  VRT_FUSE_RESTIR=0: off.
    const bool fuse_restir = pooled && c->knobs.fuse_restir;
    const bool can_fuse = (!restir || fuse_restir) && c->cam.camera_is_moving == 0 && c->cam.render_scale == 1.0f;
    // A persistent render launch ends in a tail: the last paths of every wave bounce on at low occupancy (about 0.16 ms
    // of a 1.5 ms launch at 1080p).  Fused launches of the pooled kernel are therefore OVERLAPPED: launch k+1 goes to
    // the next of n_streams render streams and writes the next copy of the colour planes / g-buffer while launch k drains
    // and its temporal pass (main stream, waits for launch k only) runs.  With n_streams + 1 copies launch k+n_streams+1
    // reuses launch k's and waits for temporal pass k, so render launches follow each other without a gap and the temporal
    // passes run beside them (ensure_overlap: how deep).  Results are unchanged; VRT_OVERLAP=0 turns it off.
    const bool may_overlap = pooled && can_fuse && !restir && c->knobs.overlap;
    for (int done = 0; done < n_samples;) {
        int g = plan_fused_count(n_samples - done, can_fuse, c->knobs.max_fused);
        // One-sample launches are pipelined like fused ones (the reference's own loop is one sample per call: scene.py:177,
        // 255-256): they render into plane 0 of the rotating copies instead of the HDR buffer.  VRT_OVERLAP_SINGLE=0: only fused ones.
        bool want_overlap = may_overlap && (g > 1 || c->knobs.overlap_single);
        if ((g > 1 || want_overlap) && !c->sets[0].multi_d && dalloc(c, &c->sets[0].multi_d, c->npix * VRT_MAX_FUSED) != hipSuccess) {
            (void)hipGetLastError(); (void)dfree(c, &c->sets[0].multi_d); g = 1; want_overlap = false;   // no memory: one launch per sample
        }
        const size_t items = (size_t)c->cfg.width * owned_rows(c) * (size_t)g;   // work items of the launch
        const FrameParams fp = make_frame_params(c);
        const RenderVariant v = render_variant(c, g);   // which kernel this launch takes
        const bool overlapped = want_overlap && ensure_overlap(c, items, v.dense12);
        const bool planes = g > 1 || overlapped;   // the launch writes colour planes of its own, not the HDR buffer
        // Its accumulation is deferred to a pass over defer_k launches (flush_deferred); a launch that is not deferred comes
        // behind the passes of those that were.
        const bool defer = overlapped && c->defer_k > 1 && can_defer(c);
        if (!defer && flush_deferred(c) != VRT_OK) return VRT_E_DEVICE;
        const int set = overlapped ? plan_set_of(c->pipe_seq, c->n_sets) : 0;
        const int lane = overlapped ? plan_lane_of(c->pipe_seq, n_lanes(c)) : 0;
        hipStream_t rs = overlapped ? lane_stream(c, lane) : c->stream;
        bool lone = !overlapped;   // every workgroup slot
        if (overlapped && c->grid_div > 1) lone = pipeline_nearly_empty(c);
        const SceneData sc = make_scene_data(c);
        bool prim_served = false, prim_queued = false;
        PrimaryQueue pq{};
        if (overlapped) {
            const Prepass pre = plan_prepass(v, overlapped, lone, c->grid_div, c->knobs.prepass);
            if (order_overlapped_launch(c, set, lane, pre, v, fp, sc, &prim_served, pixel_buffers_of(c, set, g, planes), g, &pq, &prim_queued) != VRT_OK) return VRT_E_DEVICE;
        } else if (c->last_set != 0) {
            if (restore_single_set(c) != VRT_OK) return VRT_E_DEVICE;
        }
        if (c->pending.size() > 192) resolve_completed(c);
        // (an asynchronous fetch may still be reading the HDR buffer this launch renders into; the passes below check theirs)
        if (!planes && wait_cbuf_readers(c, c->cidx) != VRT_OK) return VRT_E_DEVICE;
        const PixelBuffers out = pixel_buffers_of(c, set, g, planes);
        if (c->cam.render_scale != 1.0f) {
            // a pass that renders part of the frame: the reference's g-buffer is ONE array, so the pixels it leaves out
            // keep what the last pass wrote -- the rotating copy starts as a copy of the last one
            HIP_TRY(hipMemcpyAsync(c->d_gb_normal[c->cur], c->last_gb_normal, c->npix * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(c->d_gb_depth[c->cur], c->last_gb_depth, c->npix * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        }
        const unsigned seq = plan_seq_take(c->launch_seq);
        const bool timed = c->since_reset++ % plan_timer_period(c->knobs.time_every, restir, items, c->knobs.deep_items) == 0u;   // this launch and its passes carry timers
        c->passes_n[0]++;
        Timer t;
        if (timer_begin(c, &t, timed, 0, rs) != VRT_OK) return VRT_E_DEVICE;
        // test hook (tests/test_gpu_pipeline.py): launch number VRT_TEST_FAIL_LAUNCH (read at vrt_create) is reported as failed instead of queued
        if (c->knobs.fail_launch >= 0 && (unsigned)c->knobs.fail_launch == seq) return fail(VRT_E_DEVICE, "injected launch failure (VRT_TEST_FAIL_LAUNCH)");
        // fused samples share their camera rays through this table (vrt_pool.h)
        PrimaryRecord* const prim = v.share_primary ? lane_prim_cache(c, lane) : nullptr;
        const int all_blocks = v.dense12 ? c->render_blocks_d12 : c->render_blocks;
        const int blocks = lone ? all_blocks : plan_partial_blocks(all_blocks, c->grid_div);
        if (pooled && prim_queued) HIP_TRY(launch_render_pool_queued(rs, c->cfg.grid_res, v, blocks, fp, sc, out, c->d_work, seq, g, c->lanes[lane].pool_scratch, c->drain_signal, prim, pq));
        else if (pooled) HIP_TRY(launch_render_pool(rs, c->cfg.grid_res, v, blocks, fp, sc, out, c->d_work, seq, g, c->lanes[lane].pool_scratch, c->drain_signal, prim, prim_served));
        else HIP_TRY(launch_render(rs, c->cfg.grid_res, restir, v.instr, c->render_blocks, fp, sc, out, c->d_work, seq, g, c->knobs.chunk));
        c->drain_signalled = pooled && c->drain_signal != nullptr;
        c->prev_launch_full = blocks == all_blocks;
        if (c->prev_launch_full && pooled) c->last_full_seq = seq + 1u;
        if (timer_end(t) != VRT_OK) return VRT_E_DEVICE;
        PlaneSet& p = c->sets[set];
        if (overlapped) {
            HIP_TRY(hipEventRecord(p.ev_r, rs));
            if (!defer) HIP_TRY(hipStreamWaitEvent(c->stream, p.ev_r, 0));
            c->last_render_set = set;
            c->lanes[lane].last_seq = seq + 1u;
            c->lanes[lane].last_set = set;
            if (c->ctx_lane && rs != c->stream) c->ctx_unsettled = true;
        }
        if (defer) capture_slice(c, fp, out, g, set, lane, timed);
        // ReSTIR: spatial reuse and accumulation sample by sample over the planes of the launch (one pass with one sample)
        const int passes = defer ? 0 : restir ? g : 1;
        if (passes) c->main_touched = true;   // (the passes below run on the context's stream)
        int hist = c->hist_in, ci = c->cidx;   // (the context's own copies only move once every launch of the iteration is queued)
        for (int s = 0; s < passes; s++) {
            const bool completes_call = done + g >= n_samples && s == passes - 1;
            if (queue_sample_pass(c, fp, sc, out, s, g, timed, hist, ci, completes_call) != VRT_OK) return VRT_E_DEVICE;
            hist ^= 1; ci ^= 1;   // pathtracer.py:1298-1303 copy loop == pointer swaps, once per accumulation pass
        }
        if (overlapped && !defer) {
            HIP_TRY(hipEventRecord(p.ev_t, c->stream));
            p.ev_t_valid = true; p.ev_t_of = set;
        } else if (!overlapped && c->overlap_ready) {  // this pass used copy 0 and the single-copy buffers: later overlapped launches wait for it
            for (int s = 0; s < c->n_sets; s++) { HIP_TRY(hipEventRecord(c->sets[s].ev_t, c->stream)); c->sets[s].ev_t_valid = true; c->sets[s].ev_t_of = s; }
        }
        commit_rotation(c, set, overlapped, hist, ci, g, items);
        done += g;
        // (the K-th launch's pass is queued with it, like a pass of its own would be: no split)
        if ((int)c->deferred.size() >= c->defer_k && flush_deferred(c, false) != VRT_OK) return VRT_E_DEVICE;
    }
    return VRT_OK;
}

// after a vrt_accumulate call: the tile's own rows of the new state into the whole-frame planes (behind the call's last pass)
static int store_history_rows(vrt_ctx* c) {
    const size_t W = c->cfg.width, rows = (size_t)(c->own1 - c->own0), off = (size_t)(c->own0 - c->buf0) * W, at = (size_t)c->own0 * W;
    HIP_TRY(hipMemcpyAsync(c->d_hx_hist_d + at, c->d_hist_d[c->hist_in] + off, rows * W * sizeof(f4), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_hx_hist_s + at, c->d_hist_s[c->hist_in] + off, rows * W * sizeof(f4), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_hx_depth + at, c->last_gb_depth + off, rows * W * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_hx_normal + at, c->last_gb_normal + off, rows * W * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    return VRT_OK;
}

extern "C" int vrt_accumulate(vrt_ctx* c, int n_samples) {
    if (!c || n_samples < 0) return fail(VRT_E_INVALID, "bad argument");
    if (!c->prepared) return fail(VRT_E_STATE, "vrt_prepare has not run since the last voxel upload");
    if (!c->have_cam) return fail(VRT_E_STATE, "vrt_set_camera has not been called");
    const bool hx = c->d_hx_hist_d != nullptr && n_samples > 0;
    if (hx && c->cam.camera_is_moving) {
        if (n_samples != 1)
            return fail(VRT_E_INVALID, "moving camera on a row tile: one sample per call (each sample resamples the other tiles' state from the sample before)");
        for (int r = 0; r < c->cfg.height && c->hx_epoch > 0; r++)
            if ((r < c->own0 || r >= c->own1) && c->hx_row_epoch[(size_t)r] != c->hx_epoch)
                return fail(VRT_E_STATE, "history row " + std::to_string(r) + " has not been imported since the last vrt_accumulate (vrt_history_rows_io)");
    }
    HIP_TRY(hipSetDevice(c->device));
#if defined(VRT_HOST_PROFILE)
    const double t_acc = prof_now();
    const int rc = accumulate_impl(c, n_samples);
    { auto& p_ = g_prof["(the whole of accumulate_impl)"]; p_.first += prof_now() - t_acc; p_.second++; }
#else
    const int rc = accumulate_impl(c, n_samples);
#endif
    if (rc != VRT_OK) abort_pipeline(c);
    else c->hdr_targets_committed = c->hdr_targets_written;
    if (rc == VRT_OK && n_samples > 0) {   // what vrt_denoise must know of this call: vrt_set_camera may run before it does
        c->acc_valid = true;
        c->acc_moving = c->cam.camera_is_moving;
        c->acc_scale = c->cam.render_scale;
    }
    if (rc == VRT_OK && hx) {
        if (store_history_rows(c) != VRT_OK) { abort_pipeline(c); return VRT_E_DEVICE; }
        c->hx_epoch++;
    }
    return rc;
}
