// plan_ctx_lane_emul.cpp -- TEST TOOLING: the decisions of the pipeline shape whose third lane is the context's stream
// (voxel_rt2_amd/csrc/vrt_plan.h, PipelineShape::ctx_lane) behind a C interface.  tests/test_pipeline_ctx_lane_host.py compiles this
// with g++ and calls it through ctypes.
#include "../../voxel_rt2_amd/csrc/vrt_plan.h"

extern "C" {

// knobs: {streams, grid_div, pass_stream, ctx_lane, defer4}, -100 = the shipped default.
// out: {n_streams, grid_div, pass_on_render, defer_k, ctx_lane, pass_on_last, lanes, n_sets}.
void ctx_lane_shape(long long items, int heavy, int hw_queues, int can_defer, const int* knobs, int* out) {
    Knobs k;
    if (knobs[0] != -100) k.streams = knobs[0];
    if (knobs[1] != -100) k.grid_div = knobs[1];
    if (knobs[2] != -100) k.pass_stream = knobs[2];
    if (knobs[3] != -100) k.ctx_lane = knobs[3];
    if (knobs[4] != -100) k.defer4 = knobs[4];
    const PipelineShape sh = plan_pipeline_shape((size_t)items, heavy != 0, hw_queues, can_defer != 0, k);
    const int lanes = sh.n_streams + (sh.ctx_lane ? 1 : 0);
    out[0] = sh.n_streams; out[1] = sh.grid_div; out[2] = sh.pass_on_render ? 1 : 0; out[3] = sh.defer_k;
    out[4] = sh.ctx_lane ? 1 : 0; out[5] = sh.pass_on_last ? 1 : 0; out[6] = lanes; out[7] = lanes + sh.defer_k;
}

// The first n launches of a run in which every launch takes half the slots (none finds the pipeline empty), as vrt_pipeline.hip
// sequences them: lane and copy by turns, the gate's target, and whether the stream wait for it is queued given the last launch
// on the lane.  out: n rows of {lane, set, target, wait}.
void ctx_lane_run(int n, int lanes, int n_sets, int grid_div, unsigned* out) {
    unsigned last_seq[VRT_MAX_STREAMS] = {};
    for (unsigned k = 0; k < (unsigned)n; k++) {
        const int lane = plan_lane_of(k, lanes), set = plan_set_of(k, n_sets);
        const unsigned target = plan_gate_target(k, false, grid_div, 0, 0u);
        out[4 * k + 0] = (unsigned)lane; out[4 * k + 1] = (unsigned)set; out[4 * k + 2] = target;
        out[4 * k + 3] = plan_gate_wait(target, last_seq[lane], true, true) ? 1u : 0u;
        last_seq[lane] = k + 1u;
    }
}

}  // extern "C"
