// plan_emul.cpp -- TEST TOOLING: the launch pipeline's decisions (voxel_rt2_amd/csrc/vrt_plan.h, which knows neither HIP nor the
// context) behind a C interface.  tests/test_pipeline_plan_host.py compiles this with g++ and calls it through ctypes.
#include "../../voxel_rt2_amd/csrc/vrt_plan.h"

extern "C" {

int plan_max_sets(void) { return VRT_MAX_SETS; }

// knobs: {streams, grid_div, pass_stream, defer4, defer8}, -100 = the shipped default.  out: {n_streams, grid_div, pass_on_render, defer_k}.
void plan_shape(long long items, int heavy, int hw_queues, int can_defer, const int* knobs, int* out) {
    Knobs k;
    if (knobs[0] != -100) k.streams = knobs[0];
    if (knobs[1] != -100) k.grid_div = knobs[1];
    if (knobs[2] != -100) k.pass_stream = knobs[2];
    if (knobs[3] != -100) k.defer4 = knobs[3];
    if (knobs[4] != -100) k.defer8 = knobs[4];
    const PipelineShape sh = plan_pipeline_shape((size_t)items, heavy != 0, hw_queues, can_defer != 0, k);
    out[0] = sh.n_streams; out[1] = sh.grid_div; out[2] = sh.pass_on_render ? 1 : 0; out[3] = sh.defer_k;
}
// in: RenderInputs in declaration order, the booleans as 0 / 1.  Returns the variant as bits, in RenderVariant's order:
// pooled 1, restir 2, instr 4, cull 8, black_sun 16, dense12 32, share_primary 64.
int plan_variant(const int* in) {
    RenderInputs r;
    r.width = in[0]; r.height = in[1]; r.max_depth = in[2];
    r.knob_render = in[3]; r.knob_cull = in[4];
    r.use_restir = in[5] != 0;
    r.instrumented = in[6] != 0; r.count_as_timed = in[7] != 0;
    r.ref_oob = in[8] != 0;
    r.cull_active = in[9] != 0; r.dense_grid = in[10] != 0;
    r.light_emits = in[11] != 0;
    r.fused = in[12];
    const RenderVariant v = plan_render_variant(r);
    return (v.pooled ? 1 : 0) | (v.restir ? 2 : 0) | (v.instr ? 4 : 0) | (v.cull ? 8 : 0) | (v.black_sun ? 16 : 0) | (v.dense12 ? 32 : 0) | (v.share_primary ? 64 : 0);
}
int plan_fused(int left, int can_fuse, int max_fused) { return plan_fused_count(left, can_fuse != 0, max_fused); }
unsigned plan_period(int time_every, int restir, long long items) { return plan_timer_period(time_every, restir != 0, (size_t)items, Knobs().deep_items); }
long long plan_deep_items(void) { return Knobs().deep_items; }
unsigned plan_target(unsigned launch_seq, int prev_launch_full, int grid_div, int gate_extra, unsigned last_full_seq) {
    return plan_gate_target(launch_seq, prev_launch_full != 0, grid_div, gate_extra, last_full_seq);
}
int plan_wait(unsigned target, unsigned lane_last_seq, int gate_present, int signalled) {
    return plan_gate_wait(target, lane_last_seq, gate_present != 0, signalled != 0) ? 1 : 0;
}
int plan_blocks(int all_blocks, int grid_div) { return plan_partial_blocks(all_blocks, grid_div); }
int plan_set(unsigned pipe_seq, int n_sets) { return plan_set_of(pipe_seq, n_sets); }
int plan_lane(unsigned pipe_seq, int n_streams) { return plan_lane_of(pipe_seq, n_streams); }
// out: {mat_at, rgb_at, entries_at, heads_at, bytes} of the triangle edits' scratch
void plan_tri(long long head_bytes, long long nv, long long batch, long long* out) {
    const TriLayout l = plan_tri_layout((size_t)head_bytes, (size_t)nv, (size_t)batch);
    out[0] = (long long)l.mat_at; out[1] = (long long)l.rgb_at; out[2] = (long long)l.entries_at; out[3] = (long long)l.heads_at; out[4] = (long long)l.bytes;
}

}  // extern "C"
