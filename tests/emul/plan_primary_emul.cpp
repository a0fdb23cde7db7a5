// plan_primary_emul.cpp -- TEST TOOLING: which launches have their primary vertices shaded ahead of them (voxel_rt2_amd/csrc/vrt_plan.h,
// plan_primary), how their queue is sized (plan_primary_caps) and in which order the lane's queue operations go (plan_lane_ops), behind a
// C interface.  tests/test_pipeline_primary_host.py compiles this with g++ and calls it through ctypes.
#include "../../voxel_rt2_amd/csrc/vrt_plan.h"

extern "C" {

// in: as tests/emul/plan_prepass_emul.cpp's prepass_decision takes them -- plan_render_variant's thirteen inputs, then {overlapped, lone,
// grid_div, prepass knob} -- then {primary knob}.  Returns pre-pass queued | told << 1 | primary << 2.
int primary_decision(const int* in) {
    RenderInputs r;
    r.width = in[0]; r.height = in[1]; r.max_depth = in[2]; r.knob_render = in[3]; r.knob_cull = in[4];
    r.use_restir = in[5] != 0; r.instrumented = in[6] != 0; r.count_as_timed = in[7] != 0; r.ref_oob = in[8] != 0;
    r.cull_active = in[9] != 0; r.dense_grid = in[10] != 0; r.light_emits = in[11] != 0; r.fused = in[12];
    const Prepass p = plan_prepass(plan_render_variant(r), in[13] != 0, in[14] != 0, in[15], in[16]);
    return (p.queue ? 1 : 0) | (p.tell ? 2 : 0) | (plan_primary(p, in[17]) ? 4 : 0);
}
int primary_default_knob() { return Knobs().primary; }
void primary_caps(unsigned tiles, int n_samples, long long knob_cap, unsigned* cap, unsigned* left_cap) {
    const PrimaryCaps c = plan_primary_caps(tiles, n_samples, knob_cap);
    *cap = c.cap; *left_cap = c.left_cap;
}
// The lane's operations ahead of a launch: ops[LANE_OP_COUNT], returns how many.
int primary_lane_ops(int pre_queue, int pre_tell, int primary, int wait_pass, int wait_gate, int* ops) {
    Prepass p;
    p.queue = pre_queue != 0; p.tell = pre_tell != 0;
    LaneOp o[LANE_OP_COUNT];
    const int n = plan_lane_ops(p, primary != 0, wait_pass != 0, wait_gate != 0, o);
    for (int i = 0; i < n; i++) ops[i] = (int)o[i];
    return n;
}

}  // extern "C"
