// plan_prepass_emul.cpp -- TEST TOOLING: which launches are preceded by the camera-ray pre-pass (voxel_rt2_amd/csrc/vrt_plan.h,
// plan_prepass) and how launch numbers -- the records' tags -- are handed out around it (LaunchSeq), behind a C interface.
// tests/test_pipeline_prepass_host.py compiles this with g++ and calls it through ctypes.
#include "../../voxel_rt2_amd/csrc/vrt_plan.h"

extern "C" {

// in: plan_render_variant's inputs as tests/emul/plan_emul.cpp's plan_variant takes them -- {width, height, max_depth, knob_render,
// knob_cull, use_restir, instrumented, count_as_timed, ref_oob, cull_active, dense_grid, light_emits, fused} -- then {overlapped, lone,
// grid_div, knob}.  Returns queue | tell << 1.
int prepass_decision(const int* in) {
    RenderInputs r;
    r.width = in[0]; r.height = in[1]; r.max_depth = in[2]; r.knob_render = in[3]; r.knob_cull = in[4];
    r.use_restir = in[5] != 0; r.instrumented = in[6] != 0; r.count_as_timed = in[7] != 0; r.ref_oob = in[8] != 0;
    r.cull_active = in[9] != 0; r.dense_grid = in[10] != 0; r.light_emits = in[11] != 0; r.fused = in[12];
    const Prepass p = plan_prepass(plan_render_variant(r), in[13] != 0, in[14] != 0, in[15], in[16]);
    return (p.queue ? 1 : 0) | (p.tell ? 2 : 0);
}
// The shape a launch of `items` items runs in (plan_pipeline_shape, shipped switches): its grid_div.
int prepass_grid_div(long long items, int heavy, int hw_queues, int can_defer) {
    return plan_pipeline_shape((size_t)items, heavy != 0, hw_queues, can_defer != 0, Knobs()).grid_div;
}
// What the shipped library runs with (Knobs' default).
int prepass_default_knob() { return Knobs().prepass; }

// A run of launches as vrt_pipeline.hip numbers them.  events[i]: 0 = a launch without a pre-pass, queued; 1 = a launch with a
// pre-pass, both queued; 2 = a pre-pass queued, then the launch fails to queue and the pipeline is aborted; 3 = a launch without a
// pre-pass fails AFTER it took its number and the pipeline is aborted.  prepass_tag[i] / launch_tag[i]: the tag (number + 1) handed to
// the event's pre-pass / launch, 0 where there was none.
void prepass_run(int n, const int* events, unsigned* prepass_tag, unsigned* launch_tag) {
    LaunchSeq s;
    for (int i = 0; i < n; i++) {
        prepass_tag[i] = launch_tag[i] = 0u;
        const int e = events[i];
        if (e == 1 || e == 2) prepass_tag[i] = plan_seq_reserve(s) + 1u;
        if (e == 0 || e == 1 || e == 3) launch_tag[i] = plan_seq_take(s) + 1u;
        if (e == 2 || e == 3) plan_seq_abort(s);
    }
}

}  // extern "C"
