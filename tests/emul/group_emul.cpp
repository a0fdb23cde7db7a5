// group_emul.cpp -- TEST TOOLING: temporal_group_pixel (voxel_rt2_amd/csrc/vrt_temporal.h, VRT_DEV = inline) on the host, beside
// the K consecutive temporal_pixel passes with swapped histories that it stands for.  tests/test_temporal_group_host.py
// compiles this the way tests/emu.py compiles emul.cpp and compares the two bit for bit.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../voxel_rt2_amd/csrc/vrt_types.h"
#include "../../voxel_rt2_amd/csrc/vrt_trace.h"
#include "../../voxel_rt2_amd/csrc/vrt_bsdf.h"
#include "../../voxel_rt2_amd/csrc/vrt_sky.h"
#include "../../voxel_rt2_amd/csrc/vrt_path.h"
#include "../../voxel_rt2_amd/csrc/vrt_temporal.h"

using namespace vrt;

extern "C" {

// Buffers cover rows [row0, row1) of a W x H frame (npix = (row1 - row0) * W); the passes run over rows [r0, r1).
// Per slice s: g[s] samples, matrices view_inv / proj_inv [s][16], max_accum[s], colour planes color_d / color_s [s][4][npix][3],
// depth [s][npix], refl [s][4][npix].  hist_*0: incoming histories [npix][4].  Outputs: the final histories, HDR and filtered
// reflection depth, [npix] each (rows outside [r0, r1) keep what the caller put there).
int tg_max_group(void) { return VRT_MAX_GROUP; }

int tg_run(int W, int H, int row0, int row1, int r0, int r1, int K, const int* g, const float* view_inv, const float* proj_inv,
           const float* max_accum, const float* color_d, const float* color_s, const float* depth, const float* refl,
           const float* hist_d0, const float* hist_s0, int grouped, float* out_hist_d, float* out_hist_s, float* out_hdr, float* out_refl_f) {
    const size_t npix = (size_t)(row1 - row0) * (size_t)W;
    if (K < 1 || K > VRT_MAX_GROUP) return -1;
    auto stride_of = [&](int s) { return g[s] > 1 ? (int)npix : 0; };
    if (grouped) {
        TemporalGroup tg;
        memset(&tg, 0, sizeof(tg));
        tg.W = W; tg.H = H; tg.row0 = row0; tg.row1 = row1;
        tg.inv_res = mk2((float)(1.0 / (double)W), (float)(1.0 / (double)H));
        tg.n_slices = K;
        tg.hist_d_in = (const f4*)hist_d0; tg.hist_s_in = (const f4*)hist_s0;
        tg.hist_d_out = (f4*)out_hist_d; tg.hist_s_out = (f4*)out_hist_s;
        tg.hdr = (f3*)out_hdr; tg.gb_refl_filtered = out_refl_f;
        for (int s = 0; s < K; s++) {
            TemporalSlice& sl = tg.slice[s];
            memcpy(sl.view_inv.m, view_inv + 16 * s, 64);
            memcpy(sl.proj_inv.m, proj_inv + 16 * s, 64);
            sl.color_d = (const f3*)color_d + (size_t)s * 4 * npix;
            sl.color_s = (const f3*)color_s + (size_t)s * 4 * npix;
            sl.gb_depth = depth + (size_t)s * npix;
            sl.gb_refl_raw = refl + (size_t)s * 4 * npix;
            sl.max_accum_frames = max_accum[s];
            sl.n_samples = g[s];
            sl.sample_stride = stride_of(s);
        }
        for (int v = r0; v < r1; v++)
            for (int u = 0; u < W; u++) temporal_group_pixel(tg, u, v);
        return 0;
    }
    // K passes of their own: histories and HDR buffers swap roles after each (vrt_pipeline.hip, accumulate_impl)
    std::vector<f4> hd[2], hs[2];
    std::vector<f3> hdr[2];
    for (int b = 0; b < 2; b++) { hd[b].resize(npix); hs[b].resize(npix); hdr[b].resize(npix); }
    memcpy(hd[0].data(), hist_d0, npix * sizeof(f4));
    memcpy(hs[0].data(), hist_s0, npix * sizeof(f4));
    int in = 0;
    for (int s = 0; s < K; s++) {
        FrameParams fp;
        memset(&fp, 0, sizeof(fp));
        memcpy(fp.view_inv.m, view_inv + 16 * s, 64);
        memcpy(fp.proj_inv.m, proj_inv + 16 * s, 64);
        fp.inv_res = mk2((float)(1.0 / (double)W), (float)(1.0 / (double)H));
        fp.W = W; fp.H = H; fp.row0 = row0; fp.row1 = row1;
        fp.camera_is_moving = 0;
        fp.render_scale = 1.0f;
        fp.max_accum_frames = max_accum[s];
        TemporalBuffers tb;
        memset(&tb, 0, sizeof(tb));
        tb.color_d = (const f3*)color_d + (size_t)s * 4 * npix;
        tb.color_s = (const f3*)color_s + (size_t)s * 4 * npix;
        tb.gb_depth = depth + (size_t)s * npix;
        tb.gb_refl_raw = refl + (size_t)s * 4 * npix;
        tb.gb_refl_filtered = out_refl_f;
        tb.hist_d_in = hd[in].data(); tb.hist_d_out = hd[in ^ 1].data();
        tb.hist_s_in = hs[in].data(); tb.hist_s_out = hs[in ^ 1].data();
        tb.hdr = hdr[in ^ 1].data();
        tb.sample_stride = stride_of(s);
        tb.tile = nullptr;
        for (int v = r0; v < r1; v++)
            for (int u = 0; u < W; u++) temporal_pixel(fp, tb, u, v, g[s]);
        in ^= 1;
    }
    const size_t a = (size_t)(r0 - row0) * W, n = (size_t)(r1 - r0) * W;
    memcpy((f4*)out_hist_d + a, hd[in].data() + a, n * sizeof(f4));
    memcpy((f4*)out_hist_s + a, hs[in].data() + a, n * sizeof(f4));
    memcpy((f3*)out_hdr + a, hdr[in].data() + a, n * sizeof(f3));
    return 0;
}

}  // extern "C"
