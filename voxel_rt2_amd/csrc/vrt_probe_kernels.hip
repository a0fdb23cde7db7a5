// vrt_probe_kernels.hip -- gfx950 kernels of libvrt_hip.so that exist for the tests alone, each with its launcher.
//
//   k_detmath_probe                                       vrt_detmath_probe: one function of include/vrt_detmath.h per element
//   k_trace_probe<G, WALK>                                vrt_trace_probe: one ray per lane through a walk of the pyramid (vrt_probe.h)
//   k_shade_probe                                         vrt_shade_probe: one row of arguments per lane through a shading function (vrt_shade_probe.h)
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "vrt_kernels.h"
#include "vrt_probe.h"
#include "vrt_shade_probe.h"

namespace vrt {

__global__ void k_detmath_probe(int op, int n, const float* a, const float* b, float* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float r = 0.0f;
    switch (op) {
        case 0: r = dm_sin(a[i]); break;
        case 1: r = dm_cos(a[i]); break;
        case 2: r = dm_exp(a[i]); break;
        case 3: r = dm_log(a[i]); break;
        case 4: r = dm_pow(a[i], b[i]); break;
        case 5: r = dm_acos(a[i]); break;
        case 6: r = dm_atan2(a[i], b[i]); break;
        case 7: r = dm_min(a[i], b[i]); break;
        case 8: r = dm_max(a[i], b[i]); break;
        case 9: r = dm_round_f16(a[i]); break;
        case 10: r = a[i] / b[i]; break;
        case 11: r = dm_sqrt(a[i]); break;
        case 12: r = a[i] * b[i] + a[i]; break;  // must NOT contract
        case 13: r = (float)dm_f2i(a[i]); break;
        case 14: r = dm_u2f((uint32_t)dm_f32_to_f16(a[i])); break;             // the half code, as the low bits of the output word
        case 15: r = dm_f16_to_f32((uint16_t)(dm_f2u(a[i]) & 0xffffu)); break;  // input word's low bits = half code
    }
    out[i] = r;
}

// Test hook (vrt_trace_probe): one ray per lane through the closest-hit walk of the pyramid in global memory (vrt_probe.h).
template <int G, int WALK>
__global__ __launch_bounds__(64) void k_trace_probe(Pyramid pyr, const float* cull, int n, const float* rays, ProbeOut* out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    GlobalPyramid<G> P;
    P.p = pyr;
    const float* a = rays + (size_t)i * 6;
    ProbeOut r;
    probe_ray<G, WALK>(P, mk3(a[0], a[1], a[2]), mk3(a[3], a[4], a[5]), cull, r);
    out[i] = r;
}

// Test hook (vrt_shade_probe): one row of arguments per lane through one shading function (vrt_shade_probe.h).
__global__ __launch_bounds__(64) void k_shade_probe(FrameParams fp, SceneData sc, const float* mats_x, int op, int n, const float* in, int in_stride,
                                                    float* out, int out_stride, float* lane_tables) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    shade_probe_row(fp, sc, mats_x, op, in + (size_t)i * in_stride, out + (size_t)i * out_stride, out_stride,
                    lane_tables ? lane_tables + (size_t)i * VRT_SHADE_LANE_TABLE : nullptr);
}

// ---- host-side launchers -----------------------------------------------------------------------
hipError_t launch_detmath_probe(hipStream_t st, int op, int n, const float* a, const float* b, float* out) {
    hipLaunchKernelGGL(k_detmath_probe, dim3((n + 255) / 256), dim3(256), 0, st, op, n, a, b, out);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
hipError_t launch_shade_probe(hipStream_t st, const FrameParams& fp, const SceneData& sc, const float* mats_x, int op, int n, const float* in, int in_stride,
                              float* out, int out_stride, float* lane_tables) {
    if (op == SHADE_SHIFT && !lane_tables) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_shade_probe, dim3((n + 63) / 64), dim3(64), 0, st, fp, sc, mats_x, op, n, in, in_stride, out, out_stride, lane_tables);
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}
hipError_t launch_trace_probe(hipStream_t st, int grid_res, int walk, const Pyramid& pyr, const float* cull, int n, const float* rays, ProbeOut* out) {
    const dim3 g((n + 63) / 64), b(64);
    if (walk == PROBE_WALK_BRANCHY) VRT_BY_GRID(grid_res, hipLaunchKernelGGL((k_trace_probe<G, PROBE_WALK_BRANCHY>), g, b, 0, st, pyr, cull, n, rays, out));
    else if (walk == PROBE_WALK_FLAT) VRT_BY_GRID(grid_res, hipLaunchKernelGGL((k_trace_probe<G, PROBE_WALK_FLAT>), g, b, 0, st, pyr, cull, n, rays, out));
    else if (walk == PROBE_WALK_RECORD) VRT_BY_GRID(grid_res, hipLaunchKernelGGL((k_trace_probe<G, PROBE_WALK_RECORD>), g, b, 0, st, pyr, cull, n, rays, out));
    else return hipErrorInvalidValue;
    VRT_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace vrt
