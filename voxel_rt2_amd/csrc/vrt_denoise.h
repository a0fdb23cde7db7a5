// vrt_denoise.h -- vrt_denoise: an edge-avoiding a-trous filter (B3-spline 5x5, the stride doubling per iteration) over the accumulated
// frame, guided by the g-buffer.  Albedo-demodulated diffuse and specular are filtered apart; a tap counts where it has the centre's
// material id, a normal within dot >= 0.9 of the centre's and lies within `tol` of the centre's plane, and weighs by the samples behind
// it; the result fades back to the unfiltered accumulation as the centre's own sample count grows.  include/vrt_api.h states the
// arithmetic to the bit; the functions below are that text.  Plain functions over plain values and read-only planes, in the style of
// vrt_probe_sh.h: k_denoise_prepare / k_denoise_atrous (vrt_kernels.hip) call them a pixel a lane, and tests/emul/denoise_emul.cpp runs
// the same functions on a machine without a GPU (tests/test_denoise_host.py).
//
// What a pixel carries between the kernels (all planes [H][W], whole frames: the pass is refused on row tiles):
//   guide   16 bytes: the primary vertex's position and the oct code of its normal.  Whether the pixel is a surface pixel is
//           !near_zero3(position) -- five operations on a value the tap has loaded anyway, so no flag is stored;
//   mat     4 bytes: the g-buffer's material word, id in its low byte (the gate) and the 8-bit albedo above it (the recomposition);
//   d, s    16 bytes each: the signal's value and, in w, its sample count.  Three copies: step 1's (kept for the fade) and two that the
//           iterations alternate between.
#pragma once
#include "vrt_path.h"

namespace vrt {

#define VRT_DENOISE_MAX_ITERATIONS 6
#define VRT_DENOISE_MIN_ALBEDO 0.00392156886f   // 1 / 255: what the demodulation divides by at least

struct DenoiseGuide { float px, py, pz; uint32_t oct; };   // 16 bytes
// the settings of one call: tol = plane_tolerance * cfg.dx, formed once by the caller
struct DenoiseSettings { int iterations; float tol; float sigma_l; float full_at; int moving; };
// what an iteration reads: the guides, the material words and the previous iteration's two signals
struct DenoiseIn { const DenoiseGuide* guide; const uint32_t* mat; const f4* d; const f4* s; int W, H; };

VRT_DEV f3 denoise_pos(const DenoiseGuide& g) { return mk3(g.px, g.py, g.pz); }
VRT_DEV bool denoise_surface(const DenoiseGuide& g) { return !near_zero3(denoise_pos(g)); }
// A' of step 1: the albedo the static camera's diffuse history is divided by, and multiplied by again at the end
VRT_DEV f3 denoise_floor_albedo(uint32_t M) { return max3s(unpack_albedo(M), VRT_DENOISE_MIN_ALBEDO); }
VRT_DEV float denoise_kernel(int k) { return k == 0 ? 0.375f : (k == 1 ? 0.25f : 0.0625f); }

// Step 1 of one pixel: its guide record and the two signals.  A pixel that is no surface pixel keeps its histories as they are: no tap
// reads them (it fails every tap's surface test) and its output is the HDR frame's value.  Returns whether it is a surface pixel.
VRT_DEV bool denoise_prepare(f3 P, uint32_t normal_oct, uint32_t M, f4 Hd, f4 Hs, int moving, DenoiseGuide& g, f4& d, f4& s) {
    g.px = P.x; g.py = P.y; g.pz = P.z; g.oct = normal_oct;
    d = Hd; s = Hs;
    if (near_zero3(P)) return false;
    if (!moving) {   // (the moving camera's diffuse history is demodulated already: vrt_temporal.h, temporal_pixel)
        const f3 a = denoise_floor_albedo(M);
        d.x = Hd.x / a.x; d.y = Hd.y / a.y; d.z = Hd.z / a.z;
    }
    return true;
}

// The centre pixel of an iteration: what every one of its taps is gated and weighted against.
struct DenoiseCentre { f3 P, N; uint32_t oct, id; float lum_d, lum_s; };
struct DenoiseSums { f3 sum_d, sum_s; float wsum_d, wsum_s; };

// One signal's share of one tap that has passed the gates: steps 6 to 8.  k = K[|dx|] * K[|dy|].
VRT_DEV void denoise_add(f4 xq, float k, bool use_lum, float sigma_l, float lum_p, f3& sum, float& wsum) {
    const f3 X = mk3(xq.x, xq.y, xq.z);
    float w = k * xq.w;
    if (use_lum) {
        const float lq = lum(X);
        const float t = dm_abs(lq - lum_p) / (sigma_l * ((lum_p + lq) * 0.5f) + 0.001f);
        w = w / (1.0f + t * t);
    }
    sum = sum + w * X;
    wsum = wsum + w;
}
// One tap: pixel q = (qu, qv) against centre c.  Outside the frame, not a surface pixel, or failing a gate: nothing is added.
VRT_DEV void denoise_tap(const DenoiseIn& in, const DenoiseCentre& c, int qu, int qv, float k, bool use_lum, float sigma_l, float tol, DenoiseSums& a) {
    if (qu < 0 || qv < 0 || qu >= in.W || qv >= in.H) return;
    const int q = qv * in.W + qu;
    const DenoiseGuide g = in.guide[q];
    if (!denoise_surface(g)) return;
    if ((in.mat[q] & 255u) != c.id) return;
    const f3 nq = g.oct == c.oct ? c.N : oct_decode(g.oct);   // (the same code decodes to the same bits)
    if (!(dot3(c.N, nq) >= 0.9f)) return;
    if (!(dm_abs(dot3(c.N, denoise_pos(g) - c.P)) <= tol)) return;
    denoise_add(in.d[q], k, use_lum, sigma_l, c.lum_d, a.sum_d, a.wsum_d);
    denoise_add(in.s[q], k, use_lum, sigma_l, c.lum_s, a.sum_s, a.wsum_s);
}
VRT_DEV f4 denoise_resolve(f3 sum, float wsum, f4 xp) {
    if (!(wsum > 0.0f)) return xp;
    const f3 r = sum / wsum;
    return mk4(r.x, r.y, r.z, xp.w);   // the count stays as it is through all iterations
}
// One iteration (step 2) of pixel (u, v) at stride `stride`: the two signals' next values.  use_lum: i >= 1 and sigma_l > 0.  Taps in
// the order dy = -2 .. 2 outside, dx = -2 .. 2 inside.  Returns whether (u, v) is a surface pixel; one that is not keeps its values.
VRT_DEV bool denoise_iteration(const DenoiseIn& in, int u, int v, int stride, bool use_lum, float sigma_l, float tol, f4& d_out, f4& s_out) {
    const int p = v * in.W + u;
    const DenoiseGuide g = in.guide[p];
    const f4 dp = in.d[p], sp = in.s[p];
    d_out = dp; s_out = sp;
    if (!denoise_surface(g)) return false;
    DenoiseCentre c;
    c.P = denoise_pos(g);
    c.oct = g.oct;
    c.N = oct_decode(g.oct);
    c.id = in.mat[p] & 255u;
    c.lum_d = lum(mk3(dp.x, dp.y, dp.z));
    c.lum_s = lum(mk3(sp.x, sp.y, sp.z));
    DenoiseSums a;
    a.sum_d = mk3(0.0f); a.sum_s = mk3(0.0f); a.wsum_d = 0.0f; a.wsum_s = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++)
            denoise_tap(in, c, u + dx * stride, v + dy * stride, denoise_kernel(dx < 0 ? -dx : dx) * denoise_kernel(dy < 0 ? -dy : dy), use_lum, sigma_l, tol, a);
    }
    d_out = denoise_resolve(a.sum_d, a.wsum_d, dp);
    s_out = denoise_resolve(a.sum_s, a.wsum_s, sp);
    return true;
}

// Step 3 of one signal: the filtered value F faded back to step 1's value U by the pixel's own count.
VRT_DEV f3 denoise_fade(f4 F, f4 U, float full_at) {
    const float a = full_at > 0.0f ? dm_min(U.w / full_at, 1.0f) : 0.0f;
    const f3 f = mk3(F.x, F.y, F.z), u = mk3(U.x, U.y, U.z);
    return f + (u - f) * a;
}
// Step 3 of a surface pixel: both signals faded, the diffuse one multiplied by the albedo it was divided by, the two added.
VRT_DEV f3 denoise_finish(f4 Fd, f4 Fs, f4 Ud, f4 Us, uint32_t M, int moving, float full_at) {
    const f3 rd = denoise_fade(Fd, Ud, full_at), rs = denoise_fade(Fs, Us, full_at);
    const f3 alb = moving ? unpack_albedo(M) : denoise_floor_albedo(M);
    return (rd * alb) + rs;
}

}  // namespace vrt
