// denoise_emul.cpp -- TEST TOOLING: vrt_denoise on the host.  The per-pixel functions of voxel_rt2_amd/csrc/vrt_denoise.h under the loops
// the kernels of vrt_kernels.hip and the launcher run them in: step 1 of every pixel into scratch planes, `iterations` passes at strides
// 1, 2, 4, .. that alternate between two copies of the signals, the last one going on to step 3.  tests/denoise.py compiles this with g++
// and calls it through ctypes (tests/test_denoise_host.py).  With -DDENOISE_EMUL_MAIN it is a stand-alone program over planes of its own,
// for a run under -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>
#include <vector>
#include "vrt_denoise.h"

using namespace vrt;

extern "C" {

// The planes as vrt_fetch_buffer / vrt_fetch_hdr return them, [H][W] each: pos f32x3, normal u32 (two binary16), mat u32, hist_d / hist_s
// f32x4, hdr f32x3.  tol = plane_tolerance * dx is formed here, as vrt_denoise forms it.  out: f32[H][W][3].
int denoise_emul_run(int W, int H, const float* pos, const uint32_t* normal, const uint32_t* mat, const float* hist_d, const float* hist_s, const float* hdr,
                     int iterations, float plane_tolerance, float sigma_l, float full_at, int moving, float dx, float* out) {
    if (W <= 0 || H <= 0 || iterations < 1 || iterations > VRT_DENOISE_MAX_ITERATIONS) return -1;
    const size_t n = (size_t)W * (size_t)H;
    std::vector<DenoiseGuide> guide(n);
    std::vector<uint32_t> m(n);
    std::vector<f4> d[3], s[3];
    for (int k = 0; k < 3; k++) { d[k].resize(n); s[k].resize(n); }
    const DenoiseSettings set{iterations, plane_tolerance * dx, sigma_l, full_at, moving};
    for (size_t i = 0; i < n; i++) {   // k_denoise_prepare
        const f4 Hd = mk4(hist_d[4 * i], hist_d[4 * i + 1], hist_d[4 * i + 2], hist_d[4 * i + 3]);
        const f4 Hs = mk4(hist_s[4 * i], hist_s[4 * i + 1], hist_s[4 * i + 2], hist_s[4 * i + 3]);
        m[i] = mat[i];
        if (!denoise_prepare(mk3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]), normal[i], mat[i], Hd, Hs, moving, guide[i], d[0][i], s[0][i]))
            memcpy(out + 3 * i, hdr + 3 * i, 3 * sizeof(float));
    }
    int from = 0;   // launch_denoise_filter
    for (int it = 0; it < iterations; it++) {
        const int to = from == 1 ? 2 : 1;
        const DenoiseIn in{guide.data(), m.data(), d[from].data(), s[from].data(), W, H};
        const bool use_lum = it >= 1 && set.sigma_l > 0.0f, last = it == iterations - 1;
        for (int v = 0; v < H; v++)
            for (int u = 0; u < W; u++) {   // k_denoise_atrous
                const size_t i = (size_t)v * W + u;
                f4 xd, xs;
                const bool surface = denoise_iteration(in, u, v, 1 << it, use_lum, set.sigma_l, set.tol, xd, xs);
                if (!last) { d[to][i] = xd; s[to][i] = xs; continue; }
                if (!surface) continue;
                const f3 r = denoise_finish(xd, xs, d[0][i], s[0][i], m[i], set.moving, set.full_at);
                out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
            }
        from = to;
    }
    return 0;
}
// oct_decode of one code: float out[3]
void denoise_emul_normal(uint32_t code, float* out) {
    const f3 n = oct_decode(code);
    out[0] = n.x; out[1] = n.y; out[2] = n.z;
}
uint32_t denoise_emul_encode(float x, float y, float z) { return oct_encode(mk3(x, y, z)); }
int denoise_emul_guide_bytes(void) { return (int)sizeof(DenoiseGuide); }

}  // extern "C"

#ifdef DENOISE_EMUL_MAIN
// A 37 x 21 frame: a floor and a wall that meet at an edge, two material ids, sky holes, pixels without samples, noise on both signals;
// every iteration count, static and moving.  The filter must leave the sky pixels alone and every value finite.
int main() {
    const int W = 37, H = 21;
    const size_t n = (size_t)W * H;
    std::vector<float> pos(3 * n), hd(4 * n), hs(4 * n), hdr(3 * n), out(3 * n);
    std::vector<uint32_t> nor(n), mat(n);
    uint32_t r = 12345u;
    auto rnd = [&r] { r = r * 1664525u + 1013904223u; return (float)(r >> 8) / 16777216.0f; };
    for (int v = 0; v < H; v++)
        for (int u = 0; u < W; u++) {
            const size_t i = (size_t)v * W + u;
            const bool wall = v > 12, sky = (u * 7 + v * 3) % 23 == 0;
            pos[3 * i] = sky ? 0.0f : 0.01f * (float)u - 0.2f; pos[3 * i + 1] = sky ? 0.0f : (wall ? 0.01f * (float)(v - 12) : 0.0f) + 0.3f;
            pos[3 * i + 2] = sky ? 0.0f : (wall ? 0.12f : 0.01f * (float)v) + 0.1f;
            nor[i] = wall ? oct_encode(mk3(0.0f, 0.0f, -1.0f)) : oct_encode(mk3(0.0f, 1.0f, 0.0f));
            mat[i] = pack_material(u < 20 ? 1 : 3, mk3(0.8f, u % 5 == 0 ? 0.0f : 0.5f, 0.3f));
            const float c = (u + v) % 9 == 0 ? 0.0f : 1.0f + (float)((u * v) % 4);
            for (int a = 0; a < 3; a++) { hd[4 * i + a] = rnd(); hs[4 * i + a] = 0.2f * rnd(); hdr[3 * i + a] = 7.0f + (float)a; }
            hd[4 * i + 3] = c; hs[4 * i + 3] = c;
        }
    double sum = 0.0;
    for (int moving = 0; moving < 2; moving++)
        for (int it = 1; it <= VRT_DENOISE_MAX_ITERATIONS; it++) {
            if (denoise_emul_run(W, H, pos.data(), nor.data(), mat.data(), hd.data(), hs.data(), hdr.data(), it, 0.25f, 0.5f, 8.0f, moving, 1.0f / 64.0f, out.data())) return 2;
            for (size_t i = 0; i < n; i++) {
                const bool sky = pos[3 * i] == 0.0f && pos[3 * i + 1] == 0.0f;
                for (int a = 0; a < 3; a++) {
                    if (!(out[3 * i + a] == out[3 * i + a]) || (sky && out[3 * i + a] != hdr[3 * i + a])) { printf("pixel %zu is wrong\n", i); return 1; }
                    sum += out[3 * i + a];
                }
            }
        }
    printf("denoise_emul: %d x %d, 6 iteration counts, static and moving: finite, sky pixels untouched, sum %.6f\n", W, H, sum);
    return 0;
}
#endif
