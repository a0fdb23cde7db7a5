// radiance_emul.cpp -- TEST TOOLING: vrt_trace_radiance on the host.  The per-item functions of voxel_rt2_amd/csrc/vrt_radiance.h under the
// sampled queries' host loop (tests/emul/query_emul.h: the chunk plan of vrt_plan.h, an item's value into a scratch plane, the plane
// folded into the result in sample order) on a pyramid, texel grid, material table and sky tables the test hands over.
// tests/radiance.py compiles this with g++ and calls it through ctypes (tests/test_radiance_host.py).  With -DRADIANCE_EMUL_MAIN it is a
// stand-alone program over a small scene of its own, for a run under -fsanitize=address,undefined.
#include <cstdio>
#include "query_emul.h"

extern "C" {

// k_trace_radiance's item: an invalid ray is worth zero; sample 0 (of the call) also leaves the first hit's distance in the record.
int radiance_emul_trace(const RadScene* s, int staged, long long n, const vrt_path_ray* rays, int n_samples, uint32_t first_frame, int per, vrt_radiance* out) {
    return query_run<RadianceQuery>(s, staged, n, rays, n_samples, per, out,
                                    [first_frame](const FrameParams& fp, const SceneData& sc, const auto& P, const vrt_path_ray& r, int sample, vrt_radiance& o) {
        float t = DM_INF;
        const f3 v = radiance_ray_valid(r) ? radiance_item(fp, sc, P, r, sample, first_frame, t) : RadianceQuery::zero();
        if (sample == 0) o.t = t;
        return v;
    });
}
int radiance_emul_valid(const vrt_path_ray* r) { return radiance_ray_valid(*r) ? 1 : 0; }
int radiance_emul_chunk(long long n_rays, int n_samples) { return plan_radiance_chunk(n_rays, n_samples); }
long long radiance_emul_rays(long long n) { return plan_radiance_rays(n); }
long long radiance_emul_items(void) { return VRT_RADIANCE_ITEMS; }
int radiance_emul_staged(long long items, int knob) { return plan_radiance_staged(items, knob) ? 1 : 0; }

// the mode of the frame parameters every later call hands the device functions (query_emul.h): 0 plain, 1 poisoned; returns the mode before
int radiance_emul_poison(int on) { const int was = g_query_poison; g_query_poison = on ? 1 : 0; return was; }
// frame_params_probe on the record a call on scene `s` would hand over in the current mode: float out[8], int32 ints[4]
void radiance_emul_probe(const RadScene* s, float* out, int32_t* ints) {
    FrameParams fp;
    SceneData sc;
    scene_sampled(*s, fp, sc);
    frame_params_probe(fp, out, ints);
}

}  // extern "C"

#ifdef RADIANCE_EMUL_MAIN
// SmallScene without the roof; 96 rays (a fan from above, some from inside a block, some invalid) x 5 samples at depth 6 on both views,
// in one chunk and in chunks of 2 samples; then once more with the poisoned frame parameters.
int main() {
    SmallScene scene(false, 6);
    const int n = 96, spp = 5;
    std::vector<vrt_path_ray> rays(n);
    for (int k = 0; k < n; k++) {
        vrt_path_ray& r = rays[k];
        memset(&r, 0, sizeof(r));
        r.stream = (uint32_t)(k * 7 + 1);
        const float a = 0.0654f * (float)k, e = -0.9f + 0.02f * (float)k;
        f3 d = norm3(mk3(dm_cos(a), e, dm_sin(a)));
        r.origin[0] = 0.05f; r.origin[1] = 0.4f; r.origin[2] = -0.03f;
        if (k % 8 == 5) { r.origin[0] = 42.5f / 64.0f - 1.0f; r.origin[1] = 55.5f / 64.0f - 1.0f; r.origin[2] = 42.5f / 64.0f - 1.0f; }   // inside a block
        r.dir[0] = d.x; r.dir[1] = d.y; r.dir[2] = d.z;
        if (k % 16 == 9) r.dir[0] = r.dir[1] = r.dir[2] = 0.0f;
        if (k % 16 == 11) r.origin[1] = DM_INF;
    }
    std::vector<vrt_radiance> a(n), b(n), c(n), d(n);
    if (radiance_emul_trace(&scene.s, 0, n, rays.data(), spp, 3u, 0, a.data()) || radiance_emul_trace(&scene.s, 1, n, rays.data(), spp, 3u, 0, b.data()) ||
        radiance_emul_trace(&scene.s, 0, n, rays.data(), spp, 3u, 2, c.data())) return 2;
    radiance_emul_poison(1);   // the frame parameters no query reads, poisoned (query_emul.h): the same bytes
    if (radiance_emul_trace(&scene.s, 1, n, rays.data(), spp, 3u, 2, d.data())) return 2;
    radiance_emul_poison(0);
    if (memcmp(a.data(), d.data(), n * sizeof(vrt_radiance))) { printf("the poisoned frame parameters changed a ray\n"); return 1; }
    double sum = 0.0;
    int lit = 0, hits = 0;
    for (int k = 0; k < n; k++) {
        if (memcmp(&a[k], &b[k], sizeof(vrt_radiance)) || memcmp(&a[k], &c[k], sizeof(vrt_radiance))) { printf("ray %d differs between views or chunkings\n", k); return 1; }
        sum += a[k].rgb[0] + a[k].rgb[1] + a[k].rgb[2];
        lit += a[k].rgb[1] > 0.0f;
        hits += a[k].t < DM_INF;
    }
    printf("radiance_emul: %d rays x %d samples, %d lit, %d hit something, sum %.6f: views and chunkings agree, poisoned frame parameters change nothing\n", n, spp, lit, hits, sum);
    return lit > n / 2 && hits > n / 4 ? 0 : 1;
}
#endif
