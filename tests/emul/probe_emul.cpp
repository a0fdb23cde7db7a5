// probe_emul.cpp -- TEST TOOLING: vrt_gather_probes on the host.  The per-item functions of voxel_rt2_amd/csrc/vrt_probe_sh.h under the
// sampled queries' host loop (tests/emul/query_emul.h: the chunk plan of vrt_plan.h, an item's record into a scratch plane, the plane
// folded into the result in sample order) on the scene record of the radiance query (RadScene).  tests/probe.py compiles this with g++
// and calls it through ctypes (tests/test_probe_host.py).  With -DPROBE_EMUL_MAIN it is a stand-alone program over a small scene of
// its own, for a run under -fsanitize=address,undefined.
#include <cstdio>
#include "query_emul.h"

extern "C" {

// k_gather_probes' item: an invalid probe's item is all zeros.
int probe_emul_gather(const RadScene* s, int staged, long long n, const vrt_probe* probes, int n_samples, uint32_t first_frame, int per, vrt_sh_probe* out) {
    return query_run<ProbeQuery>(s, staged, n, probes, n_samples, per, out,
                                 [first_frame](const FrameParams& fp, const SceneData& sc, const auto& P, const vrt_probe& r, int sample, vrt_sh_probe&) {
        return probe_valid(r) ? probe_item(fp, sc, P, r, sample, first_frame) : ProbeQuery::zero();
    });
}
int probe_emul_valid(const vrt_probe* q) { return probe_valid(*q) ? 1 : 0; }
int probe_emul_chunk(long long n_probes, int n_samples) { return plan_probe_chunk(n_probes, n_samples); }
long long probe_emul_rays(long long n) { return plan_probe_rays(n); }
long long probe_emul_items(void) { return VRT_PROBE_ITEMS; }
long long probe_emul_item_bytes(void) { return (long long)sizeof(ProbeItem); }
// probe_basis at (x, y, z): float out[9]
void probe_emul_basis(float x, float y, float z, float* out) {
    float Y[9];
    probe_basis(x, y, z, Y);
    for (int i = 0; i < 9; i++) out[i] = Y[i];
}
// probe_fold / probe_mean over `count` items laid out `stride` apart, continuing `acc`
void probe_emul_fold(vrt_sh_probe* acc, const ProbeItem* values, long long stride, int count, int mean_over) {
    *acc = probe_fold(*acc, values, stride, count);
    if (mean_over > 0) *acc = probe_mean(*acc, mean_over);
}

// the mode of the frame parameters every later call hands the device functions (query_emul.h): 0 plain, 1 poisoned; returns the mode before
int probe_emul_poison(int on) { const int was = g_query_poison; g_query_poison = on ? 1 : 0; return was; }
// frame_params_probe on the record a call on scene `s` would hand over in the current mode: float out[8], int32 ints[4]
void probe_emul_probe(const RadScene* s, float* out, int32_t* ints) {
    FrameParams fp;
    SceneData sc;
    scene_sampled(*s, fp, sc);
    frame_params_probe(fp, out, ints);
}

}  // extern "C"

#ifdef PROBE_EMUL_MAIN
// SmallScene with the roof; 80 probes (open air, under the roof, inside blocks, below the floor, outside the grid, some invalid) x 5
// samples at depth 5 on both views, in one chunk and in chunks of 2 samples; then once more with the poisoned frame parameters.
int main() {
    SmallScene scene(true, 5);
    const int n = 80, spp = 5;
    std::vector<vrt_probe> probes(n);
    for (int k = 0; k < n; k++) {
        vrt_probe& r = probes[k];
        memset(&r, 0, sizeof(r));
        r.stream = (uint32_t)(k * 5 + 2);
        r.pos[0] = (30.5f + 1.0f * (float)k) / 64.0f - 1.0f; r.pos[1] = 75.5f / 64.0f - 1.0f; r.pos[2] = (38.5f + 0.7f * (float)k) / 64.0f - 1.0f;   // open air
        if (k % 4 == 1) r.pos[1] = 66.5f / 64.0f - 1.0f;      // partly under the roof
        if (k % 4 == 2) r.pos[1] = 55.5f / 64.0f - 1.0f;      // among and inside the blocks
        if (k % 16 == 3) r.pos[1] = -0.5f;                    // below the floor
        if (k % 16 == 7) r.pos[0] = 1.05f;                    // outside the grid
        if (k % 16 == 11) r.pos[2] = DM_INF;
        if (k % 16 == 15) r.pos[1] = -DM_INF;
    }
    std::vector<vrt_sh_probe> a(n), b(n), c(n), d(n);
    if (probe_emul_gather(&scene.s, 0, n, probes.data(), spp, 3u, 0, a.data()) || probe_emul_gather(&scene.s, 1, n, probes.data(), spp, 3u, 0, b.data()) ||
        probe_emul_gather(&scene.s, 0, n, probes.data(), spp, 3u, 2, c.data())) return 2;
    probe_emul_poison(1);   // the frame parameters no query reads, poisoned (query_emul.h): the same bytes
    if (probe_emul_gather(&scene.s, 1, n, probes.data(), spp, 3u, 2, d.data())) return 2;
    probe_emul_poison(0);
    if (memcmp(a.data(), d.data(), n * sizeof(vrt_sh_probe))) { printf("the poisoned frame parameters changed a probe\n"); return 1; }
    double sum = 0.0;
    int lit = 0, open = 0, sunny = 0;
    for (int k = 0; k < n; k++) {
        if (memcmp(&a[k], &b[k], sizeof(vrt_sh_probe)) || memcmp(&a[k], &c[k], sizeof(vrt_sh_probe))) { printf("probe %d differs between views or chunkings\n", k); return 1; }
        sum += a[k].sh[0][0] + a[k].sh[0][1] + a[k].sh[0][2] + a[k].sun_rgb[0];
        lit += a[k].sh[0][1] > 0.0f;
        open += a[k].sky > 0.0f;
        sunny += a[k].sun > 0.0f;
    }
    printf("probe_emul: %d probes x %d samples, %d lit, %d see sky, %d see the sun, sum %.6f: views and chunkings agree, poisoned frame parameters change nothing\n", n, spp, lit, open, sunny, sum);
    return lit > n / 2 && open > n / 4 && sunny > n / 8 ? 0 : 1;
}
#endif
