// radiance_emul.cpp -- TEST TOOLING: vrt_trace_radiance on the host.  The per-item functions of voxel_rt2_amd/csrc/vrt_radiance.h and the
// chunk plan of vrt_plan.h, driven the way vrt_api.hip and the two kernels of vrt_kernels.hip drive them -- samples in chunks of whole
// samples, an item's value into a scratch plane, the plane folded into the result in sample order -- on a pyramid, texel grid, material
// table and sky tables the test hands over.  tests/radiance.py compiles this with g++ and calls it through ctypes
// (tests/test_radiance_host.py).  With -DRADIANCE_EMUL_MAIN it is a stand-alone program over a small scene of its own, for a run under
// -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../voxel_rt2_amd/csrc/vrt_radiance.h"
#include "../../voxel_rt2_amd/csrc/vrt_plan.h"

using namespace vrt;

// The staged view of the kernel (LdsPyramid, vrt_kernels.hip: device only) restated for the host, as tests/emul/cast_emul.cpp has it.
template <int G_, bool OOB_>
struct StagedPyramid {
    static constexpr int G = G_;
    static constexpr bool flat_descend = false;
    static constexpr bool cull = true;
    static constexpr bool oob_capable = OOB_;
    bool oob;
    bool oob_ref() const { return oob; }
    const unsigned long long* l0;
    unsigned long long l1[GridDim<G_>::n1 * GridDim<G_>::n1 * GridDim<G_>::n1];
    unsigned long long l2[GridDim<G_>::n2 * GridDim<G_>::n2 * GridDim<G_>::n2];
    unsigned long long w3;
    unsigned long long load_l0(int i) const { return l0[i]; }
    unsigned long long load_l1(int i) const { return l1[i]; }
    unsigned long long load_l2(int i) const { return l2[i]; }
    unsigned long long load_l3() const { return w3; }
};

struct RadScene {   // what tests/radiance.py fills (ctypes mirror there)
    int32_t grid_res, ref_oob, floor_material, use_sky, max_depth, sky_res;
    uint32_t seed;
    int32_t pad;
    float floor_height, floor_color[3], voxel_edges, background[3], light_dir[3], light_color[3], light_cos_max, light_weight;
    float cull[8];   // the box the walks test rays against (k_cull_box's, or the open one)
    const uint32_t* grid;
    const unsigned long long *l0, *l1, *l2, *l3;
    const float *mats, *sky_scat, *sky_trans;
};

// vrt_trace_radiance's chunk loop over one block of rays (queue_radiance_block, vrt_api.hip), k_trace_radiance's item numbering and
// k_fold_radiance's fold.  per: whole samples a chunk (0: plan_radiance_chunk's).
template <class PyrT>
static void block(const FrameParams& fp, const SceneData& sc, const PyrT& P, long long n, const vrt_path_ray* rays, int n_samples, uint32_t first_frame,
                  int per, vrt_radiance* out) {
    if (per < 1) per = plan_radiance_chunk(n, n_samples);
    std::vector<f3> plane((size_t)n * per);
    for (int s0 = 0; s0 < n_samples; s0 += per) {
        const int count = per < n_samples - s0 ? per : n_samples - s0;
        for (long long i = 0; i < n * count; i++) {
            const long long ray = i % n;
            const int sample = s0 + (int)(i / n);
            float t = DM_INF;
            plane[i] = radiance_ray_valid(rays[ray]) ? radiance_item(fp, sc, P, rays[ray], sample, first_frame, t) : mk3(0.0f);
            if (sample == 0) out[ray].t = t;
        }
        for (long long ray = 0; ray < n; ray++) {
            f3 acc = s0 == 0 ? mk3(0.0f) : mk3(out[ray].rgb[0], out[ray].rgb[1], out[ray].rgb[2]);
            acc = radiance_fold(acc, plane.data() + ray, n, count);
            if (s0 + count == n_samples) acc = radiance_mean(acc, n_samples);
            out[ray].rgb[0] = acc.x; out[ray].rgb[1] = acc.y; out[ray].rgb[2] = acc.z;
        }
    }
}
template <int G>
static void trace_g(const RadScene& s, int staged, long long n, const vrt_path_ray* rays, int n_samples, uint32_t first_frame, int per, vrt_radiance* out) {
    FrameParams fp;
    memset(&fp, 0, sizeof(fp));
    fp.floor_height = s.floor_height;
    fp.floor_color = mk3(s.floor_color[0], s.floor_color[1], s.floor_color[2]);
    fp.floor_material = s.floor_material;
    fp.voxel_edges = s.voxel_edges;
    fp.background = mk3(s.background[0], s.background[1], s.background[2]);
    fp.light_dir = mk3(s.light_dir[0], s.light_dir[1], s.light_dir[2]);
    fp.light_color = mk3(s.light_color[0], s.light_color[1], s.light_color[2]);
    fp.light_cos_max = s.light_cos_max;
    fp.light_weight = s.light_weight;
    fp.use_sky = s.use_sky;
    fp.max_depth = s.max_depth;
    fp.seed = s.seed;
    fp.camera_is_moving = 1;   // (ignored by a query: were it read, the demodulation would show)
    SceneData sc;
    memset(&sc, 0, sizeof(sc));
    sc.pyr.l0 = s.l0; sc.pyr.l1 = s.l1; sc.pyr.l2 = s.l2; sc.pyr.l3 = s.l3;
    sc.pyr.ref_oob = s.ref_oob;
    sc.grid = s.grid;
    sc.mats = s.mats;
    sc.sky.scattering = s.sky_scat; sc.sky.transmittance = s.sky_trans;
    sc.sky.res = s.sky_res; sc.sky.fres = s.sky_res > 0 ? (float)(1.0 / (double)s.sky_res) : 0.0f;
    sc.cull = s.cull;
    if (!staged) {
        GlobalPyramid<G> P;
        P.p = sc.pyr;
        block(fp, sc, P, n, rays, n_samples, first_frame, per, out);
        return;
    }
    auto stage = [&](auto& P) {
        P.l0 = s.l0;
        memcpy(P.l1, s.l1, sizeof(P.l1));
        memcpy(P.l2, s.l2, sizeof(P.l2));
        P.w3 = G == 256 ? s.l3[0] : 0ULL;
        P.oob = s.ref_oob != 0;
        block(fp, sc, P, n, rays, n_samples, first_frame, per, out);
    };
    if (s.ref_oob) { static StagedPyramid<G, true> P; stage(P); }
    else { static StagedPyramid<G, false> P; stage(P); }
}

extern "C" {

int radiance_emul_trace(const RadScene* s, int staged, long long n, const vrt_path_ray* rays, int n_samples, uint32_t first_frame, int per, vrt_radiance* out) {
    if (!s || n < 0 || n_samples < 1 || (s->grid_res != 128 && s->grid_res != 256)) return -1;
    if (n == 0) return 0;
    if (s->grid_res == 256) trace_g<256>(*s, staged, n, rays, n_samples, first_frame, per, out);
    else trace_g<128>(*s, staged, n, rays, n_samples, first_frame, per, out);
    return 0;
}
int radiance_emul_valid(const vrt_path_ray* r) { return radiance_ray_valid(*r) ? 1 : 0; }
int radiance_emul_chunk(long long n_rays, int n_samples) { return plan_radiance_chunk(n_rays, n_samples); }
long long radiance_emul_rays(long long n) { return plan_radiance_rays(n); }
long long radiance_emul_items(void) { return VRT_RADIANCE_ITEMS; }
int radiance_emul_staged(long long items, int knob) { return plan_radiance_staged(items, knob) ? 1 : 0; }

}  // extern "C"

#ifdef RADIANCE_EMUL_MAIN
// A 128^3 grid with a few blocks on a floor, built here the way k_pack_grid / k_build_l0 / k_build_coarse build it; 96 rays (a fan from
// above, some from inside a block, some invalid) x 5 samples at depth 6 on both views, in one chunk and in chunks of 2 samples.
int main() {
    constexpr int G = 128, n0 = G / 4;
    std::vector<int8_t> mat((size_t)G * G * G, 0);
    std::vector<uint32_t> grid((size_t)G * G * G, 0u);
    for (int bx = 40; bx < 90; bx += 9) for (int bz = 40; bz < 90; bz += 9)
        for (int x = bx; x < bx + 6; x++) for (int z = bz; z < bz + 6; z++) for (int y = 54; y < 57 + (bx + bz) % 8; y++) {
            const int m = ((bx + bz) % 5 == 0) ? 2 : 1 + (bx % 3);
            mat[((size_t)x * G + y) * G + z] = (int8_t)m;
            grid[texel_index<G>(x, y, z)] = 200u | (120u << 8) | (60u << 16) | ((uint32_t)m << 24);
        }
    std::vector<unsigned long long> l0((size_t)n0 * n0 * n0, 0), l1(512, 0), l2(8, 0), l3(1, 0);
    for (int b = 0; b < n0 * n0 * n0; b++) {
        const int bx = b % n0, by = (b / n0) % n0, bz = b / (n0 * n0);
        for (int z = 0; z < 4; z++) for (int y = 0; y < 4; y++) for (int x = 0; x < 4; x++)
            if (mat[((size_t)(bx * 4 + x) * G + (by * 4 + y)) * G + (bz * 4 + z)] > 0) l0[b] |= 1ULL << (z * 16 + y * 4 + x);
    }
    auto coarse = [](const std::vector<unsigned long long>& fine, std::vector<unsigned long long>& out, int nc) {
        const int nf = nc * 4;
        for (int b = 0; b < nc * nc * nc; b++) {
            const int bx = b % nc, by = (b / nc) % nc, bz = b / (nc * nc);
            for (int z = 0; z < 4; z++) for (int y = 0; y < 4; y++) for (int x = 0; x < 4; x++)
                if (fine[((bz * 4 + z) * nf + (by * 4 + y)) * nf + (bx * 4 + x)] != 0) out[b] |= 1ULL << (z * 16 + y * 4 + x);
        }
    };
    coarse(l0, l1, G / 16);
    coarse(l1, l2, G / 64);
    std::vector<float> mats(128 * 14, 0.0f);
    for (int id = 0; id < 128; id++) { float* p = &mats[14 * id]; p[0] = p[1] = p[2] = 1.0f; p[5] = 0.5f; p[7] = 0.3f + 0.2f * (id % 3); p[4] = id == 3 ? 0.8f : 0.0f; p[12] = 1.0f; p[13] = 0.5f; }
    RadScene s;
    memset(&s, 0, sizeof(s));
    s.grid_res = G; s.floor_material = 1; s.max_depth = 6; s.seed = 11u;
    s.floor_height = -0.16f; s.floor_color[0] = 0.7f; s.floor_color[1] = 0.6f; s.floor_color[2] = 0.5f; s.voxel_edges = 0.06f;
    s.background[0] = 0.2f; s.background[1] = 0.3f; s.background[2] = 0.5f;
    s.light_dir[0] = 0.2873479f; s.light_dir[1] = 0.9578263f; s.light_dir[2] = 0.0f; s.light_color[0] = 1.0f; s.light_color[1] = 0.9f; s.light_color[2] = 0.8f;
    s.light_cos_max = 0.995f; s.light_weight = 3.0f;
    for (int a = 0; a < 3; a++) { s.cull[a] = -1e30f; s.cull[3 + a] = 1e30f; }
    s.grid = grid.data(); s.l0 = l0.data(); s.l1 = l1.data(); s.l2 = l2.data(); s.l3 = l3.data(); s.mats = mats.data();
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
    std::vector<vrt_radiance> a(n), b(n), c(n);
    if (radiance_emul_trace(&s, 0, n, rays.data(), spp, 3u, 0, a.data()) || radiance_emul_trace(&s, 1, n, rays.data(), spp, 3u, 0, b.data()) ||
        radiance_emul_trace(&s, 0, n, rays.data(), spp, 3u, 2, c.data())) return 2;
    double sum = 0.0;
    int lit = 0, hits = 0;
    for (int k = 0; k < n; k++) {
        if (memcmp(&a[k], &b[k], sizeof(vrt_radiance)) || memcmp(&a[k], &c[k], sizeof(vrt_radiance))) { printf("ray %d differs between views or chunkings\n", k); return 1; }
        sum += a[k].rgb[0] + a[k].rgb[1] + a[k].rgb[2];
        lit += a[k].rgb[1] > 0.0f;
        hits += a[k].t < DM_INF;
    }
    printf("radiance_emul: %d rays x %d samples, %d lit, %d hit something, sum %.6f: views and chunkings agree\n", n, spp, lit, hits, sum);
    return lit > n / 2 && hits > n / 4 ? 0 : 1;
}
#endif
