// sensor_emul.cpp -- TEST TOOLING: vrt_gather_irradiance on the host.  The per-item functions of voxel_rt2_amd/csrc/vrt_sensor.h and the
// chunk plan of vrt_plan.h, driven the way vrt_api.hip and the two kernels of vrt_kernels.hip drive them -- samples in chunks of whole
// samples, an item's record into a scratch plane, the plane folded into the result in sample order -- on the scene record of
// tests/emul/radiance_emul.cpp (RadScene, StagedPyramid: included from there, with that file's entry points).  tests/sensor.py compiles
// this with g++ and calls it through ctypes (tests/test_sensor_host.py).  With -DSENSOR_EMUL_MAIN it is a stand-alone program over a
// small scene of its own, for a run under -fsanitize=address,undefined.
#include "radiance_emul.cpp"
#include "../../voxel_rt2_amd/csrc/vrt_sensor.h"

// vrt_gather_irradiance's chunk loop over one block of sensors (queue_sensor_block, vrt_api.hip), k_gather_irradiance's item numbering
// and k_fold_irradiance's fold.  per: whole samples a chunk (0: plan_sensor_chunk's).
template <class PyrT>
static void sensor_block(const FrameParams& fp, const SceneData& sc, const PyrT& P, long long n, const vrt_sensor* sensors, int n_samples, uint32_t first_frame,
                         int per, vrt_irradiance* out) {
    if (per < 1) per = plan_sensor_chunk(n, n_samples);
    std::vector<vrt_irradiance> plane((size_t)n * per);
    for (int s0 = 0; s0 < n_samples; s0 += per) {
        const int count = per < n_samples - s0 ? per : n_samples - s0;
        for (long long i = 0; i < n * count; i++) {
            const long long k = i % n;
            const int sample = s0 + (int)(i / n);
            plane[i] = sensor_valid(sensors[k]) ? sensor_item(fp, sc, P, sensors[k], sample, first_frame) : sensor_zero();
        }
        for (long long k = 0; k < n; k++) {
            vrt_irradiance acc = s0 == 0 ? sensor_zero() : out[k];
            acc = sensor_fold(acc, plane.data() + k, n, count);
            if (s0 + count == n_samples) acc = sensor_mean(acc, n_samples);
            out[k] = acc;
        }
    }
}
template <int G>
static void gather_g(const RadScene& s, int staged, long long n, const vrt_sensor* sensors, int n_samples, uint32_t first_frame, int per, vrt_irradiance* out) {
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
    fp.camera_is_moving = 1;   // (ignored by a query)
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
        sensor_block(fp, sc, P, n, sensors, n_samples, first_frame, per, out);
        return;
    }
    auto stage = [&](auto& P) {
        P.l0 = s.l0;
        memcpy(P.l1, s.l1, sizeof(P.l1));
        memcpy(P.l2, s.l2, sizeof(P.l2));
        P.w3 = G == 256 ? s.l3[0] : 0ULL;
        P.oob = s.ref_oob != 0;
        sensor_block(fp, sc, P, n, sensors, n_samples, first_frame, per, out);
    };
    if (s.ref_oob) { static StagedPyramid<G, true> P; stage(P); }
    else { static StagedPyramid<G, false> P; stage(P); }
}

extern "C" {

int sensor_emul_gather(const RadScene* s, int staged, long long n, const vrt_sensor* sensors, int n_samples, uint32_t first_frame, int per, vrt_irradiance* out) {
    if (!s || n < 0 || n_samples < 1 || (s->grid_res != 128 && s->grid_res != 256)) return -1;
    if (n == 0) return 0;
    if (s->grid_res == 256) gather_g<256>(*s, staged, n, sensors, n_samples, first_frame, per, out);
    else gather_g<128>(*s, staged, n, sensors, n_samples, first_frame, per, out);
    return 0;
}
int sensor_emul_valid(const vrt_sensor* s) { return sensor_valid(*s) ? 1 : 0; }
int sensor_emul_chunk(long long n_sensors, int n_samples) { return plan_sensor_chunk(n_sensors, n_samples); }
long long sensor_emul_rays(long long n) { return plan_sensor_rays(n); }
long long sensor_emul_items(void) { return VRT_SENSOR_ITEMS; }
long long sensor_emul_item_bytes(void) { return (long long)sizeof(vrt_irradiance); }
// sensor_fold / sensor_mean over `count` records laid out `stride` apart, continuing `acc`
void sensor_emul_fold(vrt_irradiance* acc, const vrt_irradiance* values, long long stride, int count, int mean_over) {
    *acc = sensor_fold(*acc, values, stride, count);
    if (mean_over > 0) *acc = sensor_mean(*acc, mean_over);
}

}  // extern "C"

#ifdef SENSOR_EMUL_MAIN
// A 128^3 grid with blocks on a floor and a roof slab over some of them, built the way k_pack_grid / k_build_l0 / k_build_coarse build
// it; 80 sensors (floor points, block tops, points under the roof, some invalid) x 5 samples at depth 5 on both views, in one chunk and
// in chunks of 2 samples.
int main() {
    constexpr int G = 128, n0 = G / 4;
    std::vector<int8_t> mat((size_t)G * G * G, 0);
    std::vector<uint32_t> grid((size_t)G * G * G, 0u);
    auto put = [&](int x, int y, int z, int m) {
        mat[((size_t)x * G + y) * G + z] = (int8_t)m;
        grid[texel_index<G>(x, y, z)] = 200u | (120u << 8) | (60u << 16) | ((uint32_t)m << 24);
    };
    for (int bx = 40; bx < 90; bx += 9) for (int bz = 40; bz < 90; bz += 9)
        for (int x = bx; x < bx + 6; x++) for (int z = bz; z < bz + 6; z++) for (int y = 54; y < 57 + (bx + bz) % 8; y++)
            put(x, y, z, ((bx + bz) % 5 == 0) ? 2 : 1 + (bx % 3));
    for (int x = 40; x < 60; x++) for (int z = 40; z < 60; z++) put(x, 70, z, 1);   // the roof
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
    s.grid_res = G; s.floor_material = 1; s.max_depth = 5; s.seed = 11u;
    s.floor_height = -0.16f; s.floor_color[0] = 0.7f; s.floor_color[1] = 0.6f; s.floor_color[2] = 0.5f; s.voxel_edges = 0.06f;
    s.background[0] = 0.2f; s.background[1] = 0.3f; s.background[2] = 0.5f;
    s.light_dir[0] = 0.2873479f; s.light_dir[1] = 0.9578263f; s.light_dir[2] = 0.0f; s.light_color[0] = 1.0f; s.light_color[1] = 0.9f; s.light_color[2] = 0.8f;
    s.light_cos_max = 0.995f; s.light_weight = 3.0f;
    for (int a = 0; a < 3; a++) { s.cull[a] = -1e30f; s.cull[3 + a] = 1e30f; }
    s.grid = grid.data(); s.l0 = l0.data(); s.l1 = l1.data(); s.l2 = l2.data(); s.l3 = l3.data(); s.mats = mats.data();
    const int n = 80, spp = 5;
    std::vector<vrt_sensor> sensors(n);
    for (int k = 0; k < n; k++) {
        vrt_sensor& r = sensors[k];
        memset(&r, 0, sizeof(r));
        r.stream = (uint32_t)(k * 5 + 2);
        r.pos[0] = (30.5f + 1.0f * (float)k) / 64.0f - 1.0f; r.pos[1] = -0.16f; r.pos[2] = (38.5f + 0.7f * (float)k) / 64.0f - 1.0f;   // the floor, partly under the roof
        r.normal[1] = 1.0f;
        if (k % 4 == 1) { r.pos[1] = 71.0f / 64.0f - 1.0f; }                                          // on or above the roof
        if (k % 4 == 2) { r.normal[0] = 0.6f; r.normal[1] = 0.0f; r.normal[2] = 0.8f; r.pos[1] = 60.5f / 64.0f - 1.0f; }   // a wall's normal
        if (k % 16 == 7) r.normal[1] = 0.0f;
        if (k % 16 == 11) r.pos[2] = DM_INF;
        if (k % 16 == 15) r.reserved = 1u;
    }
    std::vector<vrt_irradiance> a(n), b(n), c(n);
    if (sensor_emul_gather(&s, 0, n, sensors.data(), spp, 3u, 0, a.data()) || sensor_emul_gather(&s, 1, n, sensors.data(), spp, 3u, 0, b.data()) ||
        sensor_emul_gather(&s, 0, n, sensors.data(), spp, 3u, 2, c.data())) return 2;
    double sum = 0.0;
    int lit = 0, open = 0, sunny = 0;
    for (int k = 0; k < n; k++) {
        if (memcmp(&a[k], &b[k], sizeof(vrt_irradiance)) || memcmp(&a[k], &c[k], sizeof(vrt_irradiance))) { printf("sensor %d differs between views or chunkings\n", k); return 1; }
        sum += a[k].sky_rgb[0] + a[k].sky_rgb[1] + a[k].sky_rgb[2] + a[k].sun_rgb[0];
        lit += a[k].sky_rgb[1] > 0.0f;
        open += a[k].sky > 0.0f;
        sunny += a[k].sun > 0.0f;
    }
    printf("sensor_emul: %d sensors x %d samples, %d lit, %d see sky, %d see the sun, sum %.6f: views and chunkings agree\n", n, spp, lit, open, sunny, sum);
    return lit > n / 2 && open > n / 4 && sunny > n / 8 ? 0 : 1;
}
#endif
