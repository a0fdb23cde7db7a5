// sensor_emul.cpp -- TEST TOOLING: vrt_gather_irradiance on the host.  The per-item functions of voxel_rt2_amd/csrc/vrt_sensor.h under the
// sampled queries' host loop (tests/emul/query_emul.h: the chunk plan of vrt_plan.h, an item's record into a scratch plane, the plane
// folded into the result in sample order) on the scene record of the radiance query (RadScene).  tests/sensor.py compiles this with g++
// and calls it through ctypes (tests/test_sensor_host.py).  With -DSENSOR_EMUL_MAIN it is a stand-alone program over a small scene of
// its own, for a run under -fsanitize=address,undefined.
#include <cstdio>
#include "query_emul.h"

extern "C" {

// k_gather_irradiance's item: an invalid sensor's record is all zeros.
int sensor_emul_gather(const RadScene* s, int staged, long long n, const vrt_sensor* sensors, int n_samples, uint32_t first_frame, int per, vrt_irradiance* out) {
    return query_run<SensorQuery>(s, staged, n, sensors, n_samples, per, out,
                                  [first_frame](const FrameParams& fp, const SceneData& sc, const auto& P, const vrt_sensor& r, int sample, vrt_irradiance&) {
        return sensor_valid(r) ? sensor_item(fp, sc, P, r, sample, first_frame) : SensorQuery::zero();
    });
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

// the mode of the frame parameters every later call hands the device functions (query_emul.h): 0 plain, 1 poisoned; returns the mode before
int sensor_emul_poison(int on) { const int was = g_query_poison; g_query_poison = on ? 1 : 0; return was; }
// frame_params_probe on the record a call on scene `s` would hand over in the current mode: float out[8], int32 ints[4]
void sensor_emul_probe(const RadScene* s, float* out, int32_t* ints) {
    FrameParams fp;
    SceneData sc;
    scene_sampled(*s, fp, sc);
    frame_params_probe(fp, out, ints);
}

}  // extern "C"

#ifdef SENSOR_EMUL_MAIN
// SmallScene with the roof; 80 sensors (floor points, block tops, points under the roof, some invalid) x 5 samples at depth 5 on both
// views, in one chunk and in chunks of 2 samples; then once more with the poisoned frame parameters.
int main() {
    SmallScene scene(true, 5);
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
    std::vector<vrt_irradiance> a(n), b(n), c(n), d(n);
    if (sensor_emul_gather(&scene.s, 0, n, sensors.data(), spp, 3u, 0, a.data()) || sensor_emul_gather(&scene.s, 1, n, sensors.data(), spp, 3u, 0, b.data()) ||
        sensor_emul_gather(&scene.s, 0, n, sensors.data(), spp, 3u, 2, c.data())) return 2;
    sensor_emul_poison(1);   // the frame parameters no query reads, poisoned (query_emul.h): the same bytes
    if (sensor_emul_gather(&scene.s, 1, n, sensors.data(), spp, 3u, 2, d.data())) return 2;
    sensor_emul_poison(0);
    if (memcmp(a.data(), d.data(), n * sizeof(vrt_irradiance))) { printf("the poisoned frame parameters changed a sensor\n"); return 1; }
    double sum = 0.0;
    int lit = 0, open = 0, sunny = 0;
    for (int k = 0; k < n; k++) {
        if (memcmp(&a[k], &b[k], sizeof(vrt_irradiance)) || memcmp(&a[k], &c[k], sizeof(vrt_irradiance))) { printf("sensor %d differs between views or chunkings\n", k); return 1; }
        sum += a[k].sky_rgb[0] + a[k].sky_rgb[1] + a[k].sky_rgb[2] + a[k].sun_rgb[0];
        lit += a[k].sky_rgb[1] > 0.0f;
        open += a[k].sky > 0.0f;
        sunny += a[k].sun > 0.0f;
    }
    printf("sensor_emul: %d sensors x %d samples, %d lit, %d see sky, %d see the sun, sum %.6f: views and chunkings agree, poisoned frame parameters change nothing\n", n, spp, lit, open, sunny, sum);
    return lit > n / 2 && open > n / 4 && sunny > n / 8 ? 0 : 1;
}
#endif
