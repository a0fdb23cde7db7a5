// sensor_orc.cpp -- TEST TOOLING: the parts of vrt_gather_irradiance (include/vrt_api.h) that the oracle can state on its own.  This
// translation unit includes the oracle's sources unchanged -- so the library it builds into (tests/emul/_sensor_orc.so, tests/sensor.py)
// carries every orc_* entry point -- and adds one function over the oracle's own sample_cone_oriented,
// sample_cosine_weighted_hemisphere, next_hit, sample_skybox_transmittance, sample_skybox, firefly_filter and scrub_needed.  Per
// (sensor, sample) it returns the ray origin, the sun sample and its term, the hemisphere direction, whether the first segment escapes,
// whether that direction lies inside the sun's cone, and for an escape the sky-only value.  What a NON-escaping hemisphere ray is
// worth is not computed here: that is the radiance query's value for ray (o, w, stream), which tests/sensor.py takes from the
// radiance query (already pinned to the oracle's render_pixel by tests/test_radiance_host.py and tests/test_gpu_radiance.py).
#include "../../oracle/orc_api.cpp"

extern "C" {

enum { SENSOR_ORC_ROW = 20 };
// out: n * n_samples rows (sensor-major: row = k * n_samples + s) of SENSOR_ORC_ROW floats:
//   [0..2] o   [3..5] ldir   [6] ndl   [7] vis_s   [8..10] sun_s   [11..13] w   [14] escapes   [15] w inside the cone   [16..18] sky-only value   [19] 0
int orc_sensor_samples(orc_ctx* c, int n, const vrt_sensor* sensors, int n_samples, uint32_t first_frame, float* out) {
    Renderer& r = c->r;
    if (n < 0 || n_samples < 1) return -1;
    for (int k = 0; k < n; k++) {
        const vrt_sensor& sn = sensors[k];
        const V3 normal = v3(sn.normal[0], sn.normal[1], sn.normal[2]);
        for (int s = 0; s < n_samples; s++) {
            float* row = out + ((size_t)k * n_samples + s) * SENSOR_ORC_ROW;
            const uint32_t f = first_frame + (uint32_t)s;
            /* 1. streams, origin (pathtracer.py:428: pos = hit_pos + normal * EPS) */
            dm_rng g = dm_rng_init(r.seed, f, sn.stream, 4u);
            const V3 o = v3(sn.pos[0], sn.pos[1], sn.pos[2]) + normal * EPS;
            /* 2. the sun (pathtracer.py:436-468 without the BSDF and MIS factors) */
            const V3 ldir = sample_cone_oriented(r.light_cone_cos_theta_max, r.light_direction, &g);
            const float ndl = dot(ldir, normal);
            float vis = 0.0f;
            V3 sun = v3(0.0f);
            if (ndl > 0.0f) {
                float dist;
                V3 n_, a_;
                int hl_, sm_;
                r.next_hit(o, ldir, INF, true, nullptr, &dist, &n_, &a_, &hl_, &sm_);
                if (dist >= INF) {
                    vis = 1.0f;
                    V3 sky_T = v3(1.0f);
                    if (r.use_physical_atmosphere == 1) sky_T = r.atmos.sample_skybox_transmittance(ldir);
                    sun = sky_T * r.light_weight * r.light_color * ndl;
                }
            }
            /* 3. the hemisphere */
            const V3 w = sample_cosine_weighted_hemisphere(normal, &g);
            float closest;
            V3 hn, ha;
            int hl, hm;
            r.next_hit(o, w, INF, false, nullptr, &closest, &hn, &ha, &hl, &hm);
            const bool escapes = closest == INF;
            const bool in_cone = dot(r.light_direction, w) >= r.light_cone_cos_theta_max;
            V3 value = v3(0.0f);
            if (escapes) {
                /* render_pixel's escape at depth 0 (pathtracer.py:500-517) on a fresh stream-0 state, with hit_sun = 0, then its two
                 * colours (:611-619: lobe 0, no emissive primary, no light sample), scrubbed and added */
                dm_rng rng = dm_rng_init(r.seed, f, sn.stream, 0u);
                const float hit_sun = 0.0f;
                V3 sky_scattering = r.background_color;
                V3 sky_T = v3(1.0f);
                if (r.use_physical_atmosphere == 1) r.atmos.sample_skybox(w, &rng, &sky_scattering, &sky_T);
                const V3 sky_emission = firefly_filter(sky_scattering + sky_T * r.light_weight * r.light_color * hit_sun);
                V3 contrib = v3(0.0f);
                const V3 throughput = v3(1.0f);
                contrib += throughput * sky_emission;
                const float first_bounce_invpdf = 1.0f;
                V3 diffuse = v3(0.0f), specular = v3(0.0f);
                diffuse += contrib * first_bounce_invpdf + v3(0.0f);
                diffuse += v3(0.0f);
                specular += v3(0.0f);
                if (Renderer::scrub_needed(diffuse)) diffuse = v3(0.0f);
                if (Renderer::scrub_needed(specular)) specular = v3(0.0f);
                value = diffuse + specular;
            }
            row[0] = o.x; row[1] = o.y; row[2] = o.z;
            row[3] = ldir.x; row[4] = ldir.y; row[5] = ldir.z;
            row[6] = ndl; row[7] = vis;
            row[8] = sun.x; row[9] = sun.y; row[10] = sun.z;
            row[11] = w.x; row[12] = w.y; row[13] = w.z;
            row[14] = escapes ? 1.0f : 0.0f; row[15] = in_cone ? 1.0f : 0.0f;
            row[16] = value.x; row[17] = value.y; row[18] = value.z; row[19] = 0.0f;
        }
    }
    return 0;
}

}  // extern "C"
