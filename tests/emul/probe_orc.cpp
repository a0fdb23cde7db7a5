// probe_orc.cpp -- TEST TOOLING: the parts of vrt_gather_probes (include/vrt_api.h) that the oracle can state on its own.  This
// translation unit includes the oracle's sources unchanged -- so the library it builds into (tests/emul/_probe_orc.so, tests/probe.py)
// carries every orc_* entry point -- and adds one function over the oracle's own sample_cone_oriented, random draws and vector
// functions, next_hit, sample_skybox_transmittance, sample_skybox, firefly_filter and scrub_needed.  Per (probe, sample) it returns the
// sun sample and its term, the sphere direction, whether the first segment escapes, whether that direction lies inside the sun's cone,
// and for an escape the sky-only value.  What a NON-escaping ray is worth is not computed here: that is the radiance query's value for
// ray (pos, w, stream), which tests/probe.py takes from the radiance query (pinned to the oracle's render_pixel by
// tests/test_radiance_host.py and tests/test_gpu_radiance.py).
#include "../../oracle/orc_api.cpp"

extern "C" {

enum { PROBE_ORC_ROW = 16 };
// out: n * n_samples rows (probe-major: row = k * n_samples + s) of PROBE_ORC_ROW floats:
//   [0..2] ldir   [3] vis_s   [4..6] sun_s   [7..9] w   [10] escapes   [11] w inside the cone   [12..14] sky-only value   [15] 0
int orc_probe_samples(orc_ctx* c, int n, const vrt_probe* probes, int n_samples, uint32_t first_frame, float* out) {
    Renderer& r = c->r;
    if (n < 0 || n_samples < 1) return -1;
    for (int k = 0; k < n; k++) {
        const vrt_probe& pr = probes[k];
        const V3 pos = v3(pr.pos[0], pr.pos[1], pr.pos[2]);
        for (int s = 0; s < n_samples; s++) {
            float* row = out + ((size_t)k * n_samples + s) * PROBE_ORC_ROW;
            const uint32_t f = first_frame + (uint32_t)s;
            /* 1. the probe's stream */
            dm_rng g = dm_rng_init(r.seed, f, pr.stream, 5u);
            /* 2. the sun: always a shadow ray, no ndl */
            const V3 ldir = sample_cone_oriented(r.light_cone_cos_theta_max, r.light_direction, &g);
            float vis = 0.0f;
            V3 sun = v3(0.0f);
            {
                float dist;
                V3 n_, a_;
                int hl_, sm_;
                r.next_hit(pos, ldir, INF, true, nullptr, &dist, &n_, &a_, &hl_, &sm_);
                if (dist >= INF) {
                    vis = 1.0f;
                    V3 sky_T = v3(1.0f);
                    if (r.use_physical_atmosphere == 1) sky_T = r.atmos.sample_skybox_transmittance(ldir);
                    sun = sky_T * r.light_weight * r.light_color;
                }
            }
            /* 3. the sphere: sample_cosine_weighted_hemisphere's lines (orc_math.h) without the normal and without the shrink */
            const float u0 = dm_rng_f32(&g);
            const float u1 = dm_rng_f32(&g);
            const float a = 1.0f - 2.0f * u0;
            const float b = dm_sqrt(1.0f - a * a);
            const float phi = DM_TWO_PI * u1;
            const V3 w = normalized(v3(b * dm_cos(phi), b * dm_sin(phi), a));
            float closest;
            V3 hn, ha;
            int hl, hm;
            r.next_hit(pos, w, INF, false, nullptr, &closest, &hn, &ha, &hl, &hm);
            const bool escapes = closest == INF;
            const bool in_cone = dot(r.light_direction, w) >= r.light_cone_cos_theta_max;
            V3 value = v3(0.0f);
            if (escapes) {
                /* render_pixel's escape at depth 0 (pathtracer.py:500-517) on a fresh stream-0 state, with hit_sun = 0, then its two
                 * colours (:611-619: lobe 0, no emissive primary, no light sample), scrubbed and added */
                dm_rng rng = dm_rng_init(r.seed, f, pr.stream, 0u);
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
            row[0] = ldir.x; row[1] = ldir.y; row[2] = ldir.z; row[3] = vis;
            row[4] = sun.x; row[5] = sun.y; row[6] = sun.z;
            row[7] = w.x; row[8] = w.y; row[9] = w.z;
            row[10] = escapes ? 1.0f : 0.0f; row[11] = in_cone ? 1.0f : 0.0f;
            row[12] = value.x; row[13] = value.y; row[14] = value.z; row[15] = 0.0f;
        }
    }
    return 0;
}

}  // extern "C"
