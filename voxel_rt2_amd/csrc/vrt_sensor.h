// vrt_sensor.h -- vrt_gather_irradiance: how much light falls on caller-supplied surface points.  Which sensors are traced at all, one
// (sensor, sample) item -- its directions, its sun term, its hemisphere path -- and the ordered sums over a sensor's samples.  Plain
// functions over plain values, in the style of vrt_cast.h / vrt_radiance.h: k_gather_irradiance (vrt_query_kernels.hip) keeps one item per lane
// and steps it with sensor_begin / sensor_sun / sensor_segment / sensor_value between refills, k_fold_query<SensorQuery> (vrt_query.h) is a loop over
// sensor_fold, and tests/emul/sensor_emul.cpp runs the same functions on a machine without a GPU (tests/test_sensor_host.py).
//
// Sample s of a sensor (frame f = first_frame + s), in binary32:
//   1. g = dm_rng_init(seed, f, stream, 4): the sensor's own random stream (4: sensor directions).  o = pos + normal * 1e-6 per
//      component, a product then a sum (pathtracer.py:428).
//   2. sun (pathtracer.py:436-468 without the BSDF and the MIS weight): ldir = sample_cone_oriented(light_cos_theta_max, light_direction)
//      on g's first two draws, ndl = dot(ldir, normal).  If ndl > 0 the shadow ray next_hit(o, ldir, inf, shadow) is cast -- whatever the
//      sun's colour: `sun` is a visibility -- and if it returns >= inf, vis_s = 1 and
//          sun_s = ((T * light_weight) * light_color) * ndl           T = the sky's transmittance along ldir under use_physical_sky, else 1
//      which is path_shade's `nd = w * bd * sky_t * light_weight * light_color * ndl` (vrt_path.h), evaluated left to right, with w and
//      bd removed.  Else vis_s = 0 and sun_s = 0.  No firefly clamp: nothing is multiplied by a BSDF here.
//   3. hemisphere: w = sample_cosine_weighted_hemisphere(normal) on g's next two draws.  The ray (o, w, stream) is path-traced as
//      vrt_trace_radiance traces it at frame f -- radiance_begin / radiance_segment / radiance_value of vrt_radiance.h, a fresh path on
//      stream (seed, f, stream, 0); nothing of the shading is restated here -- with ONE difference: a path whose first segment escapes
//      does not see the sun's disc (path_shade's DISC0 = false), because step 2 has counted the sun.  sky_s = 1 for such a path, else 0.
//      hemi_s = L_s * 3.14159274f per component (the cosine-weighted density is cos / pi).
//   4. four running sums over s in order -- sky_rgb += hemi_s, sky += sky_s, sun_rgb += sun_s, sun += vis_s -- each divided by
//      (float)n_samples at the end (sensor_fold, sensor_mean).
// The normal is assumed unit.  Where it is so far from unit that (o, w) is not a ray vrt_trace_radiance would trace (radiance_ray_valid:
// o overflows, or the hemisphere vector's squared length does and norm3 returns zeros or NaN), nothing is walked and the sample's four
// terms are zero: every walk a gather starts passes the gate of a query's.
#pragma once
#include "../../include/vrt_api.h"
#include "vrt_radiance.h"

namespace vrt {

#define VRT_SENSOR_PI 3.14159274f

// The sensors that are traced: every component finite, a normal that is not all zeros (+0 or -0), `reserved` 0 (refused on the host
// path; where the library cannot look -- device memory -- such a sensor counts as invalid).  A sample of a valid sensor costs at most one shadow
// walk and one path of at most max_depth segments, and only where its derived ray passes the radiance query's gate (sensor_begin): each
// of them a walk that ends (vrt_cast.h), whatever the sensor's components are.
VRT_DEV bool sensor_valid(const vrt_sensor& s) {
    for (int a = 0; a < 3; a++) if (!cast_finite(s.pos[a]) || !cast_finite(s.normal[a])) return false;
    return !(s.normal[0] == 0.0f && s.normal[1] == 0.0f && s.normal[2] == 0.0f) && s.reserved == 0u;
}

// Steps 1, 2 up to the shadow ray, and the hemisphere draw: all four draws of g, in order.  Leaves the sun sample in (ldir, ndl) for
// sensor_sun and a fresh path at o along w in p (p.pos is o).  The shadow ray draws nothing, so it may be walked later (sensor_sun):
// the kernel walks the shadow rays of several items together.  Returns false, with p untouched, where (o, w) is not a ray of the radiance
// query's (radiance_ray_valid): the item is then all zeros and neither ray is walked.
VRT_DEV bool sensor_begin(const FrameParams& fp, Path<false>& p, const vrt_sensor& s, uint32_t frame, f3& ldir, float& ndl) {
    dm_rng g = dm_rng_init(fp.seed, frame, s.stream, 4u);
    const f3 n = mk3(s.normal[0], s.normal[1], s.normal[2]);
    const f3 o = mk3(s.pos[0], s.pos[1], s.pos[2]) + n * VRT_EPS;
    f3 lx, ly;
    ortho_basis(fp.light_dir, lx, ly);
    ldir = cone_dir(fp.light_cos_max, fp.light_dir, lx, ly, g);
    ndl = dot3(ldir, n);
    const f3 w = cosine_dir(n, g);
    vrt_path_ray r;
    r.origin[0] = o.x; r.origin[1] = o.y; r.origin[2] = o.z;
    r.dir[0] = w.x; r.dir[1] = w.y; r.dir[2] = w.z;
    r.stream = s.stream;
    r.reserved = 0u;
    if (!radiance_ray_valid(r)) return false;
    radiance_begin(fp, p, r, frame);
    return true;
}
// Step 2's shadow ray and the sun term, from o = the path's origin: sun_s, and vis_s in `vis`.
template <class PyrT>
VRT_DEV f3 sensor_sun(const FrameParams& fp, const SceneData& sc, const PyrT& P, f3 o, f3 ldir, float ndl, TraceStats& ts, float& vis) {
    vis = 0.0f;
    f3 sun = mk3(0.0f);
    if (ndl > 0.0f) {
        Hit sh;
        next_hit<true>(fp, sc, P, o, ldir, sh, ts);
        if (sh.closest >= DM_INF) {
            vis = 1.0f;
            f3 sky_t = mk3(1.0f);
            if (fp.use_sky == 1) sky_t = sky_transmittance(sc.sky, ldir);
            sun = sky_t * fp.light_weight * fp.light_color * ndl;
        }
    }
    return sun;
}
// One segment of the hemisphere path.  Returns true when the path is over.  At the path's first segment `sky` becomes sky_s: 1 if the
// segment escapes (nothing nearer than inf: path_shade's own test), else 0.
template <class PyrT>
VRT_DEV bool sensor_segment(const FrameParams& fp, const SceneData& sc, const PyrT& P, Path<false>& p, TraceStats& ts, float& sky) {
    const bool first = p.depth == 0;
    float t = 0.0f;
    const bool done = radiance_segment<false>(fp, sc, P, p, ts, t);
    if (first) sky = (t == DM_INF) ? 1.0f : 0.0f;
    return done;
}
// hemi_s of a finished path
VRT_DEV f3 sensor_value(const Path<false>& p) { return radiance_value(p) * VRT_SENSOR_PI; }

VRT_DEV vrt_irradiance sensor_zero() {
    vrt_irradiance v;
    for (int a = 0; a < 3; a++) { v.sky_rgb[a] = 0.0f; v.sun_rgb[a] = 0.0f; }
    v.sky = 0.0f; v.sun = 0.0f;
    return v;
}
// One item from start to end, as a record of its four terms.  The sensor is valid (sensor_valid: the caller's gate).
template <class PyrT>
VRT_DEV vrt_irradiance sensor_item(const FrameParams& fp, const SceneData& sc, const PyrT& P, const vrt_sensor& s, int sample, uint32_t first_frame) {
    Path<false> p;
    f3 ldir;
    float ndl, vis, sky = 0.0f;
    TraceStats ts;
    stats_zero(ts);
    if (!sensor_begin(fp, p, s, first_frame + (uint32_t)sample, ldir, ndl)) return sensor_zero();
    const f3 sun = sensor_sun(fp, sc, P, p.pos, ldir, ndl, ts, vis);
    while (!sensor_segment(fp, sc, P, p, ts, sky)) {}
    const f3 hemi = sensor_value(p);
    vrt_irradiance v;
    v.sky_rgb[0] = hemi.x; v.sky_rgb[1] = hemi.y; v.sky_rgb[2] = hemi.z; v.sky = sky;
    v.sun_rgb[0] = sun.x; v.sun_rgb[1] = sun.y; v.sun_rgb[2] = sun.z; v.sun = vis;
    return v;
}
// The reduction over a sensor's samples, in binary32 and in sample order, as radiance_fold / radiance_mean: four running sums, each
// sum = 0; sum += term_s for s = 0 .. n_samples - 1; sum / n_samples.  A chunk of `count` consecutive samples continues the sums the chunk
// before it left (`acc`; zero before the first), so how the samples are cut into chunks cannot change a bit.  values[s * stride]: the
// chunk's records of this sensor (the scratch plane holds a sample's sensors side by side).
VRT_DEV vrt_irradiance sensor_fold(vrt_irradiance acc, const vrt_irradiance* values, long long stride, int count) {
    for (int s = 0; s < count; s++) {
        const vrt_irradiance v = values[(long long)s * stride];
        for (int a = 0; a < 3; a++) acc.sky_rgb[a] = acc.sky_rgb[a] + v.sky_rgb[a];
        acc.sky = acc.sky + v.sky;
        for (int a = 0; a < 3; a++) acc.sun_rgb[a] = acc.sun_rgb[a] + v.sun_rgb[a];
        acc.sun = acc.sun + v.sun;
    }
    return acc;
}
VRT_DEV vrt_irradiance sensor_mean(vrt_irradiance sum, int n_samples) {
    const float n = (float)n_samples;
    for (int a = 0; a < 3; a++) { sum.sky_rgb[a] = sum.sky_rgb[a] / n; sum.sun_rgb[a] = sum.sun_rgb[a] / n; }
    sum.sky = sum.sky / n;
    sum.sun = sum.sun / n;
    return sum;
}

}  // namespace vrt
