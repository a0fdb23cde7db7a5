// vrt_probe_sh.h -- vrt_gather_probes: the light at caller-supplied points in empty space as spherical-harmonic coefficients, the sun
// kept apart.  Which probes are walked at all, one (probe, sample) item -- its sun sample, its sphere direction, its path -- the basis,
// and the ordered sums over a probe's samples.  Plain functions over plain values, in the style of vrt_sensor.h: k_gather_probes
// (vrt_query_kernels.hip) keeps one item per lane and steps it with probe_begin / probe_sun / probe_segment / probe_value between refills,
// k_fold_query<ProbeQuery> (vrt_query.h) is a loop over probe_fold, and tests/emul/probe_emul.cpp runs the same functions on a machine
// without a GPU (tests/test_probe_host.py).  (vrt_probe.h is the ray probe of the walk tests: another thing.)
//
// Sample s of a probe (frame f = first_frame + s), in binary32:
//   1. g = dm_rng_init(seed, f, stream, 5): the probe's own random stream (5: probe directions).
//   2. sun: ldir = cone_dir(light_cos_max, light_dir, basis) on g's first two draws, exactly as sensor_begin draws it.  The shadow ray
//      next_hit<shadow>(pos, ldir, inf) is ALWAYS cast -- no normal, no ndl test -- and if it returns >= inf, vis_s = 1 and
//          sun_s = (T * light_weight) * light_color          T = the sky's transmittance along ldir under use_physical_sky, else 1
//      (sensor_sun's product without its ndl: the sun's irradiance on a surface that faces it).  Else both are 0.
//   3. sphere: on g's next two draws u0, u1: a = 1 - 2 u0, b = sqrt(1 - a a), w = norm3((b cos, b sin, a)) of 2 pi u1 -- cosine_dir's lines
//      without the normal and without the 1e-5 shrink.  The ray (pos, w, stream) -- the origin is pos itself -- is path-traced as
//      vrt_gather_irradiance's step 3 traces its ray at frame f: radiance_begin / sensor_segment / radiance_value, DISC0 = false, sky_s = 1
//      where the first segment escapes.  Nothing of the shading is restated here.
//   4. the item keeps L_s, sky_s, w, vis_s, sun_s (ProbeItem: 12 floats); the FOLD evaluates the basis at w and the 27 products
//      (L_s * 12.5663706f) * Yi in sample order (probe_fold), so the scratch plane holds 48 bytes an item and not 128.
//   5. thirty-two running sums, each divided by (float)n_samples at the end (probe_mean).
// The basis is the real spherical harmonics of bands 0 to 2 with Z AS THE POLAR AXIS; the world's up is y (include/vrt_api.h).
#pragma once
#include "../../include/vrt_api.h"
#include "vrt_sensor.h"

namespace vrt {

#define VRT_PROBE_4PI 12.5663706f

// One (probe, sample) item in the scratch plane.
struct ProbeItem {
    float L[3];      // L_s
    float sky;       // sky_s
    float w[3];      // the sphere direction
    float vis;       // vis_s
    float sun[3];    // sun_s
    float pad;       // 0
};

// The probes that are walked: every pos component finite.  A sample of a valid probe costs one shadow walk and one path of at most
// max_depth segments: each a walk that ends (vrt_cast.h), wherever the probe lies -- inside a solid voxel, below the floor, outside the
// grid's box: none of these is special-cased.
VRT_DEV bool probe_valid(const vrt_probe& q) { return cast_finite(q.pos[0]) && cast_finite(q.pos[1]) && cast_finite(q.pos[2]); }

// Step 3's direction: uniform on the sphere, from two draws of g.
VRT_DEV f3 probe_sphere_dir(dm_rng& g) {
    const float u0 = dm_rng_f32(&g), u1 = dm_rng_f32(&g);
    const float a = 1.0f - 2.0f * u0;
    const float b = dm_sqrt(1.0f - a * a);
    float sn, cs;
    dm_sincos(DM_TWO_PI * u1, &sn, &cs);
    return norm3(mk3(b * cs, b * sn, a));
}
// Steps 1, 2 up to the shadow ray, and the sphere draw: all four draws of g, in order.  Leaves the sun sample in ldir for probe_sun, the
// direction in w and a fresh path at pos along w in p.  The shadow ray draws nothing, so it may be walked later (probe_sun): the kernel
// walks the shadow rays of several items together.  Returns false, with p untouched, where (pos, w) is not a ray of the radiance
// query's (radiance_ray_valid; for a finite pos it always is): the item is then all zeros and neither ray is walked.
VRT_DEV bool probe_begin(const FrameParams& fp, Path<false>& p, const vrt_probe& q, uint32_t frame, f3& ldir, f3& w) {
    dm_rng g = dm_rng_init(fp.seed, frame, q.stream, 5u);
    f3 lx, ly;
    ortho_basis(fp.light_dir, lx, ly);
    ldir = cone_dir(fp.light_cos_max, fp.light_dir, lx, ly, g);
    w = probe_sphere_dir(g);
    vrt_path_ray r;
    r.origin[0] = q.pos[0]; r.origin[1] = q.pos[1]; r.origin[2] = q.pos[2];
    r.dir[0] = w.x; r.dir[1] = w.y; r.dir[2] = w.z;
    r.stream = q.stream;
    r.reserved = 0u;
    if (!radiance_ray_valid(r)) return false;
    radiance_begin(fp, p, r, frame);
    return true;
}
// Step 2's shadow ray and the sun term, from o = the path's origin: sun_s, and vis_s in `vis`.
template <class PyrT>
VRT_DEV f3 probe_sun(const FrameParams& fp, const SceneData& sc, const PyrT& P, f3 o, f3 ldir, TraceStats& ts, float& vis) {
    vis = 0.0f;
    f3 sun = mk3(0.0f);
    Hit sh;
    next_hit<true>(fp, sc, P, o, ldir, sh, ts);
    if (sh.closest >= DM_INF) {
        vis = 1.0f;
        f3 sky_t = mk3(1.0f);
        if (fp.use_sky == 1) sky_t = sky_transmittance(sc.sky, ldir);
        sun = sky_t * fp.light_weight * fp.light_color;
    }
    return sun;
}
// One segment of the path, sky_s at its first: sensor_segment's escape rule, unchanged.
template <class PyrT>
VRT_DEV bool probe_segment(const FrameParams& fp, const SceneData& sc, const PyrT& P, Path<false>& p, TraceStats& ts, float& sky) {
    return sensor_segment(fp, sc, P, p, ts, sky);
}
// L_s of a finished path
VRT_DEV f3 probe_value(const Path<false>& p) { return radiance_value(p); }

VRT_DEV ProbeItem probe_item_zero() {
    ProbeItem v;
    for (int a = 0; a < 3; a++) { v.L[a] = 0.0f; v.w[a] = 0.0f; v.sun[a] = 0.0f; }
    v.sky = 0.0f; v.vis = 0.0f; v.pad = 0.0f;
    return v;
}
VRT_DEV vrt_sh_probe probe_zero() {
    vrt_sh_probe v;
    for (int i = 0; i < 9; i++) for (int a = 0; a < 3; a++) v.sh[i][a] = 0.0f;
    for (int a = 0; a < 3; a++) v.sun_rgb[a] = 0.0f;
    v.sky = 0.0f; v.sun = 0.0f;
    return v;
}
// One item from start to end.  The probe is valid (probe_valid: the caller's gate).
template <class PyrT>
VRT_DEV ProbeItem probe_item(const FrameParams& fp, const SceneData& sc, const PyrT& P, const vrt_probe& q, int sample, uint32_t first_frame) {
    Path<false> p;
    f3 ldir, w;
    float vis, sky = 0.0f;
    TraceStats ts;
    stats_zero(ts);
    if (!probe_begin(fp, p, q, first_frame + (uint32_t)sample, ldir, w)) return probe_item_zero();
    const f3 sun = probe_sun(fp, sc, P, p.pos, ldir, ts, vis);
    while (!probe_segment(fp, sc, P, p, ts, sky)) {}
    const f3 L = probe_value(p);
    ProbeItem v;
    v.L[0] = L.x; v.L[1] = L.y; v.L[2] = L.z; v.sky = sky;
    v.w[0] = w.x; v.w[1] = w.y; v.w[2] = w.z; v.vis = vis;
    v.sun[0] = sun.x; v.sun[1] = sun.y; v.sun[2] = sun.z; v.pad = 0.0f;
    return v;
}

// The basis at (x, y, z): real spherical harmonics of bands 0 to 2, z the polar axis, (l, m) = (0,0), (1,-1), (1,0), (1,1), (2,-2) .. (2,2);
// each line left to right.
VRT_DEV void probe_basis(float x, float y, float z, float (&Y)[9]) {
    Y[0] = 0.282094792f;
    Y[1] = 0.488602512f * y;
    Y[2] = 0.488602512f * z;
    Y[3] = 0.488602512f * x;
    Y[4] = 1.09254843f * (x * y);
    Y[5] = 1.09254843f * (y * z);
    Y[6] = 0.315391565f * (3.0f * (z * z) - 1.0f);
    Y[7] = 1.09254843f * (x * z);
    Y[8] = 0.546274215f * (x * x - y * y);
}
// The reduction over a probe's samples, in binary32 and in sample order, as sensor_fold / sensor_mean: thirty-two running sums.  Per
// sample the basis at the item's w and the 27 products Lw[ch] * Yi, Lw = L_s * 4 pi, are formed HERE.  A chunk of `count` consecutive
// samples continues the sums the chunk before it left (`acc`; zero before the first), so how the samples are cut into chunks cannot
// change a bit.  values[s * stride]: the chunk's items of this probe (the scratch plane holds a sample's probes side by side).
VRT_DEV vrt_sh_probe probe_fold(vrt_sh_probe acc, const ProbeItem* values, long long stride, int count) {
    for (int s = 0; s < count; s++) {
        const ProbeItem v = values[(long long)s * stride];
        float Y[9];
        probe_basis(v.w[0], v.w[1], v.w[2], Y);
        float Lw[3];
        for (int a = 0; a < 3; a++) Lw[a] = v.L[a] * VRT_PROBE_4PI;
        for (int i = 0; i < 9; i++) for (int a = 0; a < 3; a++) acc.sh[i][a] = acc.sh[i][a] + Lw[a] * Y[i];
        acc.sky = acc.sky + v.sky;
        for (int a = 0; a < 3; a++) acc.sun_rgb[a] = acc.sun_rgb[a] + v.sun[a];
        acc.sun = acc.sun + v.vis;
    }
    return acc;
}
VRT_DEV vrt_sh_probe probe_mean(vrt_sh_probe sum, int n_samples) {
    const float n = (float)n_samples;
    for (int i = 0; i < 9; i++) for (int a = 0; a < 3; a++) sum.sh[i][a] = sum.sh[i][a] / n;
    for (int a = 0; a < 3; a++) sum.sun_rgb[a] = sum.sun_rgb[a] / n;
    sum.sky = sum.sky / n;
    sum.sun = sum.sun / n;
    return sum;
}

}  // namespace vrt
