// vrt_radiance.h -- vrt_trace_radiance: path-traced radiance along caller-supplied rays.  Which rays are traced at all, one
// (ray, sample) item from its first segment to its value, and the ordered sum over a ray's samples.  Plain functions over plain values,
// in the style of vrt_cast.h: k_trace_radiance (vrt_query_kernels.hip) keeps one item per lane and steps it with radiance_begin /
// radiance_segment / radiance_value between refills, k_fold_query<RadianceQuery> (vrt_query.h) is a loop over radiance_fold, and tests/emul/radiance_emul.cpp
// runs the same functions on a machine without a GPU (tests/test_radiance_host.py).
//
// An item is one run of the reference's render body (pathtracer.py:355-632) with ReSTIR off and a static camera, started at the
// caller's origin along the caller's direction on random stream (seed, first_frame + sample, ray.stream, 0): Path<false> and path_segment
// of vrt_path.h, which is what the render kernels run -- nothing of the shading is restated here.  It stores no pixel value
// (path_segment<false, STORE = false>) and counts nothing.
#pragma once
#include "../../include/vrt_api.h"
#include "vrt_path.h"
#include "vrt_temporal.h"
#include "vrt_cast.h"

namespace vrt {

// The rays that are traced: cast_ray_valid's gate (vrt_cast.h) without its t_max clause; a ray whose `reserved` is not 0 is refused on
// the host path and counts as invalid where the library cannot look (device memory).  Every segment of a path is a walk that ends
// (see there) and a path has at most max_depth segments, so a valid ray costs a bounded number of steps whatever its components are.
VRT_DEV bool radiance_ray_valid(const vrt_path_ray& r) {
    for (int a = 0; a < 3; a++) if (!cast_finite(r.origin[a]) || !cast_finite(r.dir[a])) return false;
    return !(r.dir[0] == 0.0f && r.dir[1] == 0.0f && r.dir[2] == 0.0f) && r.reserved == 0u;
}

// A fresh path for sample `frame - first_frame` of the ray (frame = first_frame + sample, modulo 2^32 as the reference's counter).
VRT_DEV void radiance_begin(const FrameParams& fp, Path<false>& p, const vrt_path_ray& r, uint32_t frame) {
    p.pix_u = 0;
    p.pix_v = 0;
    p.sample = 0;
    path_start(p, mk3(r.origin[0], r.origin[1], r.origin[2]), mk3(r.dir[0], r.dir[1], r.dir[2]), dm_rng_init(fp.seed, frame, r.stream, 0u));
}
// One segment: path_segment (vrt_path.h) without its stores.  Returns true when the path is over.  t_first: at the path's first segment,
// the distance of that hit -- vrt_cast_rays' t for t_max = inf (the same next_hit on the same ray), +inf into the sky.  A query counts
// nothing: the caller's `ts` is a sink.  DISC0: path_shade's (false: vrt_sensor.h's paths).
template <bool DISC0 = true, class PyrT>
VRT_DEV bool radiance_segment(const FrameParams& fp, const SceneData& sc, const PyrT& P, Path<false>& p, TraceStats& ts, float& t_first) {
    const bool first = p.depth == 0;
    float closest;
    const bool done = path_segment<false, false, DISC0>(fp, sc, P, PixelBuffers{}, 0, p, ts, closest);   // (the buffers are never read: STORE = false)
    if (first) t_first = closest;
    return done;
}
// The value of a finished path: diffuse + specular as path_finish forms them for a static camera (no demodulation), each replaced by
// zero where the temporal prepass would scrub it (scrub, vrt_temporal.h: a NaN, infinite or negative component).
VRT_DEV f3 radiance_value(const Path<false>& p) {
    f3 diffuse = mk3(0.0f), specular = mk3(0.0f);
    path_colours(p, diffuse, specular);
    return scrub(diffuse) + scrub(specular);
}
// One item from start to end.  The ray is valid (radiance_ray_valid: the caller's gate).
template <class PyrT>
VRT_DEV f3 radiance_item(const FrameParams& fp, const SceneData& sc, const PyrT& P, const vrt_path_ray& r, int sample, uint32_t first_frame,
                         float& t) {
    Path<false> p;
    radiance_begin(fp, p, r, first_frame + (uint32_t)sample);
    t = DM_INF;
    TraceStats ts;
    stats_zero(ts);
    while (!radiance_segment(fp, sc, P, p, ts, t)) {}
    return radiance_value(p);
}

// The reduction over a ray's samples, in binary32 and in sample order: sum = 0; sum += value_s for s = 0 .. n_samples - 1; sum / n_samples.
// A chunk of `count` consecutive samples continues the sum the chunk before it left (`acc`; zero before the first), so how the samples
// are cut into chunks cannot change a bit.  values[s * stride]: the chunk's values of this ray (the scratch plane holds a sample's rays
// side by side).
VRT_DEV f3 radiance_fold(f3 acc, const f3* values, long long stride, int count) {
    for (int s = 0; s < count; s++) acc = acc + values[(long long)s * stride];
    return acc;
}
VRT_DEV f3 radiance_mean(f3 sum, int n_samples) { return sum / (float)n_samples; }

}  // namespace vrt
