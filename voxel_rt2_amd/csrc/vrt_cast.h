// vrt_cast.h -- vrt_cast_rays: caller-supplied rays against the prepared scene.  Which rays are walked at all, the record a ray
// gets, and one ray's whole body (cast_row).  Plain functions over plain values, in the style of vrt_edit.h / vrt_plan.h: k_cast_rays
// (vrt_query_kernels.hip) is a grid-stride loop over cast_row, one ray per lane, and tests/emul/cast_emul.cpp runs the same function on a
// machine without a GPU (tests/test_cast_rays_host.py).
//
// A query is the reference's next_hit (pathtracer.py:218-244; next_hit in vrt_trace.h): floor plane, then the hierarchical DDA, then
// -- unless the ray is an any-hit ray, the reference's shadow ray -- the surface lookup.  It reads scene data only.
#pragma once
#include "../../include/vrt_api.h"
#include "vrt_trace.h"
#include "vrt_edit.h"

namespace vrt {

VRT_DEV bool cast_finite(float x) { return (dm_f2u(x) & 0x7f800000u) != 0x7f800000u; }   // neither inf nor NaN

// The rays that are walked.  Invalid (include/vrt_api.h): a non-finite origin or direction component, a direction of all zeros
// (+0 or -0), t_max NaN or <= 0.  Every other ray ends: the walk's loop is `while (iters < 512)` (raytrace, vrt_trace.h) and a step
// of it holds no loop but the descent, which goes down one level per turn (descend_outside: at most GridDim::lods turns), so a valid
// ray costs at most 512 steps whatever its components are -- subnormal, 1e20, on a cell boundary.  No class of finite input has to
// be added to the invalid set.
VRT_DEV bool cast_ray_valid(const vrt_ray& r) {
    for (int a = 0; a < 3; a++) if (!cast_finite(r.origin[a]) || !cast_finite(r.dir[a])) return false;
    if (r.dir[0] == 0.0f && r.dir[1] == 0.0f && r.dir[2] == 0.0f) return false;
    return r.t_max > 0.0f;   // (false for a NaN)
}

// nothing nearer than t_max
VRT_DEV void cast_miss(vrt_ray_hit& h) {
    h.t = DM_INF;
    h.kind = VRT_HIT_MISS;
    for (int a = 0; a < 3; a++) { h.cell[a] = -1; h.normal[a] = 0.0f; h.albedo[a] = 0.0f; }
    h.mat_id = 0;
}
// what an any-hit ray does not report: no surface lookup was made for it (or its result is dropped: k_cast_rays, a wave of mixed rays)
VRT_DEV void cast_strip_surface(vrt_ray_hit& h) {
    for (int a = 0; a < 3; a++) { h.normal[a] = 0.0f; h.albedo[a] = 0.0f; }
    h.mat_id = 0;
}

// One ray: the validity gate, next_hit<ANY_HIT, PyrT>, the record.
// t_max: the reference's next_hit starts from closest = max_dist and both of its tests are `t < closest`, the floor's first.  Here the
// walk runs with max_dist = inf and the result is kept if t < t_max.  That is the same record: a floor hit at f and a voxel hit at v
// (inf: none) are accepted by the reference iff f < t_max, and v < min(t_max, f if accepted); with inf the result is the floor iff
// f <= v, else the voxel, and the smaller of the two is below t_max iff the reference accepted it -- a floor at f >= t_max that the
// reference skipped cannot hide a voxel at v < t_max, since then v < f and the voxel wins here too.
// Culling stays on (sc.cull is the scene's box): a ray cull_ray() reports clear of every solid voxel is a miss for the voxel test
// either way, and at 128^3 the part of a walk behind the grown box can only end a miss (vrt_trace.h: "rays that cannot hit anything").
template <bool ANY_HIT, class PyrT>
VRT_DEV void cast_row(const FrameParams& fp, const SceneData& sc, const PyrT& P, const vrt_ray& r, vrt_ray_hit& out) {
    cast_miss(out);
    if (!cast_ray_valid(r)) return;
    const f3 pos = mk3(r.origin[0], r.origin[1], r.origin[2]), d = mk3(r.dir[0], r.dir[1], r.dir[2]);
    Hit h;
    TraceOut tr;
    TraceStats ts;
    stats_zero(ts);
    next_hit<ANY_HIT>(fp, sc, P, pos, d, h, ts, tr);
    if (!(h.closest < r.t_max)) return;
    // which of the two tests left `closest`: the voxel's runs second and is strict, so a tie is the floor's
    const bool voxel = tr.dist * GridDim<PyrT::G>::voxel_size < floor_probe(fp, pos, d);
    out.t = h.closest;
    out.kind = voxel ? VRT_HIT_VOXEL : VRT_HIT_FLOOR;
    if (voxel) { out.cell[0] = tr.ix; out.cell[1] = tr.iy; out.cell[2] = tr.iz; }
    if (!ANY_HIT) {
        out.normal[0] = h.normal.x; out.normal[1] = h.normal.y; out.normal[2] = h.normal.z;
        out.albedo[0] = h.albedo.x; out.albedo[1] = h.albedo.y; out.albedo[2] = h.albedo.z;
        out.mat_id = h.mat_id;
    }
}

// vrt_fetch_voxels: voxel `i` of the box arrays (edit_box_voxel's order) read back from the grid's stored materials and colours --
// edit_store_voxel the other way round.
VRT_DEV void fetch_box_voxel(const EditBox& b, int G, int i, const int8_t* mat, const uint8_t* rgb, int8_t* box_mat, uint8_t* box_rgb) {
    int x, y, z;
    edit_box_voxel(b, i, x, y, z);
    const int g = edit_grid_index(G, x, y, z);
    box_mat[i] = mat[g];
    for (int k = 0; k < 3; k++) box_rgb[3 * i + k] = rgb[3 * g + k];
}

}  // namespace vrt
