// cast_emul.cpp -- TEST TOOLING: the loop of k_cast_rays (voxel_rt2_amd/csrc/vrt_query_kernels.hip) run on the host over cast_row of
// voxel_rt2_amd/csrc/vrt_cast.h, ray by ray, on a pyramid and texel grid the test hands over (tests/edit.py builds them in numpy);
// the loop of k_fetch_voxels; and the plain decisions of vrt_cast_rays (vrt_plan.h).  The views of the pyramid and the scene record's
// conversion are tests/emul/query_emul.h's.  tests/cast.py compiles this with g++ and calls it through ctypes.
#include "query_emul.h"

struct CastScene {   // what tests/cast.py fills (ctypes mirror there)
    int32_t grid_res, ref_oob, floor_material, pad;
    float floor_height, floor_color[3], voxel_edges;
    float cull[8];   // the box cast_row's walk tests rays against (k_cull_box's, or the open one)
    const uint32_t* grid;
    const unsigned long long *l0, *l1, *l2, *l3;
};

// mode 0: the ray's own flag picks cast_row<true> / cast_row<false> (a wave of like rays); 1: cast_row<false> for every ray and the
// surface fields dropped on flagged rays (a wave of mixed rays)
template <class PyrT>
static void rows(const FrameParams& fp, const SceneData& sc, const PyrT& P, int mode, long long n, const vrt_ray* rays, vrt_ray_hit* hits) {
    for (long long i = 0; i < n; i++) {
        const bool any = (rays[i].flags & VRT_RAY_ANY_HIT) != 0u;
        if (any && mode == 0) cast_row<true>(fp, sc, P, rays[i], hits[i]);
        else { cast_row<false>(fp, sc, P, rays[i], hits[i]); if (any) cast_strip_surface(hits[i]); }
    }
}
extern "C" {

int cast_emul_rays(const CastScene* s, int staged, int mode, long long n, const vrt_ray* rays, vrt_ray_hit* hits) {
    if (!s || n < 0 || (s->grid_res != 128 && s->grid_res != 256)) return -1;
    FrameParams fp;
    SceneData sc;
    scene_common(*s, fp, sc);
    auto run = [&](const auto& P) { rows(fp, sc, P, mode, n, rays, hits); };
    if (s->grid_res == 256) with_view<256>(sc, staged, run);
    else with_view<128>(sc, staged, run);
    return 0;
}
int cast_emul_valid(const vrt_ray* r) { return cast_ray_valid(*r) ? 1 : 0; }
int cast_emul_staged(long long n, int knob) { return plan_cast_staged(n, knob) ? 1 : 0; }
long long cast_emul_chunk(void) { return plan_cast_chunk(); }
int cast_emul_blocks(long long n, int n_cu, int per_cu) { return plan_cast_blocks(n, n_cu, per_cu); }
// the loop of k_fetch_voxels; -1: not a box of a grid of G^3 voxels (vrt_fetch_voxels' check, which is vrt_update_voxels')
int cast_emul_fetch(int G, const int* lo, const int* hi, const int8_t* mat, const uint8_t* rgb, int8_t* box_mat, uint8_t* box_rgb) {
    EditBox box;
    for (int a = 0; a < 3; a++) { box.lo[a] = lo[a]; box.hi[a] = hi[a]; }
    if ((G != 128 && G != 256) || !edit_box_valid(box, G)) return -1;
    for (int i = 0; i < edit_box_voxels(box); i++) fetch_box_voxel(box, G, i, mat, rgb, box_mat, box_rgb);
    return 0;
}

// the mode of the frame parameters every later call hands the device functions (query_emul.h): 0 plain, 1 poisoned; returns the mode before
int cast_emul_poison(int on) { const int was = g_query_poison; g_query_poison = on ? 1 : 0; return was; }
// frame_params_probe on the record a call on scene `s` would hand over in the current mode: float out[8], int32 ints[4]
void cast_emul_probe(const CastScene* s, float* out, int32_t* ints) {
    FrameParams fp;
    SceneData sc;
    scene_common(*s, fp, sc);
    frame_params_probe(fp, out, ints);
}

}  // extern "C"
