// cast_emul.cpp -- TEST TOOLING: the loop of k_cast_rays (voxel_rt2_amd/csrc/vrt_kernels.hip) run on the host over cast_row of
// voxel_rt2_amd/csrc/vrt_cast.h, ray by ray, on a pyramid and texel grid the test hands over (tests/edit.py builds them in numpy);
// the loop of k_fetch_voxels; and the plain decisions of vrt_cast_rays (vrt_plan.h).  tests/cast.py compiles this with g++ and calls
// it through ctypes.
#include <cstring>
#include "../../voxel_rt2_amd/csrc/vrt_cast.h"
#include "../../voxel_rt2_amd/csrc/vrt_plan.h"

using namespace vrt;

// The staged view of the kernel (LdsPyramid, vrt_kernels.hip: device only) restated for the host: the same members and reads, the coarse
// levels in copies of their own where the kernel has them in LDS.  OOB as there: whether the type carries the reference's reading
// of cells outside the grid.
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
template <int G>
static void cast_g(const CastScene& s, int staged, int mode, long long n, const vrt_ray* rays, vrt_ray_hit* hits) {
    FrameParams fp;
    memset(&fp, 0, sizeof(fp));
    fp.floor_height = s.floor_height;
    fp.floor_color = mk3(s.floor_color[0], s.floor_color[1], s.floor_color[2]);
    fp.floor_material = s.floor_material;
    fp.voxel_edges = s.voxel_edges;
    SceneData sc;
    memset(&sc, 0, sizeof(sc));
    sc.pyr.l0 = s.l0; sc.pyr.l1 = s.l1; sc.pyr.l2 = s.l2; sc.pyr.l3 = s.l3;
    sc.pyr.ref_oob = s.ref_oob;
    sc.grid = s.grid;
    sc.cull = s.cull;
    if (!staged) {
        GlobalPyramid<G> P;
        P.p = sc.pyr;
        rows(fp, sc, P, mode, n, rays, hits);
        return;
    }
    auto stage = [&](auto& P) {
        P.l0 = s.l0;
        memcpy(P.l1, s.l1, sizeof(P.l1));
        memcpy(P.l2, s.l2, sizeof(P.l2));
        P.w3 = G == 256 ? s.l3[0] : 0ULL;
        P.oob = s.ref_oob != 0;
        rows(fp, sc, P, mode, n, rays, hits);
    };
    if (s.ref_oob) { static StagedPyramid<G, true> P; stage(P); }
    else { static StagedPyramid<G, false> P; stage(P); }
}

extern "C" {

int cast_emul_rays(const CastScene* s, int staged, int mode, long long n, const vrt_ray* rays, vrt_ray_hit* hits) {
    if (!s || n < 0 || (s->grid_res != 128 && s->grid_res != 256)) return -1;
    if (s->grid_res == 256) cast_g<256>(*s, staged, mode, n, rays, hits);
    else cast_g<128>(*s, staged, mode, n, rays, hits);
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

}  // extern "C"
