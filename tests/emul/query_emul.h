// query_emul.h -- TEST TOOLING: what the host builds of the three scene queries share (cast_emul.cpp, radiance_emul.cpp, sensor_emul.cpp).
// The staged view of the pyramid, the scene record the tests fill and its conversion to what the device functions read, the choice of
// view, the block loop of a sampled query -- driven the way vrt_scene_ops.hip (sampled_query) and the kernels of vrt_query_kernels.hip drive it,
// through the same traits (voxel_rt2_amd/csrc/vrt_query.h) -- and the small scene of the stand-alone programs.
#pragma once
#include <cstring>
#include <vector>
#include "../../voxel_rt2_amd/csrc/vrt_query.h"

using namespace vrt;

// The staged view of the kernels (LdsPyramid, vrt_views.h: device only) restated for the host: the same members and reads, the coarse
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
// fn(P) on the view a launch would walk on: everything through the pointers of sc.pyr, or the coarse levels staged (stage_query).
template <int G, class Fn>
static void with_view(const SceneData& sc, int staged, Fn fn) {
    if (!staged) {
        GlobalPyramid<G> P;
        P.p = sc.pyr;
        fn(P);
        return;
    }
    auto stage = [&](auto& P) {
        P.l0 = sc.pyr.l0;
        memcpy(P.l1, sc.pyr.l1, sizeof(P.l1));
        memcpy(P.l2, sc.pyr.l2, sizeof(P.l2));
        P.w3 = G == 256 ? sc.pyr.l3[0] : 0ULL;
        P.oob = sc.pyr.ref_oob != 0;
        fn(P);
    };
    if (sc.pyr.ref_oob) { static StagedPyramid<G, true> P; stage(P); }
    else { static StagedPyramid<G, false> P; stage(P); }
}

// The frame parameters a query is handed have two modes.  Plain (0): every field a query is not meant to read is zero.  Poisoned (1,
// query_emul_poison): every such field holds a hostile value -- every 32-bit word of the record a quiet NaN's bits (so a field added to
// FrameParams later is poisoned by default), the integer fields the largest int or -1, `frame` all ones, camera_is_moving the value the
// plain mode does not hold.  A query's answer must not tell the modes apart (tests/test_*_host.py: the same bytes).
static int g_query_poison = 0;
static void frame_params_base(FrameParams& fp) {
    memset(&fp, 0, sizeof(fp));
    if (!g_query_poison) return;
    static_assert(sizeof(FrameParams) % 4 == 0, "FrameParams is a record of 32-bit fields");
    const uint32_t qnan = 0x7fc00000u;
    for (size_t k = 0; k < sizeof(fp); k += 4) memcpy((char*)&fp + k, &qnan, 4);
    fp.W = fp.H = 0x7fffffff;
    fp.row0 = -1; fp.row1 = 0x7fffffff;
    fp.stripe_rows = -1; fp.stripe_period = 0x7fffffff; fp.stripe_first = -1; fp.stripe_tile_rows = 0x7fffffff;
    fp.frame = 0xffffffffu;
    fp.camera_is_moving = 1;   // (plain: 0; scene_sampled takes the other value in either mode)
}

// What every query reads of a scene record (CastScene of cast_emul.cpp, RadScene) -- of the frame parameters the floor (height, colour,
// material) and voxel_edges, as query_inputs (vrt_scene_ops.hip) lists them; of the scene the pyramid, the texels, the culling box.
template <class Scene>
static void scene_common(const Scene& s, FrameParams& fp, SceneData& sc) {
    frame_params_base(fp);
    fp.floor_height = s.floor_height;
    fp.floor_color = mk3(s.floor_color[0], s.floor_color[1], s.floor_color[2]);
    fp.floor_material = s.floor_material;
    fp.voxel_edges = s.voxel_edges;
    memset(&sc, 0, sizeof(sc));
    sc.pyr.l0 = s.l0; sc.pyr.l1 = s.l1; sc.pyr.l2 = s.l2; sc.pyr.l3 = s.l3;
    sc.pyr.ref_oob = s.ref_oob;
    sc.grid = s.grid;
    sc.cull = s.cull;
}
// The liveness check of the poisoned mode: functions that DO read fields no query reads, on the record `fp` -- camera_ray_dir(3, 2)
// (the matrices, inv_res, render_scale, the jitter) into out[0..2], pixel_texcoord(3, 2) into out[3..4]; launch_tile_rows (row0, row1,
// the stripe fields) into tile_rows; and the three plain integers.
static void frame_params_probe(const FrameParams& fp, float* out, int32_t* ints) {
    const f3 d = camera_ray_dir(fp, 3, 2);
    const f2 tc = pixel_texcoord(fp, 3.0f, 2.0f);
    out[0] = d.x; out[1] = d.y; out[2] = d.z; out[3] = tc.x; out[4] = tc.y;
    out[5] = fp.exposure; out[6] = fp.max_accum_frames; out[7] = fp.camera_pos.y;
    ints[0] = launch_tile_rows(fp); ints[1] = fp.W; ints[2] = (int32_t)fp.frame; ints[3] = fp.camera_is_moving;
}
struct RadScene {   // what tests/radiance.py fills (ctypes mirror there); tests/sensor.py fills the same record
    int32_t grid_res, ref_oob, floor_material, use_sky, max_depth, sky_res;
    uint32_t seed;
    int32_t pad;
    float floor_height, floor_color[3], voxel_edges, background[3], light_dir[3], light_color[3], light_cos_max, light_weight;
    float cull[8];   // the box the walks test rays against (k_cull_box's, or the open one)
    const uint32_t* grid;
    const unsigned long long *l0, *l1, *l2, *l3;
    const float *mats, *sky_scat, *sky_trans;
};
// ... and what a sampled query reads on top: the background, the light (direction, colour, cone, weight), the sky switch, max_depth and
// the seed; the materials and the sky tables.
static void scene_sampled(const RadScene& s, FrameParams& fp, SceneData& sc) {
    scene_common(s, fp, sc);
    fp.background = mk3(s.background[0], s.background[1], s.background[2]);
    fp.light_dir = mk3(s.light_dir[0], s.light_dir[1], s.light_dir[2]);
    fp.light_color = mk3(s.light_color[0], s.light_color[1], s.light_color[2]);
    fp.light_cos_max = s.light_cos_max;
    fp.light_weight = s.light_weight;
    fp.use_sky = s.use_sky;
    fp.max_depth = s.max_depth;
    fp.seed = s.seed;
    fp.camera_is_moving = g_query_poison ? 0 : 1;   // (ignored by a query: were it read, the demodulation would show)
    sc.mats = s.mats;
    sc.sky.scattering = s.sky_scat; sc.sky.transmittance = s.sky_trans;
    sc.sky.res = s.sky_res; sc.sky.fres = s.sky_res > 0 ? (float)(1.0 / (double)s.sky_res) : 0.0f;
}

// A sampled query's chunk loop over one block of n records (sampled_query, vrt_scene_ops.hip), the item kernels' numbering and k_fold_query's
// fold.  per: whole samples a chunk (0: plan_query_chunk's).  item(in, sample, out): the value of one (record, sample) item -- zero for
// an invalid record -- and whatever the item kernel writes to the output record directly.
template <class Q, class ItemFn>
static void query_block(long long n, const typename Q::In* in, int n_samples, int per, typename Q::Out* out, ItemFn item) {
    if (per < 1) per = plan_query_chunk(Q::max_items, n, n_samples);
    std::vector<typename Q::Item> plane((size_t)n * per);
    for (int s0 = 0; s0 < n_samples; s0 += per) {
        const int count = per < n_samples - s0 ? per : n_samples - s0;
        for (long long i = 0; i < n * count; i++) plane[i] = item(in[i % n], s0 + (int)(i / n), out[i % n]);
        for (long long k = 0; k < n; k++) query_fold<Q>(out[k], plane.data() + k, n, count, s0 == 0, s0 + count == n_samples, n_samples);
    }
}
// The whole of a sampled query's emulation for a scene record: its conversion, the view, the block.  item(fp, sc, P, in, sample, out).
template <class Q, class ItemFn>
static int query_run(const RadScene* s, int staged, long long n, const typename Q::In* in, int n_samples, int per, typename Q::Out* out, ItemFn item) {
    if (!s || n < 0 || n_samples < 1 || (s->grid_res != 128 && s->grid_res != 256)) return -1;
    if (n == 0) return 0;
    FrameParams fp;
    SceneData sc;
    scene_sampled(*s, fp, sc);
    auto run = [&](const auto& P) {
        query_block<Q>(n, in, n_samples, per, out, [&](const typename Q::In& r, int sample, typename Q::Out& o) { return item(fp, sc, P, r, sample, o); });
    };
    if (s->grid_res == 256) with_view<256>(sc, staged, run);
    else with_view<128>(sc, staged, run);
    return 0;
}

// The scene of the stand-alone programs (-DRADIANCE_EMUL_MAIN, -DSENSOR_EMUL_MAIN): a 128^3 grid with a few blocks on a floor, and with
// `roof` a slab over some of them, built the way k_pack_grid / k_build_l0 / k_build_coarse build it; a sun, a plain sky, the open
// culling box.
struct SmallScene {
    static constexpr int G = 128, n0 = G / 4;
    std::vector<int8_t> mat;
    std::vector<uint32_t> grid;
    std::vector<unsigned long long> l0, l1, l2, l3;
    std::vector<float> mats;
    RadScene s;
    void put(int x, int y, int z, int m) {
        mat[((size_t)x * G + y) * G + z] = (int8_t)m;
        grid[texel_index<G>(x, y, z)] = 200u | (120u << 8) | (60u << 16) | ((uint32_t)m << 24);
    }
    static void coarse(const std::vector<unsigned long long>& fine, std::vector<unsigned long long>& out, int nc) {
        const int nf = nc * 4;
        for (int b = 0; b < nc * nc * nc; b++) {
            const int bx = b % nc, by = (b / nc) % nc, bz = b / (nc * nc);
            for (int z = 0; z < 4; z++) for (int y = 0; y < 4; y++) for (int x = 0; x < 4; x++)
                if (fine[((bz * 4 + z) * nf + (by * 4 + y)) * nf + (bx * 4 + x)] != 0) out[b] |= 1ULL << (z * 16 + y * 4 + x);
        }
    }
    SmallScene(bool roof, int max_depth)
        : mat((size_t)G * G * G, 0), grid((size_t)G * G * G, 0u), l0((size_t)n0 * n0 * n0, 0), l1(512, 0), l2(8, 0), l3(1, 0), mats(128 * 14, 0.0f) {
        for (int bx = 40; bx < 90; bx += 9) for (int bz = 40; bz < 90; bz += 9)
            for (int x = bx; x < bx + 6; x++) for (int z = bz; z < bz + 6; z++) for (int y = 54; y < 57 + (bx + bz) % 8; y++)
                put(x, y, z, ((bx + bz) % 5 == 0) ? 2 : 1 + (bx % 3));
        if (roof) for (int x = 40; x < 60; x++) for (int z = 40; z < 60; z++) put(x, 70, z, 1);
        for (int b = 0; b < n0 * n0 * n0; b++) {
            const int bx = b % n0, by = (b / n0) % n0, bz = b / (n0 * n0);
            for (int z = 0; z < 4; z++) for (int y = 0; y < 4; y++) for (int x = 0; x < 4; x++)
                if (mat[((size_t)(bx * 4 + x) * G + (by * 4 + y)) * G + (bz * 4 + z)] > 0) l0[b] |= 1ULL << (z * 16 + y * 4 + x);
        }
        coarse(l0, l1, G / 16);
        coarse(l1, l2, G / 64);
        for (int id = 0; id < 128; id++) { float* p = &mats[14 * id]; p[0] = p[1] = p[2] = 1.0f; p[5] = 0.5f; p[7] = 0.3f + 0.2f * (id % 3); p[4] = id == 3 ? 0.8f : 0.0f; p[12] = 1.0f; p[13] = 0.5f; }
        memset(&s, 0, sizeof(s));
        s.grid_res = G; s.floor_material = 1; s.max_depth = max_depth; s.seed = 11u;
        s.floor_height = -0.16f; s.floor_color[0] = 0.7f; s.floor_color[1] = 0.6f; s.floor_color[2] = 0.5f; s.voxel_edges = 0.06f;
        s.background[0] = 0.2f; s.background[1] = 0.3f; s.background[2] = 0.5f;
        s.light_dir[0] = 0.2873479f; s.light_dir[1] = 0.9578263f; s.light_dir[2] = 0.0f; s.light_color[0] = 1.0f; s.light_color[1] = 0.9f; s.light_color[2] = 0.8f;
        s.light_cos_max = 0.995f; s.light_weight = 3.0f;
        for (int a = 0; a < 3; a++) { s.cull[a] = -1e30f; s.cull[3 + a] = 1e30f; }
        s.grid = grid.data(); s.l0 = l0.data(); s.l1 = l1.data(); s.l2 = l2.data(); s.l3 = l3.data(); s.mats = mats.data();
    }
};
