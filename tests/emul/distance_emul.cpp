// distance_emul.cpp -- TEST TOOLING: the loops of the k_dist_* kernels (voxel_rt2_amd/csrc/vrt_scene_kernels.hip) and of vrt_distance_field
// (vrt_scene_ops.hip) run on the host over the functions of voxel_rt2_amd/csrc/vrt_distance.h: the same checks, the same grown box, the same
// scratch layout (plan_distance_layout), pass z line by line, passes y and x tile by tile with the lanes and groups of a workgroup one
// after the other, each staging its lines in a local array the way the kernels stage them in LDS.  tests/distance.py compiles this with
// g++ and calls it through ctypes.
// -DDISTANCE_EMUL_MAIN: a stand-alone program (its own main, no Python) over small generated grids, checked against a brute force --
// what a sanitizer build runs.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/vrt_api.h"
#include "../../voxel_rt2_amd/csrc/vrt_distance.h"
#include "../../voxel_rt2_amd/csrc/vrt_plan.h"

using namespace vrt;

template <bool NEAR>
static void passes(int G, const DistBox& p, const int8_t* mat, int* A, int* B, uint8_t* cz, uint8_t* cy, int* d2, int* nearest) {
    const int gxn = dist_len(p.grown, 0), gyn = dist_len(p.grown, 1), gzn = dist_len(p.grown, 2);
    const int bxn = dist_len(p.box, 0), byn = dist_len(p.box, 1), bzn = dist_len(p.box, 2);
    std::vector<int> f((size_t)VRT_DIST_LINE * VRT_DIST_LANES);
    // k_dist_z
    for (int L = 0; L < gxn * gyn; L++) {
        const int x = p.grown.lo[0] + L / gyn, y = p.grown.lo[1] + L % gyn;
        for (int k = 0; k < gzn; k++) f[(size_t)k] = dist_seed(mat[edit_grid_index(G, x, y, p.grown.lo[2] + k)], p);
        for (int zi = 0; zi < bzn; zi++) {
            const DistPick b = dist_line_element<NEAR>(f.data(), 1, gzn, p.box.lo[2] - p.grown.lo[2] + zi, p.grown.lo[2]);
            const size_t o = (size_t)L * bzn + zi;
            A[o] = b.v;
            if (NEAR) cz[o] = (uint8_t)b.c;
        }
    }
    // k_dist_y
    for (int xi = 0; xi < gxn; xi++)
        for (int z0 = 0; z0 < bzn; z0 += VRT_DIST_LANES) {
            for (int j = 0; j < gyn; j++)
                for (int lane = 0; lane < VRT_DIST_LANES; lane++) f[(size_t)j * VRT_DIST_LANES + lane] = z0 + lane < bzn ? A[dist_a_index(p, xi, j, z0 + lane)] : p.cap;
            for (int lane = 0; lane < VRT_DIST_LANES && z0 + lane < bzn; lane++)
                for (int yo = 0; yo < byn; yo++) {
                    const DistPick b = dist_line_element<NEAR>(f.data() + lane, VRT_DIST_LANES, gyn, p.box.lo[1] - p.grown.lo[1] + yo, p.grown.lo[1]);
                    const size_t o = dist_b_index(p, xi, yo, z0 + lane);
                    B[o] = b.v;
                    if (NEAR) cy[o] = (uint8_t)b.c;
                }
        }
    // k_dist_x
    const int plane = byn * bzn;
    for (int p0 = 0; p0 < plane; p0 += VRT_DIST_LANES) {
        for (int j = 0; j < gxn; j++)
            for (int lane = 0; lane < VRT_DIST_LANES; lane++) f[(size_t)j * VRT_DIST_LANES + lane] = p0 + lane < plane ? B[(size_t)j * plane + p0 + lane] : p.cap;
        for (int lane = 0; lane < VRT_DIST_LANES && p0 + lane < plane; lane++) {
            const int pi = p0 + lane, yo = pi / bzn, zi = pi - yo * bzn;
            for (int xo = 0; xo < bxn; xo++) {
                const DistPick b = dist_line_element<NEAR>(f.data() + lane, VRT_DIST_LANES, gxn, p.box.lo[0] - p.grown.lo[0] + xo, p.grown.lo[0]);
                const size_t o = (size_t)xo * plane + pi;
                const int v = dist_final(b.v, p.max_d2);
                d2[o] = v;
                if (NEAR) nearest[o] = v == VRT_DIST_FAR_VALUE ? -1 : dist_assemble(p, G, b.c, yo, zi, cy, cz);
            }
        }
    }
}

static DistLayout layout_of(const DistBox& p, bool nearest) {
    return plan_distance_layout((size_t)dist_len(p.grown, 0), (size_t)dist_len(p.grown, 1), (size_t)dist_len(p.box, 0), (size_t)dist_len(p.box, 1),
                                (size_t)dist_len(p.box, 2), nearest, false);
}

extern "C" {
// plan_distance_layout's byte count for this call (the device path's: results are written to the caller's arrays); -1: a bad call
long long distance_emul_plan(int G, const int* lo, const int* hi, int max_d2, unsigned flags, int nearest) {
    EditBox box;
    for (int a = 0; a < 3; a++) { box.lo[a] = lo[a]; box.hi[a] = hi[a]; }
    if (!edit_box_valid(box, G) || max_d2 < 0 || max_d2 > VRT_DIST_MAX_D2) return -1;
    return (long long)layout_of(dist_plan_box(box, G, max_d2, flags), nearest != 0).bytes;
}
// the grown box of a call: out[0..2] = lo, out[3..5] = hi
void distance_emul_grown(int G, const int* lo, const int* hi, int max_d2, int* out) {
    EditBox box;
    for (int a = 0; a < 3; a++) { box.lo[a] = lo[a]; box.hi[a] = hi[a]; }
    const DistBox p = dist_plan_box(box, G, max_d2, 0u);
    for (int a = 0; a < 3; a++) { out[a] = p.grown.lo[a]; out[3 + a] = p.grown.hi[a]; }
}
// vrt_distance_field on host arrays: mat int8[G][G][G]; scratch: at least distance_emul_plan bytes.  Returns vrt_distance_field's code.
int distance_emul_call(int G, const int8_t* mat, const int* lo, const int* hi, int max_d2, unsigned flags, int* d2, int* nearest, uint8_t* scratch) {
    if (!mat || !lo || !hi || !d2) return VRT_E_INVALID;
    EditBox box;
    for (int a = 0; a < 3; a++) { box.lo[a] = lo[a]; box.hi[a] = hi[a]; }
    if (!edit_box_valid(box, G)) return VRT_E_INVALID;
    if (max_d2 < 0 || max_d2 > VRT_DIST_MAX_D2) return VRT_E_INVALID;
    if ((flags & ~(unsigned)VRT_DIST_TO_EMPTY) != 0u) return VRT_E_INVALID;
    if (edit_box_voxels(box) == 0) return VRT_OK;
    const DistBox p = dist_plan_box(box, G, max_d2, flags);
    const DistLayout l = layout_of(p, nearest != nullptr);
    int* A = (int*)(scratch + l.a_at);
    int* B = (int*)(scratch + l.b_at);
    if (nearest) passes<true>(G, p, mat, A, B, scratch + l.cz_at, scratch + l.cy_at, d2, nearest);
    else passes<false>(G, p, mat, A, B, nullptr, nullptr, d2, nullptr);
    return VRT_OK;
}
}

#ifdef DISTANCE_EMUL_MAIN
// every cell of the box against every target: (d2, linear index) minimised
static int check(int G, const std::vector<int8_t>& mat, const int* lo, const int* hi, int max_d2, unsigned flags, const char* name) {
    const size_t nv = (size_t)(hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]);
    std::vector<int> d2(nv, 12345), nearest(nv, 12345), d2_only(nv, 12345);
    const long long bytes = distance_emul_plan(G, lo, hi, max_d2, flags, 1);
    std::vector<uint8_t> scratch((size_t)bytes);   // exactly the planned size: the sanitizer sees a byte too far
    if (distance_emul_call(G, mat.data(), lo, hi, max_d2, flags, d2.data(), nearest.data(), scratch.data()) != VRT_OK) return 1;
    std::vector<uint8_t> scratch2((size_t)distance_emul_plan(G, lo, hi, max_d2, flags, 0));
    if (distance_emul_call(G, mat.data(), lo, hi, max_d2, flags, d2_only.data(), nullptr, scratch2.data()) != VRT_OK) return 1;
    std::vector<int> targets;
    for (int i = 0; i < G * G * G; i++) if ((mat[(size_t)i] > 0) != ((flags & 1u) != 0u)) targets.push_back(i);
    size_t o = 0;
    int bad = 0;
    for (int x = lo[0]; x < hi[0]; x++)
        for (int y = lo[1]; y < hi[1]; y++)
            for (int z = lo[2]; z < hi[2]; z++, o++) {
                int best = VRT_DIST_FAR, who = -1;
                for (int t : targets) {
                    const int tx = t / (G * G), ty = t / G % G, tz = t % G;
                    const int d = (x - tx) * (x - tx) + (y - ty) * (y - ty) + (z - tz) * (z - tz);
                    if (d <= max_d2 && d < best) { best = d; who = t; }   // (targets ascend: the first of equals is the smallest index)
                }
                if (d2[o] != best || nearest[o] != who || d2_only[o] != best) bad++;
            }
    printf("%s: %zu cells, %zu targets, %d wrong\n", name, nv, targets.size(), bad);
    return bad != 0;
}
int main(int argc, char** argv) {   // distance_emul_asan [sparse | dense | ties]: one family, or all three
    const int G = 20;
    const char* family = argc > 1 ? argv[1] : "all";
    const auto want = [&](const char* name) { return !strcmp(family, "all") || !strcmp(family, name); };
    int fails = 0;
    unsigned s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    if (want("sparse")) {   // sparse: a few solids, the box cut by the grid on one side, every max_d2 regime
        std::vector<int8_t> mat((size_t)G * G * G, 0);
        for (int k = 0; k < 9; k++) mat[rnd() % mat.size()] = (int8_t)(k % 2 ? 5 : -3 + 8 * (k % 3));
        const int lo[3] = {0, 3, 7}, hi[3] = {9, 20, 12};
        fails += check(G, mat, lo, hi, 0, 0u, "sparse max_d2=0");
        fails += check(G, mat, lo, hi, 17, 0u, "sparse max_d2=17");
        fails += check(G, mat, lo, hi, VRT_DIST_MAX_D2, 0u, "sparse unbounded");
    }
    if (want("dense")) {   // dense: half the cells, both flag values, a one-cell box and a line
        std::vector<int8_t> mat((size_t)G * G * G, 0);
        for (auto& m : mat) m = (int8_t)(rnd() % 2 ? 1 + rnd() % 100 : -(int)(rnd() % 2));
        const int lo[3] = {5, 0, 19}, hi[3] = {6, 20, 20};
        fails += check(G, mat, lo, hi, 9, 0u, "dense line");
        fails += check(G, mat, lo, hi, 9, VRT_DIST_TO_EMPTY, "dense line to_empty");
        const int lo1[3] = {19, 19, 0}, hi1[3] = {20, 20, 1};
        fails += check(G, mat, lo1, hi1, 3, VRT_DIST_TO_EMPTY, "dense cell to_empty");
    }
    if (want("ties")) {   // ties: twelve targets at d2 = 25 around one cell, and an empty grid
        std::vector<int8_t> mat((size_t)G * G * G, 0);
        const int c[3] = {10, 10, 10}, off[6][3] = {{5, 0, 0}, {0, 5, 0}, {0, 0, 5}, {3, 4, 0}, {0, 3, 4}, {4, 0, 3}};
        for (auto& o : off)
            for (int sg = -1; sg <= 1; sg += 2) mat[(size_t)(((c[0] + sg * o[0]) * G + c[1] + sg * o[1]) * G + c[2] + sg * o[2])] = 1;
        const int lo[3] = {6, 6, 6}, hi[3] = {15, 14, 13};
        fails += check(G, mat, lo, hi, 25, 0u, "ties max_d2=25");
        fails += check(G, mat, lo, hi, 24, 0u, "ties max_d2=24");
        std::vector<int8_t> none((size_t)G * G * G, 0);
        fails += check(G, none, lo, hi, 100, 0u, "empty");
    }
    printf(fails ? "FAILED\n" : "ok\n");
    return fails != 0;
}
#endif
