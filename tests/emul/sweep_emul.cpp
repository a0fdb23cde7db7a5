// sweep_emul.cpp -- TEST TOOLING: the loop of k_sweep_boxes (voxel_rt2_amd/csrc/vrt_query_kernels.hip) run on the host over the functions of
// voxel_rt2_amd/csrc/vrt_sweep.h, box by box: the lanes of a box one after the other, merged with the same order function the kernel's
// butterfly uses, on pyramid levels the test hands over (tests/edit.py builds them in numpy); the candidate region, the validity gate
// and the plain decisions of vrt_sweep_boxes (vrt_plan.h).  tests/sweep.py compiles this with g++ and calls it through ctypes.
// -DSWEEP_EMUL_MAIN: a stand-alone program (its own main, no Python) that runs the row function over one family of boxes on a small
// scene built here -- what a sanitizer build runs.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../voxel_rt2_amd/csrc/vrt_sweep.h"
#include "../../voxel_rt2_amd/csrc/vrt_plan.h"

using namespace vrt;

struct SweepScene {   // what tests/sweep.py fills (ctypes mirror there)
    int32_t grid_res, pad;
    float floor_height, pad2;
    float cull[8];   // voxel units: lo xyz, hi xyz (k_cull_box's, or the open one)
    const unsigned long long *l0, *l1;
};

// one box: k_sweep_boxes' body with `lanes` lanes run in turn
static void row(const SweepScene& s, const vrt_box_sweep& b, int lanes, bool prune, vrt_sweep_hit& out) {
    bool walk;
    SweepKey best = sweep_begin(b, s.floor_height, walk);
    if (walk) {
        const SweepRegion r = sweep_region(b, s.grid_res, s.cull);
        if (!r.empty) {
            const SweepKey start = best;
            for (int lane = 0; lane < lanes; lane++) best = sweep_better(best, sweep_lane(b, r, s.grid_res, s.l0, s.l1, start, lane, lanes, prune));
        }
    }
    sweep_record(best, b, s.grid_res, out);
}

extern "C" {

int sweep_emul_boxes(const SweepScene* s, int lanes, int prune, long long n, const vrt_box_sweep* boxes, vrt_sweep_hit* hits) {
    if (!s || n < 0 || lanes < 1 || lanes > 64 || (s->grid_res != 128 && s->grid_res != 256)) return -1;
    for (long long i = 0; i < n; i++) row(*s, boxes[i], lanes, prune != 0, hits[i]);
    return 0;
}
// region[7] per box: lo xyz, hi xyz (cells, both ends included), empty; an invalid box reports an empty region
int sweep_emul_regions(const SweepScene* s, long long n, const vrt_box_sweep* boxes, int32_t* region) {
    if (!s || n < 0 || (s->grid_res != 128 && s->grid_res != 256)) return -1;
    for (long long i = 0; i < n; i++) {
        int32_t* o = region + 7 * i;
        if (!sweep_box_valid(boxes[i])) { for (int a = 0; a < 3; a++) { o[a] = 0; o[3 + a] = -1; } o[6] = 1; continue; }
        const SweepRegion r = sweep_region(boxes[i], s->grid_res, s->cull);
        for (int a = 0; a < 3; a++) { o[a] = r.lo[a]; o[3 + a] = r.hi[a]; }
        o[6] = r.empty ? 1 : 0;
    }
    return 0;
}
int sweep_emul_valid(const vrt_box_sweep* b) { return sweep_box_valid(*b) ? 1 : 0; }
long long sweep_emul_chunk(void) { return plan_sweep_chunk(); }
int sweep_emul_blocks(long long n, int n_cu, int per_cu) { return plan_sweep_blocks(n, n_cu, per_cu); }
int sweep_emul_sizes(int which) { return which == 0 ? (int)sizeof(vrt_box_sweep) : (int)sizeof(vrt_sweep_hit); }

}  // extern "C"

#if defined(SWEEP_EMUL_MAIN)
// A 128^3 grid with a few blocks over a floor, levels built the way k_build_l0 / k_build_coarse build them, the open culling box; boxes
// from a small generator -- falling, sliding, resting on faces, overlapping, degenerate, huge and subnormal moves, the invalid classes --
// through the row function with 1 and 64 lanes, pruning on and off: the four must agree.
int main() {
    const int G = 128, n0 = G / 4, n1 = G / 16;
    std::vector<unsigned long long> l0((size_t)n0 * n0 * n0, 0), l1((size_t)n1 * n1 * n1, 0);
    auto put = [&](int x, int y, int z) { l0[((size_t)(z >> 2) * n0 + (y >> 2)) * n0 + (x >> 2)] |= 1ULL << (((z & 3) << 4) | ((y & 3) << 2) | (x & 3)); };
    for (int bx = 40; bx < 90; bx += 9) for (int bz = 40; bz < 90; bz += 9)
        for (int x = bx; x < bx + 6; x++) for (int z = bz; z < bz + 6; z++) for (int y = 54; y < 57 + (bx + bz) % 8; y++) put(x, y, z);
    put(0, 0, 0); put(127, 127, 127);
    for (int b = 0; b < n0 * n0 * n0; b++)
        if (l0[b]) { const int x = b % n0, y = (b / n0) % n0, z = b / (n0 * n0); l1[((size_t)(z >> 2) * n1 + (y >> 2)) * n1 + (x >> 2)] |= 1ULL << (((z & 3) << 4) | ((y & 3) << 2) | (x & 3)); }
    SweepScene s;
    memset(&s, 0, sizeof(s));
    s.grid_res = G; s.floor_height = -0.16f;
    for (int a = 0; a < 3; a++) { s.cull[a] = -1e30f; s.cull[3 + a] = 1e30f; }
    s.l0 = l0.data(); s.l1 = l1.data();
    uint32_t rng = 12345u;
    auto u = [&]() { rng = rng * 747796405u + 2891336453u; return (float)((rng >> 8) & 0xffffu) / 65536.0f; };
    std::vector<vrt_box_sweep> boxes;
    const float specials[] = {0.0f, -0.0f, 1e-40f, -1e30f, 1e30f, DM_INF, -DM_INF, DM_NAN, 64.0f, -64.0f, 65.0f};
    for (int i = 0; i < 4000; i++) {
        vrt_box_sweep b;
        memset(&b, 0, sizeof(b));
        for (int a = 0; a < 3; a++) {
            const float c = u() * 2.4f - 1.2f, h = (i % 7 == 0) ? 0.0f : u() * 0.1f;
            b.lo[a] = (i % 3 == 0) ? (float)(int)(c * 64.0f) / 64.0f : c;
            b.hi[a] = b.lo[a] + ((i % 3 == 0) ? (float)(int)(h * 64.0f) / 64.0f : h);
            b.move[a] = (i % 5 == 0) ? (float)((int)(u() * 5.0f) - 2) * 0.25f : u() * 2.0f - 1.0f;
        }
        b.t_max = (i % 4 == 0) ? DM_INF : u() * 2.0f + 0.01f;
        b.flags = (uint32_t)(i & 1);
        if (i % 11 == 0) {   // a special value in one of the float fields (words 3 and 7 of the record are the integer fields)
            float f[12];
            memcpy(f, &b, sizeof(b));
            const int k = (i / 11) % 12;
            f[k == 3 || k == 7 ? 0 : k] = specials[(i / 7) % 11];
            memcpy(&b, f, sizeof(b));
        }
        if (i == 1) { for (int a = 0; a < 3; a++) { b.lo[a] = -1.0f; b.hi[a] = 1.0f; b.move[a] = 0.0f; } }   // the whole grid
        boxes.push_back(b);
    }
    const size_t n = boxes.size();
    std::vector<vrt_sweep_hit> a(n), c(n);
    sweep_emul_boxes(&s, 64, 1, (long long)n, boxes.data(), a.data());
    int kinds[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < n; i++) kinds[a[i].kind & 3]++;
    for (int lanes = 1; lanes <= 64; lanes += 63)
        for (int prune = 0; prune < 2; prune++) {
            sweep_emul_boxes(&s, lanes, prune, (long long)n, boxes.data(), c.data());
            if (memcmp(a.data(), c.data(), n * sizeof(vrt_sweep_hit)) != 0) { printf("FAIL lanes=%d prune=%d\n", lanes, prune); return 1; }
        }
    printf("ok: %zu boxes, miss %d floor %d voxel %d start %d\n", n, kinds[0], kinds[1], kinds[2], kinds[3]);
    return (kinds[0] && kinds[1] && kinds[2] && kinds[3]) ? 0 : 2;
}
#endif
