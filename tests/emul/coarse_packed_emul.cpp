// coarse_packed_emul.cpp -- TEST TOOLING: descend_flat() (voxel_rt2_amd/csrc/vrt_trace.h) on a host pyramid type that declares the packed
// coarse entry, as the pooled render kernels' staged 128^3 view does (LdsPyramid2<128>, vrt_kernels.hip), against the branchy descend() on
// GlobalPyramid; and coarse_pack() against the expressions it folds.  The table of entries is filled by the loop of render_pool_body's
// staging, index by index.  tests/test_coarse_packed_host.py compiles this with g++ and calls it through ctypes.
#include <vector>
#include "../../voxel_rt2_amd/csrc/vrt_types.h"
#include "../../voxel_rt2_amd/csrc/vrt_trace.h"

using namespace vrt;

namespace {

struct Entry { unsigned long long w1; uint32_t packed; };

struct PackedHostPyramid {  // what LdsPyramid2<128> hands descend_flat(): {l1 word, coarse_pack()} per l1 cell, fine words by rank
    static constexpr int G = 128;
    static constexpr bool flat_descend = true;
    static constexpr bool cull = true;
    static constexpr bool coarse_packed = true;
    const Entry* l1p;
    const unsigned long long* l0c;
    mutable long long fine_loads = 0;
    unsigned long long load_l3() const { return 0ULL; }
    unsigned long long load_fine(int key, uint32_t idx) const { (void)key; fine_loads++; return l0c[idx]; }
    void load_coarse(int i1, int i2, unsigned long long& w1, unsigned long long& w2, uint32_t& packed) const {
        (void)i2;
        w1 = l1p[i1].w1;
        w2 = 0xdeadbeefdeadbeefULL;   // a packed type hands out no l2 word: whatever stands here must not matter
        packed = l1p[i1].packed;
    }
};
static_assert(coarse_packed_of<PackedHostPyramid>::value && !coarse_packed_of<GlobalPyramid<128>>::value, "the trait");

std::vector<Entry> stage(const unsigned long long* l1, const unsigned long long* l2, const uint32_t* l0c_base) {
    std::vector<Entry> t(512);
    for (int i = 0; i < 512; i++) {
        const unsigned long long w2 = l2[(((i >> 8) & 1) << 2) | (((i >> 5) & 1) << 1) | ((i >> 2) & 1)];
        t[i].w1 = l1[i];
        t[i].packed = coarse_pack(w2, i & 7, (i >> 3) & 7, i >> 6, l0c_base[i]);
    }
    return t;
}

GlobalPyramid<128> global_view(const unsigned long long* l0, const unsigned long long* l1, const unsigned long long* l2, const unsigned long long* l0c,
                               const uint32_t* l0c_base) {
    GlobalPyramid<128> P;
    P.p = Pyramid{};
    P.p.l0 = l0; P.p.l1 = l1; P.p.l2 = l2; P.p.l0c = l0c; P.p.l0c_base = l0c_base; P.p.l0c_count = l0c_base + 512;
    return P;
}

}  // namespace

extern "C" {

// Every cell of the 128^3 grid, every start level 0..6: descend_flat on the packed type (its brick cache carried from cell to cell, as a
// walk carries it) against descend() on GlobalPyramid (a fresh cache per query).  Returns the number of queries whose level, solid or nq
// differ; first[0..9] = x, y, z, start, then level, solid, nq of either side for the first of them.  *fine_loads: how many fine words the
// packed side asked for (so that a comparison of grids with solids cannot pass without reading one).
long long cp_compare_descents(const unsigned long long* l0, const unsigned long long* l1, const unsigned long long* l2, const unsigned long long* l0c,
                              const uint32_t* l0c_base, int* first, long long* fine_loads) {
    const GlobalPyramid<128> R = global_view(l0, l1, l2, l0c, l0c_base);
    const std::vector<Entry> table = stage(l1, l2, l0c_base);
    PackedHostPyramid P;
    P.l1p = table.data(); P.l0c = l0c;
    long long bad = 0;
    BrickCache bc;
    bc.key = -1; bc.word = 0ULL;
    for (int z = 0; z < 128; z++) for (int y = 0; y < 128; y++) for (int x = 0; x < 128; x++) {
        CoarseWords c;
        coarse_fetch(P, x, y, z, c);
        for (int start = 0; start <= 6; start++) {
            bool solid = false, rsolid = false;
            int nq = 0, rnq = 0;
            const int level = descend_flat(P, c, x, y, z, start, solid, bc, nq);
            BrickCache rbc;
            rbc.key = -1; rbc.word = 0ULL;
            const int rlevel = descend(R, x, y, z, start, rsolid, rbc, rnq);
            if (level != rlevel || solid != rsolid || nq != rnq) {
                if (bad == 0) {
                    const int v[10] = {x, y, z, start, level, (int)solid, nq, rlevel, (int)rsolid, rnq};
                    for (int k = 0; k < 10; k++) first[k] = v[k];
                }
                bad++;
            }
        }
    }
    *fine_loads = P.fine_loads;
    return bad;
}

// coarse_pack() of all 512 l1 cells against what it folds, each written out from the levels: the fine base, and levels 4, 5 and 6 both as
// descend_flat()'s unpacked expressions and as cell_occupied() reads them.  Returns the number of cells that differ (first: its index).
int cp_check_pack(const unsigned long long* l0, const unsigned long long* l1, const unsigned long long* l2, const unsigned long long* l0c,
                  const uint32_t* l0c_base, int* first) {
    const GlobalPyramid<128> R = global_view(l0, l1, l2, l0c, l0c_base);
    const std::vector<Entry> table = stage(l1, l2, l0c_base);
    int bad = 0;
    for (int i = 0; i < 512; i++) {
        const int x4 = i & 7, y4 = (i >> 3) & 7, z4 = i >> 6;
        const unsigned long long w2 = l2[((z4 >> 2) << 1 | (y4 >> 2)) << 1 | (x4 >> 2)];
        const unsigned flat = (w2 != 0ULL ? 4u : 0u) | brick_two_lods(w2, x4, y4, z4);
        const unsigned cells = (cell_occupied(R, 6, x4 >> 2, y4 >> 2, z4 >> 2) ? 4u : 0u) | (cell_occupied(R, 5, x4 >> 1, y4 >> 1, z4 >> 1) ? 2u : 0u) |
                               (cell_occupied(R, 4, x4, y4, z4) ? 1u : 0u);
        const uint32_t e = table[i].packed;
        const bool ok = table[i].w1 == l1[i] && coarse_packed_base(e) == l0c_base[i] && coarse_packed_occ456(e) == flat && coarse_packed_levels(e) == flat << 4 && flat == cells &&
                        e == (l0c_base[i] | (flat << 29));
        if (!ok) { if (bad == 0) *first = i; bad++; }
    }
    return bad;
}

}  // extern "C"
