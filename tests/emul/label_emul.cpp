// label_emul.cpp -- TEST TOOLING: the loops of the k_label_* kernels (voxel_rt2_amd/csrc/vrt_scene_kernels.hip) and of vrt_label_components
// (vrt_scene_ops.hip) run on the host over the functions of voxel_rt2_amd/csrc/vrt_label.h: the same checks, the same tiles, the same
// scratch layout (plan_label_layout), phase by phase -- every tile solved in a local array the way the kernel solves it in LDS, then the
// seams, then the finish in place.  What the device leaves to its scheduler is a parameter here: `seed` != 0 shuffles the order in which
// tiles, slots and forward neighbours are visited in every phase, and `stale` runs the seam phase on a memory whose loads return a
// randomly chosen EARLIER value of the word (a history per word; the atomic min sees the truth) -- vrt_label.h's second sentence, put
// to the test.  tests/label.py compiles this with g++ and calls it through ctypes.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/vrt_api.h"
#include "../../voxel_rt2_amd/csrc/vrt_label.h"
#include "../../voxel_rt2_amd/csrc/vrt_plan.h"

using namespace vrt;

namespace {

struct Rng {
    unsigned long long s;
    unsigned next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (unsigned)(s >> 33); }
    template <class T> void shuffle(std::vector<T>& v) {
        for (size_t i = v.size(); i > 1; i--) { const size_t j = next() % i; const T t = v[i - 1]; v[i - 1] = v[j]; v[j] = t; }
    }
};

struct TileWords {   // names: tile-local slots
    int* s;
    int load(int i) const { return s[i]; }
    int atomic_min(int i, int v) const { const int old = s[i]; if (v < old) s[i] = v; return old; }
};
struct BoxWords {   // names: grid indices
    int* L;
    const LabelBox& p;
    int load(int g) const { return L[label_box_of_grid(p, g)]; }
    int atomic_min(int g, int v) const { int& w = L[label_box_of_grid(p, g)]; const int old = w; if (v < old) w = v; return old; }
    void store(int g, int v) const { L[label_box_of_grid(p, g)] = v; }
};
struct StaleWords {   // every value a word has held; a load returns any of them
    std::vector<std::vector<int>>& hist;
    const LabelBox& p;
    Rng& rng;
    int load(int g) const { const std::vector<int>& h = hist[(size_t)label_box_of_grid(p, g)]; return h[rng.next() % h.size()]; }
    int atomic_min(int g, int v) const { std::vector<int>& h = hist[(size_t)label_box_of_grid(p, g)]; const int old = h.back(); if (v < old) h.push_back(v); return old; }
};
struct Item { int tile, t, k; };

template <class M>
void seam_phase(M& m, const LabelBox& p, const std::vector<Item>& items) {
    for (const Item& it : items) label_seam_link(m, p, label_tile(p, it.tile), it.t, it.k);
}

int flags_bad(unsigned flags) {
    const unsigned both = VRT_LABEL_CONN_18 | VRT_LABEL_CONN_26;
    return (flags & ~(unsigned)(VRT_LABEL_EMPTY | both)) != 0u || (flags & both) == both;
}

}  // namespace

extern "C" {
// plan_label_layout's byte count for a box of nv cells
long long label_emul_plan(long long nv, int staged) { return (long long)plan_label_layout((size_t)nv, staged != 0).bytes; }
// the tile's edges
void label_emul_tile(int* out) { out[0] = VRT_LABEL_TX; out[1] = VRT_LABEL_TY; out[2] = VRT_LABEL_TZ; }
// the forward neighbours of a connectivity: out[3 * k ..] = the k-th offset; returns their number
int label_emul_forward(unsigned flags, int* out) {
    EditBox b{{0, 0, 0}, {1, 1, 1}};
    const LabelBox p = label_plan_box(b, 8, flags);
    for (int k = 0; k < p.forward; k++) label_forward(k, out[3 * k], out[3 * k + 1], out[3 * k + 2]);
    return p.forward;
}
// vrt_label_components on host arrays: mat int8[G][G][G]; scratch: at least label_emul_plan bytes; staged: the host path (labels
// worked in the scratch, then copied out), else the device path (worked in `labels`).  after_tiles, if not NULL: the words as
// k_label_tile leaves them.  Returns vrt_label_components' code.
int label_emul_call(int G, const int8_t* mat, const int* lo, const int* hi, unsigned flags, int* labels, vrt_label_result* result, uint8_t* scratch, int staged,
                    unsigned seed, int stale, int* after_tiles) {
    if (!mat || !lo || !hi || !labels) return VRT_E_INVALID;
    EditBox box;
    for (int a = 0; a < 3; a++) { box.lo[a] = lo[a]; box.hi[a] = hi[a]; }
    if (!edit_box_valid(box, G)) return VRT_E_INVALID;
    if (flags_bad(flags)) return VRT_E_INVALID;
    const int nv = edit_box_voxels(box);
    if (nv == 0) {
        if (result) memset(result, 0, sizeof(*result));
        return VRT_OK;
    }
    const LabelBox p = label_plan_box(box, G, flags);
    const LabelLayout l = plan_label_layout((size_t)nv, staged != 0);
    vrt_label_result* counters = (vrt_label_result*)(scratch + l.result_at);
    int* L = staged ? (int*)(scratch + l.labels_at) : labels;
    Rng rng{seed * 2654435761ULL + 1ULL};
    memset(counters, 0, sizeof(*counters));
    // k_label_tile
    std::vector<int> tiles((size_t)label_tile_count(p));
    for (size_t i = 0; i < tiles.size(); i++) tiles[i] = (int)i;
    if (seed) rng.shuffle(tiles);
    std::vector<int> s((size_t)VRT_LABEL_TILE);
    std::vector<Item> items;
    for (int tile : tiles) {
        const LabelTile r = label_tile(p, tile);
        TileWords m{s.data()};
        for (int t = 0; t < VRT_LABEL_TILE; t++) s[(size_t)t] = label_tile_seed(p, r, mat, t);
        items.clear();
        for (int t = 0; t < VRT_LABEL_TILE; t++)
            if (m.load(t) >= 0) for (int k = 0; k < p.forward; k++) items.push_back(Item{tile, t, k});
        if (seed) rng.shuffle(items);
        for (const Item& it : items) label_tile_link(m, r, it.t, it.k);
        for (int t = 0; t < VRT_LABEL_TILE; t++) {
            int lx, ly, lz;
            label_tile_cell(t, lx, ly, lz);
            if (label_in_tile(r, lx, ly, lz)) L[label_box_index(p, r.o[0] + lx, r.o[1] + ly, r.o[2] + lz)] = label_tile_result(m, p, r, t);
        }
    }
    if (after_tiles) memcpy(after_tiles, L, 4 * (size_t)nv);
    // k_label_seams
    if (tiles.size() > 1) {
        items.clear();
        BoxWords truth{L, p};
        for (int tile : tiles) {
            const LabelTile r = label_tile(p, tile);
            for (int t = 0; t < VRT_LABEL_TILE; t++) {
                int lx, ly, lz;
                label_tile_cell(t, lx, ly, lz);
                if (!label_in_tile(r, lx, ly, lz) || !label_on_seam(p, r, lx, ly, lz)) continue;
                if (truth.load(label_grid_index(p, r.o[0] + lx, r.o[1] + ly, r.o[2] + lz)) < 0) continue;
                for (int k = 0; k < p.forward; k++) items.push_back(Item{tile, t, k});
            }
        }
        if (seed) rng.shuffle(items);
        if (stale) {
            std::vector<std::vector<int>> hist((size_t)nv);
            for (int i = 0; i < nv; i++) hist[(size_t)i].push_back(L[i]);
            StaleWords m{hist, p, rng};
            seam_phase(m, p, items);
            for (int i = 0; i < nv; i++) L[i] = hist[(size_t)i].back();
        } else {
            seam_phase(truth, p, items);
        }
    }
    // k_label_finish
    std::vector<int> cells((size_t)nv);
    for (int i = 0; i < nv; i++) cells[(size_t)i] = i;
    if (seed) rng.shuffle(cells);
    BoxWords m{L, p};
    for (int i : cells) {
        bool member, root;
        label_finish_cell(m, p, i / (p.n[2] * p.n[1]), i / p.n[2] % p.n[1], i % p.n[2], member, root);
        counters->cells += member;
        counters->components += root;
    }
    if (staged) memcpy(labels, L, 4 * (size_t)nv);
    if (result) *result = *counters;
    return VRT_OK;
}
}
