// vrt_label.h -- the arithmetic of vrt_label_components: which MEMBER cells of a box (solid, or with VRT_LABEL_EMPTY non-solid) hang
// together under 6-, 18- or 26-adjacency, every cell labelled with the smallest linear grid index of its component.  Plain functions
// over plain values: the k_label_* kernels (vrt_scene_kernels.hip) are loops over them, and tests/emul/label_emul.cpp runs the same loops on a
// machine without a GPU (tests/test_label_host.py), in any order it likes.
//
// THE FOREST.  Every member owns one word that names a member of its own set: its PARENT, and the invariant is L[x] <= x.  A cell with
// L[x] == x is a ROOT.  Linking only ever lowers a word (atomic min), so the invariant holds at every instant, every chain of parents
// strictly descends and ends in a root, and when all links are made a set's only root is its smallest cell.
// THE NAMES are linear GRID indices (x G + y) G + z from k_label_tile's stores on, although the words sit box-locally (label_box_of_grid
// finds the word of a name): the index order of the grid is the index order of the box, so "smallest" is the same cell either way, and
// the final label -- the root's grid index -- is then just one more parent, the best one.  That is what lets k_label_finish write its
// result into the very words other threads still read parents from: whichever of the two values a reader gets names a smaller-or-equal
// member of the same set.
// THE PHASES.  A box is cut into TILES of VRT_LABEL_TX x TY x TZ cells from its own corner (vrt_plan.h).  k_label_tile solves a tile in
// LDS over tile-local names (the same order again) and stores each member's tile root; k_label_seams unites across tile faces in
// global memory; k_label_finish walks every cell to its root.  Each adjacent pair of members is united exactly once: by the earlier
// cell of the pair, through the FORWARD half of the neighbourhood (label_forward), in the tile phase if the pair shares a tile and
// in the seam phase if not.
// LABEL_UNION(a, b), the lock-free min-link loop: find both roots; equal: done; order them a > b; old = atomic_min(&L[a], b); if
// old == a, a was a root and now hangs below b: done; otherwise a had the parent `old` already, and the loop goes on uniting old with b
// (old and a are one set, and if old > b the word now says b: old's set must still meet b's).
// WHY IT ENDS AND WHY IT IS RIGHT -- the two sentences the kernels rely on:
//   1. Every iteration strictly lowers a value -- a find step moves to a smaller name, a failed link replaces a by old < a, so
//      max(a, b) falls -- so the loop ends, after at most as many steps as the names are large.
//   2. The loop stays correct when a find returns a STALE NON-ROOT of the same set (a word read from a cache another CU never
//      refreshed: an earlier value of it, which also named a member of the set), because the atomic read-modify-write sees the truth
//      -- old != a -- and the loop continues from it.
// Nothing waits for anybody: no thread's progress depends on another's.
#pragma once
#include "vrt_edit.h"
#include "vrt_plan.h"

namespace vrt {

#define VRT_LABEL_NONE (-1)   // the word of a cell that is no member; also its label

struct LabelBox {
    EditBox box;
    int G, shift;     // the grid's edge; its log2 if a power of two, else 0 (label_box_of_grid divides)
    int n[3];         // the box's extent
    int tiles[3];     // tiles per axis
    int forward;      // forward neighbours: 3, 9 or 13
    int empty;        // members are the non-solid cells
};
VRT_DEV LabelBox label_plan_box(const EditBox& b, int G, uint32_t flags) {
    LabelBox p;
    p.box = b;
    p.G = G;
    p.shift = 0;
    for (int s = 1; s < 16; s++) if ((1 << s) == G) p.shift = s;
    const int t[3] = {VRT_LABEL_TX, VRT_LABEL_TY, VRT_LABEL_TZ};
    for (int a = 0; a < 3; a++) { p.n[a] = b.hi[a] - b.lo[a]; p.tiles[a] = (p.n[a] + t[a] - 1) / t[a]; }
    p.forward = (flags & 4u) ? 13 : (flags & 2u) ? 9 : 3;   // VRT_LABEL_CONN_26, VRT_LABEL_CONN_18
    p.empty = (flags & 1u) != 0u;                            // VRT_LABEL_EMPTY
    return p;
}
VRT_DEV int label_tile_count(const LabelBox& p) { return p.tiles[0] * p.tiles[1] * p.tiles[2]; }

// SOLID is the fine occupancy bit: material byte > 0, signed
VRT_DEV bool label_member(int8_t m, int empty) { return (m > 0) != (empty != 0); }

// The forward neighbours: the 13 offsets that are lexicographically later in (x, y, z), those with |d|_1 = 1 first (k < 3), then
// |d|_1 = 2 (k < 9), then 3 -- two bits per offset and axis in one word per axis.
constexpr uint32_t label_forward_code(int axis) {
    const int t[13][3] = {{0, 0, 1}, {0, 1, 0}, {1, 0, 0}, {0, 1, -1}, {0, 1, 1}, {1, -1, 0}, {1, 1, 0}, {1, 0, -1}, {1, 0, 1}, {1, -1, -1}, {1, -1, 1}, {1, 1, -1}, {1, 1, 1}};
    uint32_t w = 0;
    for (int k = 0; k < 13; k++) w |= (uint32_t)(t[k][axis] + 1) << (2 * k);
    return w;
}
VRT_DEV void label_forward(int k, int& dx, int& dy, int& dz) {
    constexpr uint32_t X = label_forward_code(0), Y = label_forward_code(1), Z = label_forward_code(2);
    dx = (int)((X >> (2 * k)) & 3u) - 1;
    dy = (int)((Y >> (2 * k)) & 3u) - 1;
    dz = (int)((Z >> (2 * k)) & 3u) - 1;
}

// box-local coordinates (0 <= b < n) <-> the word's place, the cell's name
VRT_DEV int label_box_index(const LabelBox& p, int bx, int by, int bz) { return (bx * p.n[1] + by) * p.n[2] + bz; }
VRT_DEV int label_grid_index(const LabelBox& p, int bx, int by, int bz) { return edit_grid_index(p.G, p.box.lo[0] + bx, p.box.lo[1] + by, p.box.lo[2] + bz); }
VRT_DEV int label_box_of_grid(const LabelBox& p, int g) {
    int x, y, z;
    if (p.shift) { x = g >> (2 * p.shift); y = (g >> p.shift) & (p.G - 1); z = g & (p.G - 1); }
    else { x = g / (p.G * p.G); y = g / p.G % p.G; z = g % p.G; }
    return label_box_index(p, x - p.box.lo[0], y - p.box.lo[1], z - p.box.lo[2]);
}

// A tile: its corner in box-local coordinates and its extent, cut by the box.  Tile-local name t = (lx TY + ly) TZ + lz, z fastest.
struct LabelTile { int o[3], n[3]; };
VRT_DEV LabelTile label_tile(const LabelBox& p, int i) {   // the i-th tile, z running fastest
    const int t[3] = {VRT_LABEL_TX, VRT_LABEL_TY, VRT_LABEL_TZ};
    const int c[3] = {i / (p.tiles[2] * p.tiles[1]), i / p.tiles[2] % p.tiles[1], i % p.tiles[2]};
    LabelTile r;
    for (int a = 0; a < 3; a++) { r.o[a] = c[a] * t[a]; r.n[a] = p.n[a] - r.o[a] < t[a] ? p.n[a] - r.o[a] : t[a]; }
    return r;
}
VRT_DEV void label_tile_cell(int t, int& lx, int& ly, int& lz) { lz = t % VRT_LABEL_TZ; ly = t / VRT_LABEL_TZ % VRT_LABEL_TY; lx = t / (VRT_LABEL_TZ * VRT_LABEL_TY); }
VRT_DEV int label_tile_index(int lx, int ly, int lz) { return (lx * VRT_LABEL_TY + ly) * VRT_LABEL_TZ + lz; }
VRT_DEV bool label_in_tile(const LabelTile& r, int lx, int ly, int lz) { return lx >= 0 && ly >= 0 && lz >= 0 && lx < r.n[0] && ly < r.n[1] && lz < r.n[2]; }

// ---- the forest, over a memory policy M: load(name), atomic_min(name, value) -> the old word, store(name, value) -------------------------
template <class M>
VRT_DEV int label_find(M& m, int x) {
    for (;;) {
        const int parent = m.load(x);
        if (parent == x) return x;
        x = parent;   // parent < x
    }
}
template <class M>
VRT_DEV void label_union(M& m, int a, int b) {
    for (;;) {
        a = label_find(m, a);
        b = label_find(m, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = m.atomic_min(a, b);
        if (old == a) return;
        a = old;   // old < a: max(a, b) fell
    }
}

// ---- k_label_tile: names are tile-local, the words the tile's LDS --------------------------------------------------------------------------
// the seed of slot t: its own name for a member, VRT_LABEL_NONE for a non-member and for a slot outside the box
VRT_DEV int label_tile_seed(const LabelBox& p, const LabelTile& r, const int8_t* mat, int t) {
    int lx, ly, lz;
    label_tile_cell(t, lx, ly, lz);
    if (!label_in_tile(r, lx, ly, lz)) return VRT_LABEL_NONE;
    return label_member(mat[label_grid_index(p, r.o[0] + lx, r.o[1] + ly, r.o[2] + lz)], p.empty) ? t : VRT_LABEL_NONE;
}
// slot t, a MEMBER (the caller has looked), united with its k-th forward neighbour if that is a member inside the tile
template <class M>
VRT_DEV void label_tile_link(M& m, const LabelTile& r, int t, int k) {
    int lx, ly, lz, dx, dy, dz;
    label_tile_cell(t, lx, ly, lz);
    label_forward(k, dx, dy, dz);
    if (!label_in_tile(r, lx + dx, ly + dy, lz + dz)) return;
    const int u = label_tile_index(lx + dx, ly + dy, lz + dz);
    if (m.load(u) < 0) return;
    label_union(m, t, u);
}
// what the tile phase leaves in the box's word of slot t (inside the box): the NAME of its tile root, or VRT_LABEL_NONE
template <class M>
VRT_DEV int label_tile_result(M& m, const LabelBox& p, const LabelTile& r, int t) {
    if (m.load(t) < 0) return VRT_LABEL_NONE;
    int lx, ly, lz;
    label_tile_cell(label_find(m, t), lx, ly, lz);
    return label_grid_index(p, r.o[0] + lx, r.o[1] + ly, r.o[2] + lz);
}

// ---- k_label_seams: names are grid indices, the words the label array ---------------------------------------------------------------------
// can a forward neighbour of slot (lx, ly, lz) lie in another tile?  (dx is 0 or 1; dy and dz are -1, 0 or 1; 6-adjacency has no -1.)
VRT_DEV bool label_on_seam(const LabelBox& p, const LabelTile& r, int lx, int ly, int lz) {
    const bool back = p.forward > 3;
    return lx == r.n[0] - 1 || ly == r.n[1] - 1 || lz == r.n[2] - 1 || (back && (ly == 0 || lz == 0));
}
// slot t of tile r, a MEMBER (the caller has looked), united with its k-th forward neighbour if that is a member of the box in ANOTHER tile
template <class M>
VRT_DEV void label_seam_link(M& m, const LabelBox& p, const LabelTile& r, int t, int k) {
    int lx, ly, lz, dx, dy, dz;
    label_tile_cell(t, lx, ly, lz);
    label_forward(k, dx, dy, dz);
    if (label_in_tile(r, lx + dx, ly + dy, lz + dz)) return;
    const int bx = r.o[0] + lx + dx, by = r.o[1] + ly + dy, bz = r.o[2] + lz + dz;
    if (bx < 0 || by < 0 || bz < 0 || bx >= p.n[0] || by >= p.n[1] || bz >= p.n[2]) return;   // outside the box: does not exist
    const int c = label_grid_index(p, r.o[0] + lx, r.o[1] + ly, r.o[2] + lz), u = label_grid_index(p, bx, by, bz);
    if (m.load(u) < 0) return;
    label_union(m, c, u);
}

// ---- k_label_finish: the final mapping -- a member's root (a grid index already), a non-member VRT_LABEL_NONE ------------------------------------
// cell (bx, by, bz) of the box: stores and returns its label; member / root: what the counters take
template <class M>
VRT_DEV int label_finish_cell(M& m, const LabelBox& p, int bx, int by, int bz, bool& member, bool& root) {
    const int c = label_grid_index(p, bx, by, bz);
    member = m.load(c) >= 0;
    root = false;
    if (!member) return VRT_LABEL_NONE;
    const int r = label_find(m, c);
    root = r == c;
    if (!root) m.store(c, r);   // (a parent like any other to whoever still reads it)
    return r;
}

}  // namespace vrt
