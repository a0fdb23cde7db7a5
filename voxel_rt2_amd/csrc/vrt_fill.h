// vrt_fill.h -- vrt_fill_triangles: the inside of a closed triangle mesh filled with voxels in a box of a prepared grid.  A triangle's
// set-up for the parity test (edge functions, plane function, tie signs), the column test, the first cell of a column above the triangle,
// the columns a triangle can own at all, its work items and one lane's share of an item, the toggle bit of (column, cell), the prefix-XOR
// of a column's toggle words, and one voxel of the resolve.  Plain functions over plain values, in the style of vrt_voxelize.h, whose
// snap and validity gate are used as they are: the k_fill_* kernels (vrt_scene_kernels.hip) are loops over them, and
// tests/emul/fill_emul.cpp runs the same loops on a machine without a GPU (tests/test_fill_host.py).
//
// WHAT IS COMPUTED (include/vrt_api.h, INSIDE).  Cell c is inside iff an odd number of valid triangles cross below its centre
// q = 64 c + 32, the centre taken at q + (eps, eps^2, eps^3).  For a column (c_x, c_y) a triangle either owns it (the perturbed
// vertical line meets the triangle) or not, and if it does, it crosses below exactly the cells from fill_first_cell upwards.  So a
// triangle TOGGLES one bit per owned column, at its first cell, and a cell is inside iff the XOR of the toggles at and below it is
// set: the prefix-XOR of the column.  XOR commutes: scheduling, batches and the host path's chunks cannot change a bit.
//
// EVERYTHING IS PREMULTIPLIED BY sigma = sign(n_z), so that "in" reads > 0 for either orientation and sigma F is non-decreasing in c_z.
//
// HEADROOM (vrt_voxelize.h: |s| < 2^17, edge components < 2^18, normal components < 2^37).  An edge function
// E = d_x (q_y - p_y) - d_y (q_x - p_x) has two terms below 2^18 * 2^17: |E| < 2^36.  It is formed as E(0, 0) + 64 (d_x c_y - d_y c_x),
// the bracket in int32: |c| <= 2^11 covers every cell of a valid triangle's bounds (at most 9 * 128 = 1152 voxels from the origin), so
// the bracket stays below 2 * 2^18 * 2^11 = 2^30.  The plane function F = n . (q - v0) has three terms below 2^37 * 2^17: < 3 * 2^54 < 2^56.
// int64 never overflows (tests/test_fill_host.py runs the extreme triangles against unbounded integers).
#pragma once
#include "vrt_voxelize.h"

namespace vrt {

// ---- the set-up -----------------------------------------------------------------------------------------------------------------------
struct FillTri {
    int32_t v[3][3];              // the snapped vertices
    int32_t bmin[3], bmax[3];     // their bounds
    int64_t nn[3];                // e0 x e1, as vox_axes forms it
    int32_t sigma;                // sign(n_z); 0: edge-on or degenerate seen along z, crosses nothing
    int32_t dx[3], dy[3];         // sigma d of the directed edges v0->v1, v1->v2, v2->v0
    int64_t e0[3];                // sigma E of each edge at cell (0, 0)
    bool etie[3];                 // E == 0: sigma E' > 0, E' the sign of the first non-zero of (-d_y, d_x)
    int64_t fx, fy, f0;           // sigma n_x, sigma n_y, and sigma F at cell (0, 0, 0)
    int64_t slope;                // 64 |n_z|: what sigma F gains per cell along z
    bool ftie;                    // F == 0: sigma F' > 0, F' the sign of the first non-zero of (n_x, n_y, n_z)
};
VRT_DEV int fill_sign(int64_t x) { return x > 0 ? 1 : x < 0 ? -1 : 0; }
VRT_DEV void fill_setup(const vrt_triangle& t, int G, FillTri& s) {
    VoxTri u;
    vox_snap_tri(t, G, u);
    for (int a = 0; a < 3; a++) {
        for (int i = 0; i < 3; i++) s.v[i][a] = u.v[i][a];
        s.bmin[a] = u.bmin[a]; s.bmax[a] = u.bmax[a];
    }
    int32_t e[2][3];
    for (int a = 0; a < 3; a++) { e[0][a] = s.v[1][a] - s.v[0][a]; e[1][a] = s.v[2][a] - s.v[1][a]; }
    s.nn[0] = (int64_t)e[0][1] * e[1][2] - (int64_t)e[0][2] * e[1][1];
    s.nn[1] = (int64_t)e[0][2] * e[1][0] - (int64_t)e[0][0] * e[1][2];
    s.nn[2] = (int64_t)e[0][0] * e[1][1] - (int64_t)e[0][1] * e[1][0];
    const int sg = fill_sign(s.nn[2]);
    s.sigma = sg;
    for (int i = 0; i < 3; i++) {
        const int32_t* p = s.v[i];
        const int32_t* r = s.v[(i + 1) % 3];
        const int32_t dx = r[0] - p[0], dy = r[1] - p[1];
        s.dx[i] = sg * dx; s.dy[i] = sg * dy;
        s.e0[i] = sg * ((int64_t)dx * (32 - p[1]) - (int64_t)dy * (32 - p[0]));
        s.etie[i] = sg * (dy != 0 ? -fill_sign(dy) : fill_sign(dx)) > 0;
    }
    s.fx = sg * s.nn[0]; s.fy = sg * s.nn[1];
    s.f0 = sg * (s.nn[0] * (32 - s.v[0][0]) + s.nn[1] * (32 - s.v[0][1]) + s.nn[2] * (32 - s.v[0][2]));
    s.slope = 64 * (sg * s.nn[2]);
    s.ftie = sg * (s.nn[0] != 0 ? fill_sign(s.nn[0]) : s.nn[1] != 0 ? fill_sign(s.nn[1]) : sg) > 0;
}

// ---- the column test and the first cell ---------------------------------------------------------------------------------------------
// Does the vertical line through the perturbed centre of column (cx, cy) meet the triangle?  sigma E' > 0 on all three edges.
VRT_DEV bool fill_column_in(const FillTri& s, int cx, int cy) {
    if (s.sigma == 0) return false;
    for (int i = 0; i < 3; i++) {
        const int64_t E = s.e0[i] + 64 * (int64_t)(s.dx[i] * cy - s.dy[i] * cx);
        if (E < 0 || (E == 0 && !s.etie[i])) return false;
    }
    return true;
}
// The smallest c_z, unbounded, whose cell the triangle crosses below, for a column that is in: sigma F = A + slope c_z with
// A = sigma F at c_z = 0, and the cell counts iff sigma F > 0, or sigma F == 0 and the tie says so: A + slope c_z >= t with t = 0 or 1,
// c_z = ceil((t - A) / slope), one floor division (slope > 0 because sigma != 0; |t - A + slope| < 2^57).
VRT_DEV int64_t fill_first_cell(const FillTri& s, int cx, int cy) {
    const int64_t A = s.f0 + 64 * (s.fx * cx + s.fy * cy);
    const int64_t num = (s.ftie ? 0 : 1) - A + s.slope - 1;
    int64_t q = num / s.slope;
    if (num - q * s.slope < 0) q--;   // (C++ division truncates towards zero)
    return q;
}

// ---- the columns a triangle can own at all ------------------------------------------------------------------------------------------
// The perturbed centre of an owned column lies strictly inside the projected triangle, so its centre lies within the closed xy bounds:
// 64 c + 32 in [bmin, bmax], c from (bmin + 31) >> 6 to (bmax - 32) >> 6, clipped to the box: an EditCells in two dimensions (one
// layer on z).  None if the triangle is edge-on along z, or if it lies wholly above the box: its first cell in any column is at least
// (bmin_z + 31) >> 6, and nothing is toggled at or beyond hi_z.  A triangle BELOW the box keeps its columns.
VRT_DEV EditCells fill_cells(const FillTri& s, const EditBox& clip) {
    EditCells r;
    bool empty = s.sigma == 0 || ((s.bmin[2] + 31) >> 6) >= clip.hi[2];
    for (int a = 0; a < 2; a++) {
        int lo = (s.bmin[a] + 31) >> 6, hi = (s.bmax[a] - 32) >> 6;
        if (lo < clip.lo[a]) lo = clip.lo[a];
        if (hi > clip.hi[a] - 1) hi = clip.hi[a] - 1;   // (the clip box is not empty: the caller checks)
        r.lo[a] = lo; r.n[a] = hi - lo + 1;
        if (hi < lo) empty = true;
    }
    r.lo[2] = 0; r.n[2] = 1;
    if (empty) for (int a = 0; a < 3; a++) { r.lo[a] = 0; r.n[a] = 0; }
    return r;
}
// ---- work items -------------------------------------------------------------------------------------------------------------------------
// A triangle's work is cut into ITEMS: one aligned tile of 16 x 16 columns that holds some of fill_cells each, x running fastest
// (edit_cell).  A triangle spanning a 256^3 grid has 256 of them, a wave takes one at a time; a small triangle has one to four.
// Entries, item numbers and the search are vrt_voxelize.h's (VoxEntry, vox_find_entry).
VRT_DEV EditCells fill_tiles(const EditCells& cells) {
    EditCells r;
    for (int a = 0; a < 3; a++) { r.lo[a] = 0; r.n[a] = 0; }
    if (cells.n[0] == 0) return r;
    for (int a = 0; a < 2; a++) { r.lo[a] = cells.lo[a] >> 4; r.n[a] = ((cells.lo[a] + cells.n[a] - 1) >> 4) - r.lo[a] + 1; }
    r.n[2] = 1;
    return r;
}
// items of triangle t clipped to `clip` (0: invalid, edge-on, above the box, or no column of the box); valid reports the gate
VRT_DEV uint32_t fill_tri_items(const vrt_triangle& t, int G, const EditBox& clip, bool& valid) {
    valid = vox_tri_valid(t);
    if (!valid) return 0u;
    FillTri s;
    fill_setup(t, G, s);
    return (uint32_t)edit_cell_count(fill_tiles(fill_cells(s, clip)));
}
// One lane's share of an item: the k-th (0 .. 3) of its four columns of tile (tx, ty) -- x = lane & 15, y = lane >> 4 plus 4 k, so that
// a wave's 64 lanes are four rows of 16 -- and whether the triangle owns it.
VRT_DEV bool fill_lane_column(const FillTri& s, const EditCells& cells, int tx, int ty, int lane, int k, int& cx, int& cy) {
    cx = tx * 16 + (lane & 15);
    cy = ty * 16 + (lane >> 4) + 4 * k;
    if (cx < cells.lo[0] || cx >= cells.lo[0] + cells.n[0] || cy < cells.lo[1] || cy >= cells.lo[1] + cells.n[1]) return false;
    return fill_column_in(s, cx, cy);
}

// ---- the toggle bitmap ------------------------------------------------------------------------------------------------------------------
// One bit per voxel of the box, bits running along z: column (x, y) of the box is fill_words_z consecutive 32-bit words, bit z' & 31
// of word z' >> 5 for z' = c_z - lo_z.  A first cell below the box is clamped up to lo_z (the triangle crosses below every cell of
// the column); at or beyond hi_z nothing is toggled (it crosses below none).
VRT_DEV int fill_words_z(const EditBox& b) { return (b.hi[2] - b.lo[2] + 31) >> 5; }
VRT_DEV int fill_words(const EditBox& b) { return (b.hi[0] - b.lo[0]) * (b.hi[1] - b.lo[1]) * fill_words_z(b); }   // at most 256 * 256 * 8
// the word (-1: none) and the bit mask of column (cx, cy) of the box for a first cell `first`
VRT_DEV int fill_toggle_at(const EditBox& b, int cx, int cy, int64_t first, uint32_t& bit) {
    if (first >= (int64_t)b.hi[2]) return -1;
    const int z = first <= (int64_t)b.lo[2] ? 0 : (int)first - b.lo[2];
    bit = 1u << (z & 31);
    return ((cx - b.lo[0]) * (b.hi[1] - b.lo[1]) + (cy - b.lo[1])) * fill_words_z(b) + (z >> 5);
}
// The prefix-XOR of one word of a column: bit k of the result = carry ^ (XOR of bits 0 .. k of w) = is cell 32 word + k inside;
// the carry leaves as the word's top bit, for the next word up.
VRT_DEV uint32_t fill_prefix_word(uint32_t w, uint32_t& carry) {
    w ^= w << 1; w ^= w << 2; w ^= w << 4; w ^= w << 8; w ^= w << 16;
    if (carry) w = ~w;
    carry = w >> 31;
    return w;
}

// ---- the resolve ------------------------------------------------------------------------------------------------------------------------
// Voxel i of the box arrays: the payload if the cell is inside, the grid's stored voxel otherwise.  The column's words are prefixed
// from the bottom up to the voxel's own (at most eight; a wave's lanes are neighbours along z and read the same few).  Returns INSIDE.
VRT_DEV bool fill_resolve_voxel(const EditBox& b, int G, int i, const uint32_t* toggles, uint32_t payload, const int8_t* mat, const uint8_t* rgb,
                                int8_t* box_mat, uint8_t* box_rgb) {
    const int hz = b.hi[2] - b.lo[2], z = i % hz;
    const uint32_t* col = toggles + (i / hz) * fill_words_z(b);
    uint32_t carry = 0u, w = 0u;
    for (int k = 0; k <= (z >> 5); k++) w = fill_prefix_word(col[k], carry);
    const bool inside = ((w >> (z & 31)) & 1u) != 0u;
    if (inside) {
        box_mat[i] = (int8_t)(uint8_t)(payload >> 24);
        box_rgb[3 * i] = (uint8_t)payload; box_rgb[3 * i + 1] = (uint8_t)(payload >> 8); box_rgb[3 * i + 2] = (uint8_t)(payload >> 16);
    } else {
        int x, y, zz;
        edit_box_voxel(b, i, x, y, zz);
        const int g = edit_grid_index(G, x, y, zz);
        box_mat[i] = mat[g];
        for (int k = 0; k < 3; k++) box_rgb[3 * i + k] = rgb[3 * g + k];
    }
    return inside;
}

}  // namespace vrt
