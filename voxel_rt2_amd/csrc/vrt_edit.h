// vrt_edit.h -- the index arithmetic of vrt_update_voxels: replacing the voxels of a box [lo, hi) of a prepared grid at a cost that
// follows the box, not the grid.  Which voxel a box-local index is and where it sits in the grid's arrays, which cells of a pyramid
// level a box touches, and the rebuild of one word of a level.  Plain functions over plain values: the k_edit_* kernels
// (vrt_scene_kernels.hip) are loops over them, one index per thread, and tests/emul/edit_emul.cpp runs the same loops on a machine without
// a GPU (tests/test_voxel_edit_host.py).
//
// A word is always RECOMPUTED from the level below (the fine level from the materials), never patched: a removed voxel clears its
// bit, and the last voxel of a cell clears the cell's bit all the way up.  Levels are rebuilt bottom up, each after the one below.
#pragma once
#include <cstring>
#include "vrt_trace.h"

namespace vrt {

struct EditBox { int lo[3], hi[3]; };   // voxels [lo, hi) per axis, the index space of vrt_upload_voxels: 0 <= lo <= hi <= G

VRT_DEV bool edit_box_valid(const EditBox& b, int G) {
    for (int a = 0; a < 3; a++) if (b.lo[a] < 0 || b.lo[a] > b.hi[a] || b.hi[a] > G) return false;
    return true;
}
VRT_DEV int edit_box_voxels(const EditBox& b) { return (b.hi[0] - b.lo[0]) * (b.hi[1] - b.lo[1]) * (b.hi[2] - b.lo[2]); }   // at most 256^3
// voxel `i` of the box arrays (mat int8[hx][hy][hz], rgb uint8[hx][hy][hz][3], C order: z runs fastest) -> its grid coordinates
VRT_DEV void edit_box_voxel(const EditBox& b, int i, int& x, int& y, int& z) {
    const int hy = b.hi[1] - b.lo[1], hz = b.hi[2] - b.lo[2];
    z = b.lo[2] + i % hz;
    y = b.lo[1] + (i / hz) % hy;
    x = b.lo[0] + i / (hz * hy);
}
VRT_DEV int edit_grid_index(int G, int x, int y, int z) { return (x * G + y) * G + z; }   // [x][y][z]: d_mat, and d_rgb at 3 x this

// k_pack_grid's texel (voxel_world.py:69-87): a negative material byte stores alpha 0
VRT_DEV uint32_t edit_pack_texel(int8_t m, const uint8_t* rgb) {
    const uint32_t a = (m < 0) ? 0u : (uint32_t)m;
    return (uint32_t)rgb[0] | ((uint32_t)rgb[1] << 8) | ((uint32_t)rgb[2] << 16) | (a << 24);
}
// Store and pack voxel `i` of the box: the grid's material and colour arrays (what a later plain vrt_prepare reads) and its texel.
template <int G>
VRT_DEV void edit_store_voxel(const EditBox& b, int i, const int8_t* box_mat, const uint8_t* box_rgb, int8_t* mat, uint8_t* rgb, uint32_t* grid) {
    int x, y, z;
    edit_box_voxel(b, i, x, y, z);
    const int g = edit_grid_index(G, x, y, z);
    const int8_t m = box_mat[i];
    mat[g] = m;
    for (int k = 0; k < 3; k++) rgb[3 * g + k] = box_rgb[3 * i + k];
    grid[texel_index<G>(x, y, z)] = edit_pack_texel(m, box_rgb + 3 * i);
}

// The cells of edge (1 << shift) voxels a non-empty box touches: n[a] cells from lo[a] on each axis.
// shift 2: the 4^3 bricks (l0 words), 4: the 16^3 cells (l1 words), 6: the 64^3 cells (l2 words), 8: the l3 word.
struct EditCells { int lo[3], n[3]; };
VRT_DEV EditCells edit_cells(const EditBox& b, int shift) {
    EditCells c;
    for (int a = 0; a < 3; a++) { c.lo[a] = b.lo[a] >> shift; c.n[a] = ((b.hi[a] - 1) >> shift) - c.lo[a] + 1; }
    return c;
}
VRT_DEV int edit_cell_count(const EditCells& c) { return c.n[0] * c.n[1] * c.n[2]; }
// the i-th touched cell, x running fastest like the words of a level
VRT_DEV void edit_cell(const EditCells& c, int i, int& cx, int& cy, int& cz) {
    cx = c.lo[0] + i % c.n[0];
    cy = c.lo[1] + (i / c.n[0]) % c.n[1];
    cz = c.lo[2] + i / (c.n[0] * c.n[1]);
}
VRT_DEV int edit_word_index(int n, int cx, int cy, int cz) { return (cz * n + cy) * n + cx; }   // a level of n^3 words

// One fine word from the materials (k_build_l0: bit z*16 + y*4 + x = material > 0, signed).  The four voxels of a z run are
// four consecutive bytes at a multiple of four: one load.
VRT_DEV unsigned long long edit_fine_word(const int8_t* mat, int G, int bx, int by, int bz) {
    unsigned long long w = 0ULL;
    for (int y = 0; y < 4; y++)
        for (int x = 0; x < 4; x++) {
            int8_t run[4];
            memcpy(run, mat + edit_grid_index(G, bx * 4 + x, by * 4 + y, bz * 4), 4);
            for (int z = 0; z < 4; z++) if (run[z] > 0) w |= 1ULL << (z * 16 + y * 4 + x);
        }
    return w;
}
// One word of a coarser level of n_coarse^3 words from the level below it (k_build_coarse: one bit per non-zero child word)
VRT_DEV unsigned long long edit_coarse_word(const unsigned long long* fine, int n_coarse, int bx, int by, int bz) {
    const int n_fine = n_coarse * 4;
    unsigned long long w = 0ULL;
    for (int z = 0; z < 4; z++)
        for (int y = 0; y < 4; y++)
            for (int x = 0; x < 4; x++)
                if (fine[edit_word_index(n_fine, bx * 4 + x, by * 4 + y, bz * 4 + z)] != 0ULL) w |= 1ULL << (z * 16 + y * 4 + x);
    return w;
}
// The i-th fine word the box touches, rebuilt in place.
VRT_DEV void edit_rebuild_fine(const EditBox& b, int i, const int8_t* mat, unsigned long long* l0, int G) {
    int bx, by, bz;
    edit_cell(edit_cells(b, 2), i, bx, by, bz);
    l0[edit_word_index(G >> 2, bx, by, bz)] = edit_fine_word(mat, G, bx, by, bz);
}
// The i-th word the box touches of the level whose cells have edge (1 << shift) voxels (4: l1, 6: l2, 8: l3), from the level below.
VRT_DEV void edit_rebuild_coarse(const EditBox& b, int shift, int i, const unsigned long long* fine, unsigned long long* coarse, int G) {
    int bx, by, bz;
    edit_cell(edit_cells(b, shift), i, bx, by, bz);
    const int n_coarse = G >> shift;
    coarse[edit_word_index(n_coarse, bx, by, bz)] = edit_coarse_word(fine, n_coarse, bx, by, bz);
}

}  // namespace vrt
