// vrt_move.h -- the arithmetic of vrt_move_voxels: the voxels of a source box moved or copied under a fixed-point affine map that takes
// a DESTINATION cell to its SOURCE cell (include/vrt_api.h states the rules).  Plain functions over plain values: the k_move_* kernels
// (vrt_scene_kernels.hip) are loops over them, and tests/emul/move_emul.cpp runs the same loops on a machine without a GPU
// (tests/test_move_host.py).  Integers only: nothing here rounds.
//
// THE MAP.  S_a = sum_b m[3a+b] (2 d_b + 1) + t[a] in int64, the source cell s_a = S_a >> 17 (arithmetic: a floor).  |m| <= 2^20,
// 2 d + 1 < 2^9 and |t| <= 2^40 (move_valid) bound every product by 2^29, the three of a row by 2^31 and S by 2^41: no int64 operation
// can overflow, and s fits an int.  One step along z adds 2 m[3a+2] to S_a (move_step_z): the kernels walk a z run with it.
// THE SNAPSHOT.  One word per cell of the source box, written before anything changes: r | g << 8 | b << 16 | mat << 24 of a PIECE
// cell (selected, material > 0 -- so the word is not 0), else 0.  Everything the passes need of the source BEFORE is in it: a
// destination cell receives iff its source cell's word is not 0 and then takes the word's bytes; a cell is vacated iff
// VRT_MOVE_ERASE_SOURCE is set, it lies in the source box and its own word is not 0.
// THE PASSES.  snapshot over the source box; count over the destination box (blocked, written, the tight box -- VRT_MOVE_DRY_RUN ends
// here); then box arrays of the source box (vacated cells cleared) and of the destination box, each through launch_edit.  The
// destination's arrays are built AFTER the source box's edit and read the grid as that edit left it: a vacated cell is recognised
// by its snapshot word, not by the grid, and every cell that is not vacated still holds its bytes BEFORE, so move_dst_cell sees the
// same values in the count pass and in the build pass.  With VRT_MOVE_IF_FREE the build passes read the count pass's `blocked` and
// copy the grid's own bytes when it is not 0 (move_go).
#pragma once
#include "vrt_edit.h"

namespace vrt {

#define VRT_MOVE_M_MAX (1 << 20)
#define VRT_MOVE_T_MAX (1LL << 40)
#define VRT_MOVE_FLAGS 15u
// the destination box is cut into tiles of TX x TY x TZ cells from its own corner, a workgroup a tile; a thread walks VRT_MOVE_RUN cells along z
#define VRT_MOVE_TX 4
#define VRT_MOVE_TY 4
#define VRT_MOVE_TZ 64
#define VRT_MOVE_RUN 4
#define VRT_MOVE_TILE (VRT_MOVE_TX * VRT_MOVE_TY * VRT_MOVE_TZ)

// the call's arguments as the passes take them (vrt_voxel_move's fields; the boxes checked, not empty where a pass runs over them)
struct MovePlan {
    EditBox src, dst;
    int m[9];
    long long t[3];
    int select_value;
    unsigned flags;
    int G;
    int tiles[3];   // of the destination box
};
// the device's record: the tight box as a running minimum / inclusive maximum (move_record_begin), the three sums
struct MoveRecord { int lo[3], hi[3]; unsigned long long written, blocked, erased; };

VRT_DEV bool move_valid(const int m[9], const long long t[3], unsigned flags, unsigned reserved) {
    for (int i = 0; i < 9; i++) if (m[i] > VRT_MOVE_M_MAX || m[i] < -VRT_MOVE_M_MAX) return false;
    for (int a = 0; a < 3; a++) if (t[a] > VRT_MOVE_T_MAX || t[a] < -VRT_MOVE_T_MAX) return false;
    return (flags & ~VRT_MOVE_FLAGS) == 0u && reserved == 0u;
}
VRT_DEV MovePlan move_plan(const EditBox& src, const EditBox& dst, const int m[9], const long long t[3], int select_value, unsigned flags, int G) {
    MovePlan p;
    p.src = src; p.dst = dst;
    for (int i = 0; i < 9; i++) p.m[i] = m[i];
    for (int a = 0; a < 3; a++) p.t[a] = t[a];
    p.select_value = select_value; p.flags = flags; p.G = G;
    const int tile[3] = {VRT_MOVE_TX, VRT_MOVE_TY, VRT_MOVE_TZ};
    for (int a = 0; a < 3; a++) p.tiles[a] = (dst.hi[a] - dst.lo[a] + tile[a] - 1) / tile[a];
    return p;
}
VRT_DEV int move_tile_count(const MovePlan& p) { return p.tiles[0] * p.tiles[1] * p.tiles[2]; }

// ---- the map --------------------------------------------------------------------------------------------------------------------------
VRT_DEV void move_map(const MovePlan& p, int dx, int dy, int dz, long long S[3]) {
    for (int a = 0; a < 3; a++)
        S[a] = (long long)p.m[3 * a] * (2 * dx + 1) + (long long)p.m[3 * a + 1] * (2 * dy + 1) + (long long)p.m[3 * a + 2] * (2 * dz + 1) + p.t[a];
}
VRT_DEV void move_step_z(const MovePlan& p, long long S[3]) {   // S of (dx, dy, dz + 1) from S of (dx, dy, dz)
    for (int a = 0; a < 3; a++) S[a] += 2LL * p.m[3 * a + 2];
}
// the source cell of S: its index in the source box's arrays, or -1 where it lies outside the source box
VRT_DEV int move_source(const MovePlan& p, const long long S[3]) {
    int s[3];
    for (int a = 0; a < 3; a++) {
        const long long v = S[a] >> 17;
        if (v < p.src.lo[a] || v >= p.src.hi[a]) return -1;
        s[a] = (int)v - p.src.lo[a];
    }
    return (s[0] * (p.src.hi[1] - p.src.lo[1]) + s[1]) * (p.src.hi[2] - p.src.lo[2]) + s[2];
}
// grid cell (x, y, z): its index in the source box's arrays, or -1 outside it
VRT_DEV int move_src_index(const MovePlan& p, int x, int y, int z) {
    if (x < p.src.lo[0] || x >= p.src.hi[0] || y < p.src.lo[1] || y >= p.src.hi[1] || z < p.src.lo[2] || z >= p.src.hi[2]) return -1;
    return ((x - p.src.lo[0]) * (p.src.hi[1] - p.src.lo[1]) + (y - p.src.lo[1])) * (p.src.hi[2] - p.src.lo[2]) + (z - p.src.lo[2]);
}

// ---- the snapshot ---------------------------------------------------------------------------------------------------------------------
VRT_DEV bool move_selected(const MovePlan& p, const int* select, int i) { return select == nullptr || select[i] == p.select_value; }
VRT_DEV uint32_t move_snap_word(bool selected, int8_t mat, const uint8_t* rgb) {
    if (!selected || mat <= 0) return 0u;
    return (uint32_t)rgb[0] | ((uint32_t)rgb[1] << 8) | ((uint32_t)rgb[2] << 16) | ((uint32_t)(uint8_t)mat << 24);
}
// cell i of the source box: its word
VRT_DEV uint32_t move_snap_cell(const MovePlan& p, int i, const int8_t* mat, const uint8_t* rgb, const int* select) {
    int x, y, z;
    edit_box_voxel(p.src, i, x, y, z);
    const int g = edit_grid_index(p.G, x, y, z);
    return move_snap_word(move_selected(p, select, i), mat[g], rgb + 3 * (size_t)g);
}

// ---- the predicates -------------------------------------------------------------------------------------------------------------------
// own_word: the snapshot word of the cell itself, 0 for a cell outside the source box
VRT_DEV bool move_vacated(unsigned flags, uint32_t own_word) { return (flags & 1u) != 0u && own_word != 0u; }   // VRT_MOVE_ERASE_SOURCE
VRT_DEV bool move_occupied(int8_t mat_before, bool vacated) { return mat_before > 0 && !vacated; }
// does the call change the grid at all?  blocked: the count pass's sum
VRT_DEV bool move_go(unsigned flags, unsigned long long blocked) { return (flags & 8u) == 0u || blocked == 0ULL; }   // VRT_MOVE_IF_FREE

// ---- one destination cell -------------------------------------------------------------------------------------------------------------
struct MoveCell { int8_t mat; uint8_t rgb[3]; bool written, blocked; };
// from_word: the snapshot word of s(d), 0 where s(d) lies outside the source box; own_word: as for move_vacated; mat, rgb: the cell's
// stored bytes (BEFORE, or behind the source box's edit: the same for every cell that is not vacated, and unused for one that is)
VRT_DEV MoveCell move_dst_cell(unsigned flags, bool go, uint32_t from_word, uint32_t own_word, int8_t mat, const uint8_t* rgb) {
    MoveCell o;
    const bool receives = from_word != 0u, vacated = move_vacated(flags, own_word), occupied = move_occupied(mat, vacated);
    o.blocked = receives && occupied;
    o.written = go && receives && !((flags & 2u) != 0u && occupied);   // VRT_MOVE_KEEP_SOLID
    if (o.written) {
        o.mat = (int8_t)(from_word >> 24);
        o.rgb[0] = (uint8_t)from_word; o.rgb[1] = (uint8_t)(from_word >> 8); o.rgb[2] = (uint8_t)(from_word >> 16);
    } else if (go && vacated) {
        o.mat = 0; o.rgb[0] = o.rgb[1] = o.rgb[2] = 0;
    } else {
        o.mat = mat; o.rgb[0] = rgb[0]; o.rgb[1] = rgb[1]; o.rgb[2] = rgb[2];
    }
    return o;
}
// one source cell's outcome in the source box's arrays: cleared if vacated, else its stored bytes
VRT_DEV void move_src_cell(unsigned flags, bool go, uint32_t own_word, int8_t mat, const uint8_t* rgb, int8_t& out_mat, uint8_t* out_rgb) {
    const bool clear = go && move_vacated(flags, own_word);
    out_mat = clear ? (int8_t)0 : mat;
    for (int k = 0; k < 3; k++) out_rgb[k] = clear ? (uint8_t)0 : rgb[k];
}

// ---- the destination box's tiles: a workgroup a tile, a thread a run of VRT_MOVE_RUN cells along z ------------------------------------------
// run r (0 .. VRT_MOVE_TILE / VRT_MOVE_RUN - 1) of tile i: its first cell in grid coordinates and how many of its cells lie in the box (0: none)
VRT_DEV int move_tile_run(const MovePlan& p, int i, int r, int& x, int& y, int& z) {
    const int c[3] = {i / (p.tiles[2] * p.tiles[1]), i / p.tiles[2] % p.tiles[1], i % p.tiles[2]};
    const int runs_z = VRT_MOVE_TZ / VRT_MOVE_RUN;
    x = p.dst.lo[0] + c[0] * VRT_MOVE_TX + r / (runs_z * VRT_MOVE_TY);
    y = p.dst.lo[1] + c[1] * VRT_MOVE_TY + r / runs_z % VRT_MOVE_TY;
    z = p.dst.lo[2] + c[2] * VRT_MOVE_TZ + r % runs_z * VRT_MOVE_RUN;
    if (x >= p.dst.hi[0] || y >= p.dst.hi[1] || z >= p.dst.hi[2]) return 0;
    return p.dst.hi[2] - z < VRT_MOVE_RUN ? p.dst.hi[2] - z : VRT_MOVE_RUN;
}
// what a thread's cells add to the record; folded over the wave, then over the workgroup, then one atomic a word (k_move_dst)
struct MoveTally { int lo[3], hi[3]; unsigned written, blocked; };
VRT_DEV MoveTally move_tally_none() { return MoveTally{{0x7fffffff, 0x7fffffff, 0x7fffffff}, {(int)0x80000000, (int)0x80000000, (int)0x80000000}, 0u, 0u}; }
// One run of the destination box: the map once, then the z step.  BUILD: the cells' bytes into the destination box's arrays (go: move_go
// of the count pass's sum); else the count pass, which takes go = true -- what VRT_MOVE_IF_FREE withholds is taken off the record at the end
// (move_result).  mat, rgb: the grid's arrays; snap: the source box's words.
template <bool BUILD>
VRT_DEV void move_dst_run(const MovePlan& p, bool go, int x, int y, int z, int n, const int8_t* mat, const uint8_t* rgb, const uint32_t* snap, int8_t* box_mat,
                          uint8_t* box_rgb, MoveTally& tally) {
    long long S[3];
    move_map(p, x, y, z, S);
    const int ny = p.dst.hi[1] - p.dst.lo[1], nz = p.dst.hi[2] - p.dst.lo[2];
    int i = ((x - p.dst.lo[0]) * ny + (y - p.dst.lo[1])) * nz + (z - p.dst.lo[2]);
    int g = edit_grid_index(p.G, x, y, z);
    for (int k = 0; k < n; k++, z++, i++, g++) {
        const int from = move_source(p, S), own = move_src_index(p, x, y, z);
        const MoveCell o = move_dst_cell(p.flags, go, from < 0 ? 0u : snap[from], own < 0 ? 0u : snap[own], mat[g], rgb + 3 * (size_t)g);
        if (BUILD) {
            box_mat[i] = o.mat;
            for (int ch = 0; ch < 3; ch++) box_rgb[3 * (size_t)i + ch] = o.rgb[ch];
        } else {
            tally.blocked += o.blocked ? 1u : 0u;
            if (o.written) {
                tally.written++;
                const int c[3] = {x, y, z};
                for (int a = 0; a < 3; a++) { tally.lo[a] = c[a] < tally.lo[a] ? c[a] : tally.lo[a]; tally.hi[a] = c[a] > tally.hi[a] ? c[a] : tally.hi[a]; }
            }
        }
        move_step_z(p, S);
    }
}
// cell i of the source box into the source box's arrays
VRT_DEV void move_src_build(const MovePlan& p, bool go, int i, const int8_t* mat, const uint8_t* rgb, const uint32_t* snap, int8_t* box_mat, uint8_t* box_rgb) {
    int x, y, z;
    edit_box_voxel(p.src, i, x, y, z);
    const int g = edit_grid_index(p.G, x, y, z);
    move_src_cell(p.flags, go, snap[i], mat[g], rgb + 3 * (size_t)g, box_mat[i], box_rgb + 3 * (size_t)i);
}

// ---- the record -------------------------------------------------------------------------------------------------------------------------
VRT_DEV void move_record_begin(MoveRecord& r) {
    for (int a = 0; a < 3; a++) { r.lo[a] = 0x7fffffff; r.hi[a] = (int)0x80000000; }
    r.written = r.blocked = r.erased = 0ULL;
}
// The caller's record from the device's: the box half-open, zero when nothing was written; under VRT_MOVE_IF_FREE with a blocked cell
// nothing was written or erased.  out: lo[3], hi[3], written, blocked, erased as vrt_move_result holds them.
VRT_DEV void move_result(unsigned flags, const MoveRecord& r, int out_lo[3], int out_hi[3], long long& written, long long& blocked, long long& erased) {
    const bool go = move_go(flags, r.blocked);
    written = go ? (long long)r.written : 0LL;
    erased = go ? (long long)r.erased : 0LL;
    blocked = (long long)r.blocked;
    for (int a = 0; a < 3; a++) { out_lo[a] = written ? r.lo[a] : 0; out_hi[a] = written ? r.hi[a] + 1 : 0; }
}

// ---- the scratch (a buffer of the context's own): the snapshot words, the box arrays of the larger box, the record, the staged selection --
struct MoveLayout { size_t mat_at, rgb_at, record_at, select_at, bytes; };
VRT_DEV MoveLayout move_layout(size_t n_src, size_t n_dst, bool staged_select) {
    const size_t n_max = n_src > n_dst ? n_src : n_dst;
    MoveLayout l;
    l.mat_at = (4 * n_src + 255) & ~(size_t)255;
    l.rgb_at = (l.mat_at + n_max + 255) & ~(size_t)255;
    l.record_at = (l.rgb_at + 3 * n_max + 255) & ~(size_t)255;
    l.select_at = l.record_at + 256;
    l.bytes = l.select_at + (staged_select ? 4 * n_src : 0);
    return l;
}

}  // namespace vrt
