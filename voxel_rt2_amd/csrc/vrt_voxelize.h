// vrt_voxelize.h -- vrt_voxelize_triangles: caller-supplied triangles voxelised into a box of a prepared grid.  The snap of a world
// coordinate to 64ths of a voxel, which triangles are tested at all, a triangle's set-up (edges, the thirteen axes, its projected
// interval on each), the cube test at any power-of-two cell edge, the cells a triangle can cover at all, the work items of a triangle
// and one lane's share of an item, and one voxel of the resolve.  Plain functions over plain values, in the style of vrt_edit.h /
// vrt_cast.h / vrt_sweep.h: the k_vox_* kernels (vrt_scene_kernels.hip) are loops over them, and tests/emul/voxelize_emul.cpp runs the same
// loops on a machine without a GPU (tests/test_voxelize_host.py).
//
// NO FLOAT SURVIVES THE SNAP.  include/vrt_api.h defines coverage on the snapped integer vertices, and everything here after vox_snap is
// exact integer arithmetic, so there is nothing to round and nothing a compiler could contract: the device and the host build agree
// because both are right.
//
// HEADROOM.  |w| <= VRT_TRI_MAX_COORD = 8 gives |s| <= (8 + 1) * 128 * 64 = 73 728 < 2^17 at grid_res 256.  Edge components are
// differences of two of those, < 2^18; a component of the normal e0 x e1 is a difference of two products of those, < 2^37; a component
// of e_i x axis_a is an edge component or 0.  A projection n . p has three terms with |p_a| < 2^17 (a vertex, or a corner of a cell of
// the grid: at most 64 * 256 = 2^14): below 3 * 2^37 * 2^17 < 2^56 on the normal, below 2 * 2^18 * 2^17 = 2^36 on the nine cross axes.
// int64 never overflows (tests/test_voxelize_host.py runs the extreme triangle against unbounded integers).  On the cross axes the dot
// product with a CELL INDEX (< 2^9) stays below 2^28 and is formed in int32: 64-bit multiplies are not cheap on CDNA.
//
// THE TEST IS COMPLETE FOR DEGENERATE HULLS.  The separating-axis theorem for two convex polytopes asks for the face normals of both
// and the cross products of their edge directions.  A proper triangle and a cube: 3 + 1 + 9 axes.  A segment (three collinear
// vertices, two of which may coincide) has no face, its edges are all parallel to its direction d or zero, so the nine cross axes hold
// d x axis_a (the other candidates), and the zero normal separates nothing (both intervals project to 0): the test is the segment /
// box test.  A point has zero edges throughout: what is left is the three cube normals, which is the point-in-closed-box test.  A zero
// axis never separates, so it can only be superfluous.
#pragma once
#include <cmath>
#include "../../include/vrt_api.h"
#include "vrt_edit.h"

namespace vrt {

// ---- the snap and the gate --------------------------------------------------------------------------------------------------------
// u = (w + 1) * (G / 2) in binary32 -- a sum and a product, nothing to contract -- then round-half-even of u * 64 (exact: a power of
// two).  The grid plane p(k) = k * dx - 1 is exact in binary32, p(k) + 1 = k * dx and (k * dx) * (G / 2) = k are exact too: s = 64 k.
VRT_DEV int32_t vox_snap(float w, int G) {
    const float u = (w + 1.0f) * (float)(G / 2);
    return (int32_t)rintf(u * 64.0f);
}
VRT_DEV bool vox_coord_ok(float w) {   // finite and inside [-VRT_TRI_MAX_COORD, VRT_TRI_MAX_COORD] (false for a NaN)
    return w >= -VRT_TRI_MAX_COORD && w <= VRT_TRI_MAX_COORD;
}
// The triangles that are voxelised (include/vrt_api.h).  The reserved words are checked here too: the host path has refused such a
// triangle before anything ran, on the device path it is skipped and counted.
VRT_DEV bool vox_tri_valid(const vrt_triangle& t) {
    for (int a = 0; a < 3; a++) if (!vox_coord_ok(t.v0[a]) || !vox_coord_ok(t.v1[a]) || !vox_coord_ok(t.v2[a])) return false;
    return t.reserved0 == 0u && t.reserved1 == 0u;
}

// ---- the set-up ---------------------------------------------------------------------------------------------------------------------
// Everything about a triangle that does not depend on the cell.  For an axis n the triangle projects to [min, max] of n . v_i and the
// cube with lower corner m = E * c and edge E to E * [n . c + neg, n . c + pos] with neg / pos the sums of n's negative / positive
// components: the per-cell test is a dot product with the cell index plus constants.
struct VoxTri {
    int32_t v[3][3];              // the snapped vertices
    int32_t bmin[3], bmax[3];     // their bounds: the three cube normals
    int64_t nn[3], nmin, nmax, nneg, npos;                  // the triangle's normal e0 x e1
    int32_t cn[9][3];             // e_i x axis_a at [3 * i + a]
    int64_t cmin[9], cmax[9];
    int32_t cneg[9], cpos[9];
};
VRT_DEV int64_t vox_min3(int64_t a, int64_t b, int64_t c) { const int64_t m = a < b ? a : b; return m < c ? m : c; }
VRT_DEV int64_t vox_max3(int64_t a, int64_t b, int64_t c) { const int64_t m = a > b ? a : b; return m > c ? m : c; }
VRT_DEV void vox_snap_tri(const vrt_triangle& t, int G, VoxTri& s) {
    for (int a = 0; a < 3; a++) {
        s.v[0][a] = vox_snap(t.v0[a], G); s.v[1][a] = vox_snap(t.v1[a], G); s.v[2][a] = vox_snap(t.v2[a], G);
        s.bmin[a] = (int32_t)vox_min3(s.v[0][a], s.v[1][a], s.v[2][a]);
        s.bmax[a] = (int32_t)vox_max3(s.v[0][a], s.v[1][a], s.v[2][a]);
    }
}
// the axes of a snapped triangle (vox_snap_tri has run)
VRT_DEV void vox_axes(VoxTri& s) {
    int32_t e[3][3];
    for (int a = 0; a < 3; a++) { e[0][a] = s.v[1][a] - s.v[0][a]; e[1][a] = s.v[2][a] - s.v[1][a]; e[2][a] = s.v[0][a] - s.v[2][a]; }
    s.nn[0] = (int64_t)e[0][1] * e[1][2] - (int64_t)e[0][2] * e[1][1];
    s.nn[1] = (int64_t)e[0][2] * e[1][0] - (int64_t)e[0][0] * e[1][2];
    s.nn[2] = (int64_t)e[0][0] * e[1][1] - (int64_t)e[0][1] * e[1][0];
    // (the three vertices project to the same value on the normal of a proper triangle: min == max; kept general for the segment)
    int64_t p[3];
    for (int i = 0; i < 3; i++) p[i] = s.nn[0] * s.v[i][0] + s.nn[1] * s.v[i][1] + s.nn[2] * s.v[i][2];
    s.nmin = vox_min3(p[0], p[1], p[2]);
    s.nmax = vox_max3(p[0], p[1], p[2]);
    s.nneg = s.npos = 0;
    for (int a = 0; a < 3; a++) { if (s.nn[a] < 0) s.nneg += s.nn[a]; else s.npos += s.nn[a]; }
    for (int i = 0; i < 3; i++)
        for (int a = 0; a < 3; a++) {
            const int b = (a + 1) % 3, c = (a + 2) % 3, k = 3 * i + a;
            // e x axis_a: component b is e_c, component c is -e_b, component a is 0
            s.cn[k][a] = 0; s.cn[k][b] = e[i][c]; s.cn[k][c] = -e[i][b];
            for (int j = 0; j < 3; j++) p[j] = (int64_t)s.cn[k][b] * s.v[j][b] + (int64_t)s.cn[k][c] * s.v[j][c];
            s.cmin[k] = vox_min3(p[0], p[1], p[2]);
            s.cmax[k] = vox_max3(p[0], p[1], p[2]);
            s.cneg[k] = (s.cn[k][b] < 0 ? s.cn[k][b] : 0) + (s.cn[k][c] < 0 ? s.cn[k][c] : 0);
            s.cpos[k] = (s.cn[k][b] > 0 ? s.cn[k][b] : 0) + (s.cn[k][c] > 0 ? s.cn[k][c] : 0);
        }
}
VRT_DEV void vox_setup(const vrt_triangle& t, int G, VoxTri& s) { vox_snap_tri(t, G, s); vox_axes(s); }

// ---- the cube test ------------------------------------------------------------------------------------------------------------------
// Does the closed triangle share a point with the closed cube of edge (1 << shift) voxels whose index at that level is (cx, cy, cz),
// i.e. [E c_a, E c_a + E]^3 with E = 64 << shift?  shift 0: a voxel (the COVERS of include/vrt_api.h), 2: a 4^3 brick, 4: a 16^3 cell.
// Separated iff the projections are strictly apart on one of the thirteen axes.  A cube holds every smaller cube inside it, so a
// cube that is not met holds no voxel that is: what the rejection of bricks and 16^3 cells rests on.
VRT_DEV bool vox_cube(const VoxTri& s, int cx, int cy, int cz, int shift) {
    const int64_t E = (int64_t)64 << shift;
    const int c[3] = {cx, cy, cz};
    for (int a = 0; a < 3; a++) {
        const int64_t m = E * c[a];
        if (s.bmin[a] > m + E || s.bmax[a] < m) return false;
    }
    const int64_t d = s.nn[0] * cx + s.nn[1] * cy + s.nn[2] * cz;
    if (s.nmax < E * (d + s.nneg) || s.nmin > E * (d + s.npos)) return false;
    for (int k = 0; k < 9; k++) {
        const int32_t dk = s.cn[k][0] * cx + s.cn[k][1] * cy + s.cn[k][2] * cz;
        if (s.cmax[k] < E * (int64_t)(dk + s.cneg[k]) || s.cmin[k] > E * (int64_t)(dk + s.cpos[k])) return false;
    }
    return true;
}

// ---- the cells a triangle can cover at all ----------------------------------------------------------------------------------------
// The cells of edge (1 << shift) voxels that touch both the triangle's closed bounds and the clip box: n[a] cells from lo[a] per axis
// (EditCells, vrt_edit.h); n = 0 on every axis if there is none.  Cell c touches [bmin, bmax] iff E c <= bmax and E (c + 1) >= bmin,
// E = 64 << shift: c from ((bmin - 1) >> k) to (bmax >> k), k = 6 + shift (>> of a negative value is the arithmetic shift: floor).
VRT_DEV EditCells vox_cells(const VoxTri& s, const EditBox& clip, int shift) {
    EditCells r;
    bool empty = false;
    const int k = 6 + shift;
    for (int a = 0; a < 3; a++) {
        int lo = (s.bmin[a] - 1) >> k, hi = s.bmax[a] >> k;
        const int blo = clip.lo[a] >> shift, bhi = (clip.hi[a] - 1) >> shift;   // (the clip box is not empty: the caller checks)
        if (lo < blo) lo = blo;
        if (hi > bhi) hi = bhi;
        r.lo[a] = lo; r.n[a] = hi - lo + 1;
        if (hi < lo) empty = true;
    }
    if (empty) for (int a = 0; a < 3; a++) { r.lo[a] = 0; r.n[a] = 0; }
    return r;
}

// ---- work items ---------------------------------------------------------------------------------------------------------------------
// A triangle's work is cut into ITEMS: one 16^3 cell of vox_cells(shift 4) each, x running fastest (edit_cell).  A triangle spanning a
// 256^3 grid has 4096 of them and a wave takes one at a time, so no wave walks a large triangle alone; a triangle smaller than a 16^3
// cell has one to eight.  The set-up pass counts a batch's items and leaves one entry per triangle that has any, in the order of
// their first item, so that an item number is found by a binary search over `first`.
struct VoxEntry { unsigned long long first; uint32_t tri; uint32_t items; };   // tri: index within the batch
// items of triangle t clipped to `clip` (0: invalid, or nothing of it inside the box); valid reports the gate
VRT_DEV uint32_t vox_tri_items(const vrt_triangle& t, int G, const EditBox& clip, bool& valid) {
    valid = vox_tri_valid(t);
    if (!valid) return 0u;
    VoxTri s;
    vox_snap_tri(t, G, s);
    return (uint32_t)edit_cell_count(vox_cells(s, clip, 4));
}
// the entry that holds item g: the last with first <= g (n >= 1 entries, entries[0].first == 0 <= g)
VRT_DEV long long vox_find_entry(const VoxEntry* entries, long long n, unsigned long long g) {
    long long lo = 0, hi = n - 1;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (entries[mid].first <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}
VRT_DEV int vox_box_index(const EditBox& b, int x, int y, int z) {   // edit_box_voxel the other way round
    return ((x - b.lo[0]) * (b.hi[1] - b.lo[1]) + (y - b.lo[1])) * (b.hi[2] - b.lo[2]) + (z - b.lo[2]);
}
VRT_DEV bool vox_in_box(const EditBox& b, int x, int y, int z) {
    return x >= b.lo[0] && x < b.hi[0] && y >= b.lo[1] && y < b.hi[1] && z >= b.lo[2] && z < b.hi[2];
}
// One lane's share of an item, first half: does the lane's brick of the item's 16^3 cell (cx, cy, cz) -- bit x + 4 y + 16 z of the
// lane number, as in an l1 word -- need its voxels tried?  Inside the brick range of the triangle and the box, and met.
VRT_DEV bool vox_lane_brick(const VoxTri& s, const EditCells& bricks, int cx, int cy, int cz, int lane) {
    const int b[3] = {cx * 4 + (lane & 3), cy * 4 + ((lane >> 2) & 3), cz * 4 + (lane >> 4)};
    for (int a = 0; a < 3; a++) if (b[a] < bricks.lo[a] || b[a] >= bricks.lo[a] + bricks.n[a]) return false;
    return vox_cube(s, b[0], b[1], b[2], 2);
}
// Second half: the lane's voxel of brick `brick` (0 .. 63 within the 16^3 cell): -1, or the box-local index of a voxel the triangle
// covers -- the lane then raises owner[index] to the triangle's global number + 1.
VRT_DEV int vox_lane_voxel(const VoxTri& s, const EditBox& clip, int cx, int cy, int cz, int brick, int lane) {
    const int x = (cx * 4 + (brick & 3)) * 4 + (lane & 3), y = (cy * 4 + ((brick >> 2) & 3)) * 4 + ((lane >> 2) & 3), z = (cz * 4 + (brick >> 4)) * 4 + (lane >> 4);
    if (!vox_in_box(clip, x, y, z) || !vox_cube(s, x, y, z, 0)) return -1;
    return vox_box_index(clip, x, y, z);
}

// ---- the resolve ----------------------------------------------------------------------------------------------------------------------
// Voxel i of the box arrays from its owner word.  Owner o > base: triangle o - 1 (global number), which is tris[o - 1 - base] of the
// batch at hand, wrote it last: its payload.  Owner 0 and `final`: nobody did, the grid's stored voxel.  Otherwise (an owner of an
// earlier batch, whose own resolve has written the box arrays already; or owner 0 before the last batch) nothing.  Returns whether
// the voxel is WRITTEN (o != 0) -- counted and bounded by the last batch's resolve only.
VRT_DEV bool vox_resolve_voxel(const EditBox& b, int G, int i, const uint32_t* owner, unsigned long long base, const vrt_triangle* tris, bool final,
                               const int8_t* mat, const uint8_t* rgb, int8_t* box_mat, uint8_t* box_rgb) {
    const uint32_t o = owner[i];
    if ((unsigned long long)o > base) {
        const uint32_t p = tris[(unsigned long long)o - 1ULL - base].voxel;
        box_mat[i] = (int8_t)(uint8_t)(p >> 24);
        box_rgb[3 * i] = (uint8_t)p; box_rgb[3 * i + 1] = (uint8_t)(p >> 8); box_rgb[3 * i + 2] = (uint8_t)(p >> 16);
    } else if (o == 0u && final) {
        int x, y, z;
        edit_box_voxel(b, i, x, y, z);
        const int g = edit_grid_index(G, x, y, z);
        box_mat[i] = mat[g];
        for (int k = 0; k < 3; k++) box_rgb[3 * i + k] = rgb[3 * g + k];
    }
    return o != 0u;
}

}  // namespace vrt
