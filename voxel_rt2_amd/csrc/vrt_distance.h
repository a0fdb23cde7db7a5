// vrt_distance.h -- the arithmetic of vrt_distance_field: the exact squared Euclidean distance from every cell of a box to the nearest
// TARGET cell of the grid (solid, or with VRT_DIST_TO_EMPTY non-solid), bounded by max_d2, and which target that is.  Plain functions
// over plain values: the k_dist_* kernels (vrt_scene_kernels.hip) are loops over them, one output element per call, and
// tests/emul/distance_emul.cpp runs the same loops on a machine without a GPU (tests/test_distance_host.py).
//
// THE TRANSFORM is separable: (x-t_x)^2 + (y-t_y)^2 + (z-t_z)^2 is minimised axis by axis, z first, then y, then x.
//   pass z: A[x][y][z] = min over z' of (z-z')^2 for targets (x, y, z')                        and cz = the z' chosen
//   pass y: B[x][y][z] = min over y' of A[x][y'][z] + (y-y')^2                                   and cy = the y' chosen
//   pass x: D[x][y][z] = min over x' of B[x'][y][z] + (x-x')^2                                   and x' itself
// Every value is CAPPED at cap = max_d2 + 1 ("no target near enough"): a pass's result never exceeds its own input (j = 0), so by
// induction everything stays <= cap, and cap + 255^2 < 2^19.  A result <= max_d2 is a sum of uncapped terms only, so it is exact;
// a result > max_d2 becomes VRT_DIST_FAR.
// THE GROWN BOX.  R = floor(sqrt(max_d2)).  A target within max_d2 of a box cell differs from it by at most R on every axis, so it lies
// in the box grown by R on every side (clipped to the grid: only cells inside the grid exist).  Pass z runs over the lines (x, y) of
// the grown box and yields the box's z range; pass y over (x of the grown box, z of the box) and yields the box's y range; pass x
// yields the box.  Nothing outside the grown box is read.
// THE LINE PASS is the pruned scan: best = f[i]; for j = 1, 2, ... while j^2 can still beat best (j^2 < best; j^2 <= best where a tie
// still matters for `nearest`), f[i-j] + j^2 and f[i+j] + j^2 are compared against best.  A line is at most 256 entries.
// THE TIE RULE.  Among the targets that attain D the smallest linear index (t_x G + t_y) G + t_z wins: lexicographic in (x, y, z).
// Pass x keeps the smallest x' among the minimisers (dist_better on (value, coordinate)); B[x'] was itself attained at the smallest
// y' (pass y), and A[x'][y'] at the smallest z' (pass z): dist_assemble reads cy at (x', y, z), then cz at (x', y', z).
#pragma once
#include "vrt_edit.h"

namespace vrt {

#define VRT_DIST_FAR_VALUE 0x7fffffff   // VRT_DIST_FAR of include/vrt_api.h
#define VRT_DIST_LINE 256               // entries of a line at most (grid_res <= 256)

VRT_DEV int dist_isqrt(int v) {   // floor(sqrt(v)), v <= 195075: at most 441 steps, once a call
    int r = 0;
    while ((r + 1) * (r + 1) <= v) r++;
    return r;
}

struct DistBox {
    EditBox box, grown;   // the cells asked for; the cells read
    int max_d2, cap;      // cap = max_d2 + 1
    int to_empty;         // targets are the non-solid cells
};
VRT_DEV DistBox dist_plan_box(const EditBox& b, int G, int max_d2, uint32_t flags) {
    DistBox p;
    const int R = dist_isqrt(max_d2);
    p.box = b;
    for (int a = 0; a < 3; a++) {
        p.grown.lo[a] = b.lo[a] - R < 0 ? 0 : b.lo[a] - R;
        p.grown.hi[a] = b.hi[a] + R > G ? G : b.hi[a] + R;
    }
    p.max_d2 = max_d2;
    p.cap = max_d2 + 1;
    p.to_empty = (flags & 1u) != 0u;   // VRT_DIST_TO_EMPTY
    return p;
}
VRT_DEV int dist_len(const EditBox& b, int a) { return b.hi[a] - b.lo[a]; }

// SOLID is the fine occupancy bit: material byte > 0, signed
VRT_DEV bool dist_target(int8_t m, int to_empty) { return (m > 0) != (to_empty != 0); }
VRT_DEV int dist_seed(int8_t m, const DistBox& p) { return dist_target(m, p.to_empty) ? 0 : p.cap; }

// (value, coordinate) pairs: the smaller value, among equal values the smaller coordinate
struct DistPick { int v, c; };
VRT_DEV bool dist_better(int v, int c, int bv, int bc) { return v < bv || (v == bv && c < bc); }

// One output element of a line pass: entry i of the line f[0 .. n) (entry k at f[k * stride]; coordinate base + k).
// TIES: keep the smallest coordinate among equal values, which costs the scan the steps with j^2 == best.
template <bool TIES>
VRT_DEV DistPick dist_line_element(const int* f, int stride, int n, int i, int base) {
    DistPick best;
    best.v = f[i * stride];
    best.c = base + i;
    for (int j = 1; TIES ? j * j <= best.v : j * j < best.v; j++) {
        const int lo = i - j, hi = i + j, q = j * j;
        if (lo < 0 && hi >= n) break;
        if (lo >= 0) {
            const int v = f[lo * stride] + q;
            if (TIES ? dist_better(v, base + lo, best.v, best.c) : v < best.v) { best.v = v; best.c = base + lo; }
        }
        if (hi < n) {
            const int v = f[hi * stride] + q;
            if (TIES ? dist_better(v, base + hi, best.v, best.c) : v < best.v) { best.v = v; best.c = base + hi; }
        }
    }
    return best;
}

// Where things sit in the scratch arrays (C order, z fastest; gx, gy: the grown box's extent, by, bz: the box's):
//   A, cz: [gx][gy][bz]     B, cy: [gx][by][bz]     d2, nearest: [bx][by][bz]
VRT_DEV size_t dist_a_index(const DistBox& p, int xi, int yi, int zi) { return ((size_t)xi * dist_len(p.grown, 1) + yi) * dist_len(p.box, 2) + zi; }
VRT_DEV size_t dist_b_index(const DistBox& p, int xi, int yo, int zi) { return ((size_t)xi * dist_len(p.box, 1) + yo) * dist_len(p.box, 2) + zi; }

// the final mapping
VRT_DEV int dist_final(int v, int max_d2) { return v <= max_d2 ? v : VRT_DIST_FAR_VALUE; }
// `nearest` of box cell (., yo, zi) whose pass x chose x' = xq (a grid coordinate) with a value <= max_d2
VRT_DEV int dist_assemble(const DistBox& p, int G, int xq, int yo, int zi, const uint8_t* cy, const uint8_t* cz) {
    const int xi = xq - p.grown.lo[0];
    const int yq = cy[dist_b_index(p, xi, yo, zi)];
    const int zq = cz[dist_a_index(p, xi, yq - p.grown.lo[1], zi)];
    return edit_grid_index(G, xq, yq, zq);
}

}  // namespace vrt
