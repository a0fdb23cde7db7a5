// vrt_sweep.h -- vrt_sweep_boxes: caller-supplied axis-aligned boxes moved through the prepared scene.  Which boxes are tested at all,
// one cell's test, the floor's, the order candidates are ranked by, the cells a box can meet at all, and one lane's share of a box
// (sweep_lane).  Plain functions over plain values, in the style of vrt_cast.h / vrt_edit.h: k_sweep_boxes (vrt_query_kernels.hip) gives a box
// to a wave of 64 lanes and merges their candidates with a cross-lane minimum, and tests/emul/sweep_emul.cpp runs the same lanes one
// after the other on a machine without a GPU (tests/test_sweep_boxes_host.py).
//
// The answer is specified in include/vrt_api.h as a minimum over ALL solid cells of the grid; the code here visits the cells of a
// candidate region only.  Two arguments carry that.
//
// THE REGION IS A SUPERSET (sweep_region).  Let a cell c be accepted by the per-cell test: it is met (enter < exit, exit > 0) and either
// enter < 0 (a start overlap) or 0 <= enter < t_max (a contact that counts).  Put tau = max(enter, 0): then 0 <= tau < t_max, and on every
// axis e_a <= enter <= tau and x_a >= exit > tau.  Take an axis with move_a > 0 (move_a < 0 is its mirror image).  e_a is the rounded
// quotient of d = fl(p(c_a) - hi_a) by move_a, and rounding is monotone, so e_a <= tau gives d <= tau * move_a * (1 + 2^-23) + (a
// subnormal's worth of move_a): the box's upper face at tau, hi_a + tau * move_a, is no lower than p(c_a) - delta.  What delta holds: the
// rounding of d -- |hi_a| <= VRT_SWEEP_MAX_COORD = 64 and |p| <= 1, so half an ulp of 65, 2^-18 -- and 2^-23 of a product that is at
// most |d| <= 66 where it matters (a larger product has carried the face past the plane by itself): together below 2^-16, where a cell
// is 2^-6 or 2^-7 wide.  The same for x_a > tau: the lower face at tau is below p(c_a + 1) + delta.  The box's faces at tau lie between
// their positions at t = 0 and at t = t_max (it moves monotonically and tau < t_max), which is the hull; the hull's own arithmetic (one
// product, one sum, of values clamped to the grid's neighbourhood) errs by less than 2^-16 again.  So cell c's slab [p(c_a), p(c_a + 1)]
// comes within 2^-15 of the hull on every axis with a non-zero move, and so lies inside the hull WIDENED BY ONE CELL; on an axis with
// move_a == 0 the test's own comparisons (lo_a < p(c_a + 1) && hi_a > p(c_a)) are exact and say that the slab overlaps the hull itself.
// Without the bound on the coordinates the rounding of d grows with |hi_a| and at 2^17 reaches a cell: that is what VRT_SWEEP_MAX_COORD
// is for.  The region is also clipped against the grid (only cells inside it exist) and against the scene's culling box (sc.cull: the
// bounds of the solid bricks, grown -- every solid cell lies inside it).
//
// EVERY BOX ENDS.  The region is clamped to the grid before anything is counted, so sweep_lane's loop runs over at most (G / 4)^3 bricks
// -- 32 768 or 262 144 -- shared among the lanes, and the loop over a brick's set bits clears one bit per turn: at most 64 turns.  No
// field of the box enters a loop bound except through that clamp; a subnormal, huge or zero move only changes what the divisions give.
#pragma once
#include "../../include/vrt_api.h"
#include "vrt_trace.h"

namespace vrt {

VRT_DEV bool sweep_finite(float x) { return (dm_f2u(x) & 0x7f800000u) != 0x7f800000u; }   // neither inf nor NaN

// The boxes that are tested (include/vrt_api.h).  `reserved` is checked here too: the host path has refused such a box before anything
// ran, on the device path it gets the miss record.
VRT_DEV bool sweep_box_valid(const vrt_box_sweep& b) {
    for (int a = 0; a < 3; a++) {
        if (!sweep_finite(b.lo[a]) || !sweep_finite(b.hi[a]) || !sweep_finite(b.move[a])) return false;
        if (b.lo[a] > b.hi[a]) return false;
        if (b.lo[a] < -VRT_SWEEP_MAX_COORD || b.hi[a] > VRT_SWEEP_MAX_COORD) return false;
    }
    if (b.reserved != 0u) return false;
    return b.t_max > 0.0f;   // (false for a NaN; +inf passes)
}

// plane k of the grid: exact in binary32 for dx = 2^-6 and 2^-7
VRT_DEV float sweep_plane(int k, float dx) { return (float)k * dx - 1.0f; }

// The per-cell test on a SPAN of cells [c0, c1] per axis, i.e. on the slab [p(c0_a), p(c1_a + 1)]: a cell is the span c0 == c1, and a
// 4x4x4 brick is a span too.  Returns whether the span is met; enter / exit as the header defines them, axis = the lowest a with
// e_a == enter.  Every e_a and x_a is monotone in the planes it is formed from (a difference and a quotient, both correctly rounded), so a
// span's enter is a lower bound of the enter of every cell inside it and its exit an upper bound of theirs: a span that is not met holds
// no cell that is, and no cell of it is entered before the span is -- what sweep_lane's pruning rests on, bit for bit.
VRT_DEV bool sweep_span(const vrt_box_sweep& b, float dx, const int* c0, const int* c1, float& enter, float& exit, int& axis) {
    float e[3], x[3];
    for (int a = 0; a < 3; a++) {
        const float plo = sweep_plane(c0[a], dx), phi = sweep_plane(c1[a] + 1, dx), m = b.move[a];
        if (m > 0.0f) { e[a] = (plo - b.hi[a]) / m; x[a] = (phi - b.lo[a]) / m; }
        else if (m < 0.0f) { e[a] = (phi - b.lo[a]) / m; x[a] = (plo - b.hi[a]) / m; }
        else {
            if (!(b.lo[a] < phi && b.hi[a] > plo)) return false;
            e[a] = -DM_INF; x[a] = DM_INF;
        }
    }
    enter = dm_max(dm_max(e[0], e[1]), e[2]);
    exit = dm_min(dm_min(x[0], x[1]), x[2]);
    axis = e[0] == enter ? 0 : e[1] == enter ? 1 : 2;
    return enter < exit && exit > 0.0f;
}

// The total order on candidates -- (start overlap first, then t by its bits, then the linear index; the floor before every cell) -- as
// one 64-bit key whose unsigned order it is: bit 57 clear for a start overlap, bits 25..56 the bits of t (t >= +0, so they order as t
// does; 0 for a start overlap), bits 0..24 the cell's linear index (x * G + y) * G + z plus one, 0 for the floor.  Nothing met: all ones.
typedef unsigned long long SweepKey;
#define VRT_SWEEP_KEY_MISS (~0ULL)
VRT_DEV SweepKey sweep_key(bool start, float t, int index_plus_one) {
    return ((SweepKey)(start ? 0u : 1u) << 57) | ((SweepKey)(start ? 0u : dm_f2u(t)) << 25) | (SweepKey)(unsigned)index_plus_one;
}
VRT_DEV SweepKey sweep_better(SweepKey a, SweepKey b) { return a < b ? a : b; }
VRT_DEV bool sweep_key_start(SweepKey k) { return ((k >> 57) & 1ULL) == 0ULL; }
VRT_DEV float sweep_key_t(SweepKey k) { return dm_u2f((uint32_t)(k >> 25)); }
VRT_DEV int sweep_key_index(SweepKey k) { return (int)(k & 0x1ffffffULL) - 1; }   // -1: the floor

// one solid cell's candidate
VRT_DEV SweepKey sweep_cell_key(const vrt_box_sweep& b, int G, float dx, int x, int y, int z) {
    const int c[3] = {x, y, z};
    float enter, exit;
    int axis;
    if (!sweep_span(b, dx, c, c, enter, exit, axis)) return VRT_SWEEP_KEY_MISS;
    const int index = (x * G + y) * G + z;
    if (enter < 0.0f) return sweep_key(true, 0.0f, index + 1);
    const float t = enter + 0.0f;   // (-0 becomes +0)
    return t < b.t_max ? sweep_key(false, t, index + 1) : VRT_SWEEP_KEY_MISS;
}
// the floor's: the infinite plane y = floor_height, solid below
VRT_DEV SweepKey sweep_floor_key(const vrt_box_sweep& b, float floor_height) {
    if (b.flags & VRT_SWEEP_NO_FLOOR) return VRT_SWEEP_KEY_MISS;
    if (b.lo[1] < floor_height) return sweep_key(true, 0.0f, 0);
    if (b.move[1] < 0.0f) {
        const float t = (floor_height - b.lo[1]) / b.move[1] + 0.0f;
        if (t < b.t_max) return sweep_key(false, t, 0);
    }
    return VRT_SWEEP_KEY_MISS;
}

// The candidate region, in cells, both ends included (see the head of this file): the hull of the box at t = 0 and at t = t_max, widened
// by one cell, clipped against the grid and against the culling box (cull[0..2] / cull[3..5], voxel units).
struct SweepRegion { int lo[3], hi[3]; bool empty; };
VRT_DEV SweepRegion sweep_region(const vrt_box_sweep& b, int G, const float* cull) {
    SweepRegion r;
    r.empty = false;
    const float half = (float)(G / 2), res = (float)G;
    for (int a = 0; a < 3; a++) {
        const float shift = b.move[a] == 0.0f ? 0.0f : b.t_max * b.move[a];   // (inf * 0 would be a NaN; +-inf for an unbounded sweep)
        const float h0 = dm_clamp(dm_min(b.lo[a], b.lo[a] + shift), -2.0f, 2.0f), h1 = dm_clamp(dm_max(b.hi[a], b.hi[a] + shift), -2.0f, 2.0f);
        int c0 = (int)dm_floor((h0 + 1.0f) * half) - 1, c1 = (int)dm_floor((h1 + 1.0f) * half) + 1;
        const int k0 = (int)dm_clamp(cull[a], 0.0f, res), k1 = (int)dm_clamp(cull[3 + a], 0.0f, res) - 1;   // (a grid without solids: lo > hi)
        c0 = c0 < 0 ? 0 : c0;
        c1 = c1 > G - 1 ? G - 1 : c1;
        r.lo[a] = c0 < k0 ? k0 : c0;
        r.hi[a] = c1 > k1 ? k1 : c1;
        if (r.lo[a] > r.hi[a]) r.empty = true;
    }
    return r;
}

// One lane's share of a box: bricks lane, lane + lanes, ... of the region's 4x4x4 bricks, x running fastest (neighbouring lanes load
// neighbouring l0 words), starting from `best` (the floor's candidate, or nothing).  A brick whose l1 bit is clear is not loaded.
// prune: a brick that is not met as a span, or is entered later than the lane's best (or not before t_max), is skipped -- by sweep_span's
// monotonicity none of its cells can be met, overlap at the start (their enter is >= the span's > 0) or come before or level with the
// best.  l0 / l1: the pyramid's two finest levels (words of a level of n^3: (bz * n + by) * n + bx).
VRT_DEV SweepKey sweep_lane(const vrt_box_sweep& b, const SweepRegion& r, int G, const unsigned long long* l0, const unsigned long long* l1,
                            SweepKey best, int lane, int lanes, bool prune) {
    const float dx = 2.0f / (float)G;
    const int n0 = G >> 2, n1 = G >> 4;
    const int b0[3] = {r.lo[0] >> 2, r.lo[1] >> 2, r.lo[2] >> 2};
    const int nb[3] = {(r.hi[0] >> 2) - b0[0] + 1, (r.hi[1] >> 2) - b0[1] + 1, (r.hi[2] >> 2) - b0[2] + 1};
    const int total = nb[0] * nb[1] * nb[2];   // at most (G / 4)^3
    for (int j = lane; j < total; j += lanes) {
        const int bx = b0[0] + j % nb[0], by = b0[1] + (j / nb[0]) % nb[1], bz = b0[2] + j / (nb[0] * nb[1]);
        const unsigned long long w1 = l1[((bz >> 2) * n1 + (by >> 2)) * n1 + (bx >> 2)];
        if (!((w1 >> brick_bit(bx, by, bz)) & 1ULL)) continue;
        unsigned long long w = l0[(bz * n0 + by) * n0 + bx];
        if (prune && w != 0ULL) {
            const int c0[3] = {bx * 4, by * 4, bz * 4}, c1[3] = {bx * 4 + 3, by * 4 + 3, bz * 4 + 3};
            float enter, exit;
            int axis;
            if (!sweep_span(b, dx, c0, c1, enter, exit, axis)) continue;
            if (best == VRT_SWEEP_KEY_MISS ? !(enter < b.t_max) : enter > sweep_key_t(best)) continue;
        }
        while (w != 0ULL) {
            const int bit = __builtin_ctzll(w);
            w &= w - 1ULL;
            const int x = bx * 4 + (bit & 3), y = by * 4 + ((bit >> 2) & 3), z = bz * 4 + (bit >> 4);
            if (x < r.lo[0] || x > r.hi[0] || y < r.lo[1] || y > r.hi[1] || z < r.lo[2] || z > r.hi[2]) continue;   // outside the region
            best = sweep_better(best, sweep_cell_key(b, G, dx, x, y, z));
        }
    }
    return best;
}

// nothing met before t_max
VRT_DEV void sweep_miss(vrt_sweep_hit& h) {
    h.t = DM_INF;
    h.kind = VRT_SWEEP_MISS;
    for (int a = 0; a < 3; a++) { h.cell[a] = -1; h.normal[a] = 0.0f; }
}
// The record of the winning candidate.  A contact's axis is not part of the key: the winner's cell test is run once more for it.
VRT_DEV void sweep_record(SweepKey k, const vrt_box_sweep& b, int G, vrt_sweep_hit& h) {
    sweep_miss(h);
    if (k == VRT_SWEEP_KEY_MISS) return;
    const int index = sweep_key_index(k);
    const int c[3] = {index < 0 ? -1 : index / (G * G), index < 0 ? -1 : (index / G) % G, index < 0 ? -1 : index % G};
    for (int a = 0; a < 3; a++) h.cell[a] = c[a];
    if (sweep_key_start(k)) { h.t = 0.0f; h.kind = VRT_SWEEP_START; return; }
    h.t = sweep_key_t(k);
    if (index < 0) { h.kind = VRT_SWEEP_FLOOR; h.normal[1] = 1.0f; return; }
    h.kind = VRT_SWEEP_VOXEL;
    float enter, exit;
    int axis = 0;
    sweep_span(b, 2.0f / (float)G, c, c, enter, exit, axis);
    for (int a = 0; a < 3; a++) if (a == axis) h.normal[a] = b.move[a] > 0.0f ? -1.0f : 1.0f;   // (no indexing by `axis`: the records stay in registers)
}

// What a box starts from before any cell is looked at: nothing for an invalid box (`walk` false: it gets the miss record), else the
// floor's candidate; a floor overlap at the start cannot be beaten (key 0), so no cell is looked at either.
VRT_DEV SweepKey sweep_begin(const vrt_box_sweep& b, float floor_height, bool& walk) {
    walk = false;
    if (!sweep_box_valid(b)) return VRT_SWEEP_KEY_MISS;
    const SweepKey k = sweep_floor_key(b, floor_height);
    walk = k != 0ULL;
    return k;
}

}  // namespace vrt
