// move_emul.cpp -- TEST TOOLING: the loops of the k_move_* kernels (voxel_rt2_amd/csrc/vrt_scene_kernels.hip) and of vrt_move_voxels
// (vrt_scene_ops.hip) run on the host over the functions of voxel_rt2_amd/csrc/vrt_move.h: the same checks, the same tiles and runs, the
// same scratch layout (move_layout), pass by pass in the order the call queues them -- snapshot, count, the source box's arrays and their
// store, the destination box's arrays (built from the grid as the first store left it) and theirs.  Of launch_edit only the store of the
// box arrays into the grid's material and colour arrays is run here: what it derives from them is tests/emul/edit_emul.cpp's subject.
// tests/move.py compiles this with g++ and calls it through ctypes.
// -DMOVE_EMUL_MAIN: a stand-alone program (its own main, no Python) over a small generated grid -- what a sanitizer build runs.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/vrt_api.h"
#include "../../voxel_rt2_amd/csrc/vrt_move.h"

using namespace vrt;

namespace {
void store_box(int G, const EditBox& b, const int8_t* box_mat, const uint8_t* box_rgb, int8_t* mat, uint8_t* rgb) {   // k_edit_store's two arrays
    for (int i = 0; i < edit_box_voxels(b); i++) {
        int x, y, z;
        edit_box_voxel(b, i, x, y, z);
        const size_t g = (size_t)edit_grid_index(G, x, y, z);
        mat[g] = box_mat[i];
        for (int k = 0; k < 3; k++) rgb[3 * g + k] = box_rgb[3 * (size_t)i + k];
    }
}
}  // namespace

extern "C" {
long long move_emul_plan(long long n_src, long long n_dst, int staged) { return (long long)move_layout((size_t)n_src, (size_t)n_dst, staged != 0).bytes; }
void move_emul_tile(int* out) { out[0] = VRT_MOVE_TX; out[1] = VRT_MOVE_TY; out[2] = VRT_MOVE_TZ; out[3] = VRT_MOVE_RUN; }
// the full map of cell d and the source cell it names: S[3], s[3] (S >> 17)
void move_emul_map(const int* m, const long long* t, const int* d, long long* S, long long* s) {
    EditBox none{{0, 0, 0}, {0, 0, 0}};
    const MovePlan p = move_plan(none, none, m, t, 0, 0u, 256);
    move_map(p, d[0], d[1], d[2], S);
    for (int a = 0; a < 3; a++) s[a] = S[a] >> 17;
}
// S of the n cells of the z line from d on, by the z step: S[3 * n]
void move_emul_line(const int* m, const long long* t, const int* d, int n, long long* S) {
    EditBox none{{0, 0, 0}, {0, 0, 0}};
    const MovePlan p = move_plan(none, none, m, t, 0, 0u, 256);
    long long at[3];
    move_map(p, d[0], d[1], d[2], at);
    for (int k = 0; k < n; k++) {
        for (int a = 0; a < 3; a++) S[3 * k + a] = at[a];
        move_step_z(p, at);
    }
}
// vrt_move_voxels on host arrays: mat int8[G][G][G] and rgb uint8[G][G][G][3] are the stored voxels, edited in place; scratch: at least
// move_emul_plan bytes; staged: the selection is copied into the scratch first.  Returns vrt_move_voxels' code.
int move_emul_call(int G, int8_t* mat, uint8_t* rgb, const vrt_voxel_move* mv, const int* select, int staged, vrt_move_result* result, uint8_t* scratch) {
    if (!mat || !rgb || !mv || (G != 128 && G != 256)) return VRT_E_INVALID;
    if (staged != 0 && staged != 1) return VRT_E_INVALID;
    long long t[3];
    for (int a = 0; a < 3; a++) t[a] = (long long)mv->t[a];
    EditBox src, dst;
    for (int a = 0; a < 3; a++) { src.lo[a] = mv->src_lo[a]; src.hi[a] = mv->src_hi[a]; dst.lo[a] = mv->dst_lo[a]; dst.hi[a] = mv->dst_hi[a]; }
    if (!edit_box_valid(src, G) || !move_valid(mv->m, t, mv->flags, mv->reserved) || !edit_box_valid(dst, G)) return VRT_E_INVALID;
    if (result) memset(result, 0, sizeof(*result));
    const int n_src = edit_box_voxels(src), n_dst = edit_box_voxels(dst);
    if (n_src == 0) return VRT_OK;
    const MovePlan p = move_plan(src, dst, mv->m, t, mv->select_value, mv->flags, G);
    const MoveLayout l = move_layout((size_t)n_src, (size_t)n_dst, select && staged);
    uint32_t* snap = (uint32_t*)scratch;
    int8_t* box_mat = (int8_t*)(scratch + l.mat_at);
    uint8_t* box_rgb = scratch + l.rgb_at;
    MoveRecord* rec = (MoveRecord*)(scratch + l.record_at);
    if (select && staged) { memcpy(scratch + l.select_at, select, 4 * (size_t)n_src); select = (const int*)(scratch + l.select_at); }
    // k_move_begin, k_move_snapshot
    move_record_begin(*rec);
    for (int i = 0; i < n_src; i++) {
        snap[i] = move_snap_cell(p, i, mat, rgb, select);
        if (move_vacated(p.flags, snap[i])) rec->erased++;
    }
    // k_move_dst<false>: tiles, runs
    auto dst_pass = [&](bool build, bool go) {
        for (int tile = 0; tile < move_tile_count(p); tile++)
            for (int r = 0; r < VRT_MOVE_TILE / VRT_MOVE_RUN; r++) {
                int x, y, z;
                const int n = move_tile_run(p, tile, r, x, y, z);
                if (n <= 0) continue;
                MoveTally tl = move_tally_none();
                if (build) move_dst_run<true>(p, go, x, y, z, n, mat, rgb, snap, box_mat, box_rgb, tl);
                else {
                    move_dst_run<false>(p, true, x, y, z, n, mat, rgb, snap, nullptr, nullptr, tl);
                    rec->blocked += tl.blocked;
                    if (tl.written) {
                        rec->written += tl.written;
                        for (int a = 0; a < 3; a++) { if (tl.lo[a] < rec->lo[a]) rec->lo[a] = tl.lo[a]; if (tl.hi[a] > rec->hi[a]) rec->hi[a] = tl.hi[a]; }
                    }
                }
            }
    };
    if (n_dst) dst_pass(false, true);
    if (!(mv->flags & VRT_MOVE_DRY_RUN)) {
        const bool go = move_go(p.flags, rec->blocked);
        if (mv->flags & VRT_MOVE_ERASE_SOURCE) {   // k_move_src, launch_edit
            for (int i = 0; i < n_src; i++) move_src_build(p, go, i, mat, rgb, snap, box_mat, box_rgb);
            store_box(G, src, box_mat, box_rgb, mat, rgb);
        }
        if (n_dst) {                               // k_move_dst<true>, launch_edit
            dst_pass(true, go);
            store_box(G, dst, box_mat, box_rgb, mat, rgb);
        }
    }
    if (result) {
        long long written, blocked, erased;
        move_result(mv->flags, *rec, result->lo, result->hi, written, blocked, erased);
        result->written = written; result->blocked = blocked; result->erased = erased;
    }
    return VRT_OK;
}
}

#if defined(MOVE_EMUL_MAIN)
// A 128^3 grid with a block of voxels; moves that overlap their source, reach the grid's faces, sit at the coefficient bounds and carry
// a selection, each flag combination once: no out-of-bounds access, no overflow, and a copy there and back restores the grid.
int main() {
    const int G = 128;
    std::vector<int8_t> mat((size_t)G * G * G, 0);
    std::vector<uint8_t> rgb((size_t)G * G * G * 3, 0);
    for (int x = 60; x < 70; x++) for (int y = 10; y < 20; y++) for (int z = 0; z < 9; z++) {
        const size_t g = (size_t)edit_grid_index(G, x, y, z);
        mat[g] = (int8_t)((x + y + z) % 5 == 0 ? -3 : 1 + (x * 7 + y * 3 + z) % 120);
        rgb[3 * g] = (uint8_t)x; rgb[3 * g + 1] = (uint8_t)y; rgb[3 * g + 2] = (uint8_t)(z + 1);
    }
    const std::vector<int8_t> mat0 = mat;
    const std::vector<uint8_t> rgb0 = rgb;
    long long checked = 0;
    auto call = [&](vrt_voxel_move mv, const int* select, int staged, vrt_move_result* res) {
        EditBox s, d;
        for (int a = 0; a < 3; a++) { s.lo[a] = mv.src_lo[a]; s.hi[a] = mv.src_hi[a]; d.lo[a] = mv.dst_lo[a]; d.hi[a] = mv.dst_hi[a]; }
        const size_t need = (size_t)move_emul_plan(edit_box_voxels(s), edit_box_voxels(d), select && staged);
        std::vector<uint8_t> scratch(need);   // exactly the plan's bytes: the sanitizer guards the end
        const int rc = move_emul_call(G, mat.data(), rgb.data(), &mv, select, staged, res, scratch.data());
        checked++;
        return rc;
    };
    vrt_voxel_move mv;
    memset(&mv, 0, sizeof(mv));
    const int slo[3] = {61, 13, 2}, shi[3] = {68, 19, 7};
    for (int a = 0; a < 3; a++) { mv.src_lo[a] = slo[a]; mv.src_hi[a] = shi[a]; mv.dst_lo[a] = 0; mv.dst_hi[a] = G; }
    std::vector<int> select((size_t)(7 * 6 * 5));
    for (size_t i = 0; i < select.size(); i++) select[i] = (int)(i % 2);
    // identity + shift by (1, 0, -1) on every flag combination, with and without a selection
    for (unsigned flags = 0; flags < 16; flags++)
        for (int sel = 0; sel < 3; sel++) {
            mat = mat0; rgb = rgb0;
            mv.flags = flags; mv.select_value = 1;
            for (int i = 0; i < 9; i++) mv.m[i] = i % 4 == 0 ? 65536 : 0;
            mv.t[0] = -(1LL << 17); mv.t[1] = 0; mv.t[2] = 1LL << 17;
            vrt_move_result r;
            if (call(mv, sel ? select.data() : nullptr, sel == 2, &r) != VRT_OK) { printf("FAIL: flags %u\n", flags); return 1; }
            if ((flags & VRT_MOVE_DRY_RUN) && (mat != mat0 || rgb != rgb0)) { printf("FAIL: a dry run wrote\n"); return 1; }
        }
    // the coefficient bounds, every sign pattern of the diagonal and of t
    for (int k = 0; k < 64; k++) {
        mat = mat0; rgb = rgb0;
        mv.flags = VRT_MOVE_ERASE_SOURCE;
        for (int i = 0; i < 9; i++) mv.m[i] = (k >> (i % 3)) & 1 ? VRT_MOVE_M_MAX : -VRT_MOVE_M_MAX;
        for (int a = 0; a < 3; a++) mv.t[a] = (k >> (3 + a)) & 1 ? VRT_MOVE_T_MAX : -VRT_MOVE_T_MAX;
        if (call(mv, nullptr, 0, nullptr) != VRT_OK) { printf("FAIL: bounds %d\n", k); return 1; }
    }
    // a quarter turn about z's axis through (64.5, 50.5, *), into empty space, and back: a copy, then the copy by the inverse turn, restores the grid
    {
        mat = mat0; rgb = rgb0;
        vrt_voxel_move a;
        memset(&a, 0, sizeof(a));
        for (int i = 0; i < 3; i++) { a.src_lo[i] = slo[i]; a.src_hi[i] = shi[i]; a.dst_lo[i] = 0; a.dst_hi[i] = G; }
        a.flags = VRT_MOVE_ERASE_SOURCE;
        // forward p' = R (p - c) + c, R = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]; the map is its inverse: s = R^T (d - c) + c
        a.m[1] = 65536; a.m[3] = -65536; a.m[8] = 65536;
        a.t[0] = (long long)((64.5 - 50.5) * 131072.0); a.t[1] = (long long)((50.5 + 64.5) * 131072.0); a.t[2] = 0;
        vrt_move_result r1, r2;
        if (call(a, nullptr, 0, &r1) != VRT_OK) return 1;
        vrt_voxel_move b = a;
        for (int i = 0; i < 3; i++) { b.src_lo[i] = r1.lo[i]; b.src_hi[i] = r1.hi[i]; }
        b.m[1] = -65536; b.m[3] = 65536;
        b.t[0] = (long long)((64.5 + 50.5) * 131072.0); b.t[1] = (long long)((50.5 - 64.5) * 131072.0);
        if (call(b, nullptr, 0, &r2) != VRT_OK) return 1;
        if (r1.written != r1.erased || r2.written != r1.written) { printf("FAIL: the turn lost voxels: %lld %lld %lld\n", (long long)r1.written, (long long)r1.erased, (long long)r2.written); return 1; }
        // negative material bytes inside the box are no piece cells and stayed; everything else went there and back
        if (mat != mat0 || rgb != rgb0) { printf("FAIL: there and back differs\n"); return 1; }
    }
    printf("ok: %lld calls\n", checked);
    return 0;
}
#endif
