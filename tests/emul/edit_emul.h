// edit_emul.h -- TEST TOOLING shared by edit_emul.cpp, voxelize_emul.cpp and fill_emul.cpp: launch_edit's loops, and what the emulations
// of the two triangle edits (vox_emul_call, fill_emul_call) have in common -- the checks of tri_edit (voxel_rt2_amd/csrc/vrt_scene_ops.hip),
// the count-and-bounds tally both resolve kernels end on (tri_tally, vrt_scene_kernels.hip) and the result record's conversion.
#pragma once
#include <cstring>
#include "../../voxel_rt2_amd/csrc/vrt_voxelize.h"

namespace vrt {

template <int G>
static void emul_edit_loops(const EditBox& box, const int8_t* box_mat, const uint8_t* box_rgb, int8_t* mat, uint8_t* rgb, uint32_t* grid,
                            unsigned long long* l0, unsigned long long* l1, unsigned long long* l2, unsigned long long* l3) {
    for (int i = 0; i < edit_box_voxels(box); i++) edit_store_voxel<G>(box, i, box_mat, box_rgb, mat, rgb, grid);
    for (int i = 0; i < edit_cell_count(edit_cells(box, 2)); i++) edit_rebuild_fine(box, i, mat, l0, G);
    for (int i = 0; i < edit_cell_count(edit_cells(box, 4)); i++) edit_rebuild_coarse(box, 4, i, l0, l1, G);
    for (int i = 0; i < edit_cell_count(edit_cells(box, 6)); i++) edit_rebuild_coarse(box, 6, i, l1, l2, G);
    if (G == 256) for (int i = 0; i < edit_cell_count(edit_cells(box, 8)); i++) edit_rebuild_coarse(box, 8, i, l2, l3, G);
}
// launch_edit: the loops of the k_edit_* kernels index by index, in the order launch_edit queues them.  G: 128 or 256.
static void emul_edit(int G, const EditBox& box, const int8_t* box_mat, const uint8_t* box_rgb, int8_t* mat, uint8_t* rgb, uint32_t* grid,
                      unsigned long long* l0, unsigned long long* l1, unsigned long long* l2, unsigned long long* l3) {
    if (G == 256) emul_edit_loops<256>(box, box_mat, box_rgb, mat, rgb, grid, l0, l1, l2, l3);
    else emul_edit_loops<128>(box, box_mat, box_rgb, mat, rgb, grid, l0, l1, l2, l3);
}

// The checks of a triangle edit on host arrays, `box` built and *result zeroed on the way: -1 = VRT_E_INVALID, 0 = VRT_OK with nothing
// to do (an empty box, no triangle), 1 = go on.  chunk: triangles a batch; grab: items a wave reserves at a time.
static int emul_tri_checks(int G, long long n, const vrt_triangle* tris, const int* lo, const int* hi, long long chunk, int grab, EditBox& box,
                           vrt_voxelize_result* result) {
    if (!tris || !lo || !hi || (G != 128 && G != 256) || chunk < 1 || grab < 1) return -1;
    if (n < 0 || n >= 4294967295LL) return -1;
    for (int a = 0; a < 3; a++) { box.lo[a] = lo[a]; box.hi[a] = hi[a]; }
    if (!edit_box_valid(box, G)) return -1;
    for (long long k = 0; k < n; k++) if (tris[k].reserved0 != 0u || tris[k].reserved1 != 0u) return -1;
    if (result) memset(result, 0, sizeof(*result));
    return edit_box_voxels(box) == 0 || n == 0 ? 0 : 1;
}
// What a call counts: the invalid triangles (the set-up pass), the voxels the final resolve writes and their tight box; `store` converts
// as the call does (hi exclusive, the box left zero when nothing was written).
struct EmulTally {
    long long voxels = 0, invalid = 0;
    int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-1, -1, -1};
    void add(const EditBox& box, int i) {
        int c[3];
        edit_box_voxel(box, i, c[0], c[1], c[2]);
        voxels++;
        for (int a = 0; a < 3; a++) { if (c[a] < lo[a]) lo[a] = c[a]; if (c[a] > hi[a]) hi[a] = c[a]; }
    }
    void store(vrt_voxelize_result* result) const {
        if (!result) return;
        result->voxels = voxels; result->invalid = invalid;
        if (voxels) for (int a = 0; a < 3; a++) { result->lo[a] = lo[a]; result->hi[a] = hi[a] + 1; }
    }
};

}  // namespace vrt
