// edit_emul.cpp -- TEST TOOLING: the loops of the k_edit_* kernels (voxel_rt2_amd/csrc/vrt_scene_kernels.hip, launch_edit) run on the host over
// the functions of voxel_rt2_amd/csrc/vrt_edit.h, index by index, in the order launch_edit queues them (the loops: edit_emul.h).
// tests/test_voxel_edit_host.py compiles this with g++ and calls it through ctypes.
#include "edit_emul.h"

using namespace vrt;

extern "C" {

// 0: applied (an empty box: nothing to do); -1: not a box of a grid of G^3 voxels -- vrt_update_voxels' checks
int edit_apply(int G, const int* lo, const int* hi, const int8_t* box_mat, const uint8_t* box_rgb, int8_t* mat, uint8_t* rgb, uint32_t* grid,
               unsigned long long* l0, unsigned long long* l1, unsigned long long* l2, unsigned long long* l3) {
    EditBox box;
    for (int a = 0; a < 3; a++) { box.lo[a] = lo[a]; box.hi[a] = hi[a]; }
    if ((G != 128 && G != 256) || !edit_box_valid(box, G)) return -1;
    if (edit_box_voxels(box) == 0) return 0;
    emul_edit(G, box, box_mat, box_rgb, mat, rgb, grid, l0, l1, l2, l3);
    return 0;
}
// how many words of the level with cells of (1 << shift) voxels a box touches (the size of the k_edit_* grids)
int edit_touched(const int* lo, const int* hi, int shift) {
    EditBox box;
    for (int a = 0; a < 3; a++) { box.lo[a] = lo[a]; box.hi[a] = hi[a]; }
    return edit_box_voxels(box) == 0 ? 0 : edit_cell_count(edit_cells(box, shift));
}

}  // extern "C"
