// voxelize_emul.cpp -- TEST TOOLING: the loops of the k_vox_* kernels (voxel_rt2_amd/csrc/vrt_scene_kernels.hip) and of vrt_voxelize_triangles
// (vrt_scene_ops.hip) run on the host over the functions of voxel_rt2_amd/csrc/vrt_voxelize.h: the set-up pass triangle by triangle, the
// rasterise pass grab by grab with the 64 lanes of a wave one after the other, the resolve voxel by voxel, then launch_edit's loops
// (vrt_edit.h) -- in chunks whose size the caller chooses, so that ownership has to carry across them.  tests/voxelize.py compiles this
// with g++ and calls it through ctypes.
// -DVOX_EMUL_MAIN: a stand-alone program (its own main, no Python) over a small generated mesh -- what a sanitizer build runs.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../voxel_rt2_amd/csrc/vrt_voxelize.h"
#include "edit_emul.h"
#include "../../voxel_rt2_amd/csrc/vrt_plan.h"

using namespace vrt;

// k_vox_setup + k_vox_raster over one batch
static void batch(int G, const EditBox& clip, unsigned long long base, long long m, const vrt_triangle* tris, int grab, std::vector<uint32_t>& owner,
                  long long& invalid) {
    std::vector<VoxEntry> entries;
    unsigned long long total = 0;
    for (long long i = 0; i < m; i++) {
        bool valid;
        const uint32_t items = vox_tri_items(tris[i], G, clip, valid);
        if (!valid) invalid++;
        if (items) { entries.push_back(VoxEntry{total, (uint32_t)i, items}); total += items; }
    }
    for (unsigned long long g0 = 0; g0 < total; g0 += (unsigned long long)grab) {   // one grab of one wave
        unsigned long long g = g0;
        const unsigned long long g1 = g + grab < total ? g + grab : total;
        long long e = vox_find_entry(entries.data(), (long long)entries.size(), g);
        while (g < g1 && e < (long long)entries.size()) {
            const VoxEntry en = entries[(size_t)e++];
            VoxTri s;
            vox_setup(tris[en.tri], G, s);
            const EditCells cells = vox_cells(s, clip, 4), bricks = vox_cells(s, clip, 2);
            const uint32_t mine = (uint32_t)(base + en.tri + 1ULL);
            const unsigned long long end = en.first + en.items < g1 ? en.first + en.items : g1;
            for (; g < end; g++) {
                int cx, cy, cz;
                edit_cell(cells, (int)(g - en.first), cx, cy, cz);
                if (!vox_cube(s, cx, cy, cz, 4)) continue;
                unsigned long long todo = 0ULL;
                for (int lane = 0; lane < 64; lane++) if (vox_lane_brick(s, bricks, cx, cy, cz, lane)) todo |= 1ULL << lane;
                for (int brick = 0; brick < 64; brick++) {
                    if (!((todo >> brick) & 1ULL)) continue;
                    for (int lane = 0; lane < 64; lane++) {
                        const int at = vox_lane_voxel(s, clip, cx, cy, cz, brick, lane);
                        if (at >= 0 && owner[(size_t)at] < mine) owner[(size_t)at] = mine;
                    }
                }
            }
        }
    }
}

extern "C" {

// vrt_voxelize_triangles on host arrays (tests/edit.py's HostGrid): 0 = VRT_OK, -1 = VRT_E_INVALID.  chunk: triangles a batch; grab: items
// a wave reserves at a time.  once = 0: every batch's owners are resolved while its triangles are at hand (the host path's chunks); once = 1:
// the batches only raise owners and one resolve with base 0 over the whole array follows (the device path with n above a batch).
// result: a vrt_voxelize_result.
int vox_emul_call(int G, long long n, const vrt_triangle* tris, const int* lo, const int* hi, long long chunk, int grab, int once, int8_t* mat, uint8_t* rgb,
                  uint32_t* grid, unsigned long long* l0, unsigned long long* l1, unsigned long long* l2, unsigned long long* l3, vrt_voxelize_result* result) {
    EditBox box;
    if (const int go = emul_tri_checks(G, n, tris, lo, hi, chunk, grab, box, result); go <= 0) return go;
    const int nv = edit_box_voxels(box);
    std::vector<uint32_t> owner((size_t)nv, 0u);
    std::vector<int8_t> box_mat((size_t)nv, (int8_t)0x55);
    std::vector<uint8_t> box_rgb((size_t)nv * 3, (uint8_t)0x55);
    EmulTally tally;
    for (long long at = 0; at < n; at += chunk) {
        const long long m = chunk < n - at ? chunk : n - at;
        batch(G, box, (unsigned long long)at, m, tris + at, grab, owner, tally.invalid);
        const bool final = at + m >= n;
        if (once && !final) continue;
        const long long base = once ? 0 : at;
        for (int i = 0; i < nv; i++) {   // k_vox_resolve
            const bool written = vox_resolve_voxel(box, G, i, owner.data(), (unsigned long long)base, tris + base, final, mat, rgb, box_mat.data(), box_rgb.data());
            if (final && written) tally.add(box, i);
        }
    }
    emul_edit(G, box, box_mat.data(), box_rgb.data(), mat, rgb, grid, l0, l1, l2, l3);   // launch_edit
    tally.store(result);
    return 0;
}
// COVERS of include/vrt_api.h for one triangle and n cells (int32[n][3]); out[i] = 1 / 0, or -1 throughout for an invalid triangle
int vox_emul_covers(int G, const vrt_triangle* t, long long n, const int32_t* cells, int8_t* out, int shift) {
    if (!vox_tri_valid(*t)) { for (long long i = 0; i < n; i++) out[i] = -1; return 0; }
    VoxTri s;
    vox_setup(*t, G, s);
    for (long long i = 0; i < n; i++) out[i] = vox_cube(s, cells[3 * i], cells[3 * i + 1], cells[3 * i + 2], shift) ? 1 : 0;
    return 1;
}
int vox_emul_snap(float w, int G) { return vox_snap(w, G); }
int vox_emul_valid(const vrt_triangle* t) { return vox_tri_valid(*t) ? 1 : 0; }
// the set-up record flattened to int64: v[9], bmin[3], bmax[3], nn[3], nmin, nmax, nneg, npos, then per cross axis k (9 of them):
// cn[3], cmin, cmax, cneg, cpos  -- 22 + 63 = 85 values
int vox_emul_setup(const vrt_triangle* t, int G, long long* out) {
    VoxTri s;
    vox_setup(*t, G, s);
    int o = 0;
    for (int i = 0; i < 3; i++) for (int a = 0; a < 3; a++) out[o++] = s.v[i][a];
    for (int a = 0; a < 3; a++) out[o++] = s.bmin[a];
    for (int a = 0; a < 3; a++) out[o++] = s.bmax[a];
    for (int a = 0; a < 3; a++) out[o++] = s.nn[a];
    out[o++] = s.nmin; out[o++] = s.nmax; out[o++] = s.nneg; out[o++] = s.npos;
    for (int k = 0; k < 9; k++) {
        for (int a = 0; a < 3; a++) out[o++] = s.cn[k][a];
        out[o++] = s.cmin[k]; out[o++] = s.cmax[k]; out[o++] = s.cneg[k]; out[o++] = s.cpos[k];
    }
    return o;
}
// the clipped cells of a triangle at a level: lo[3], n[3]
void vox_emul_cells(const vrt_triangle* t, int G, const int* lo, const int* hi, int shift, int* out) {
    EditBox box;
    for (int a = 0; a < 3; a++) { box.lo[a] = lo[a]; box.hi[a] = hi[a]; }
    VoxTri s;
    vox_snap_tri(*t, G, s);
    const EditCells c = vox_cells(s, box, shift);
    for (int a = 0; a < 3; a++) { out[a] = c.lo[a]; out[3 + a] = c.n[a]; }
}
long long vox_emul_plan(int which) { return which == 0 ? plan_voxelize_chunk() : which == 1 ? plan_voxelize_batch() : VRT_VOX_ITEMS_PER_GRAB; }
int vox_emul_sizes(int which) { return which == 0 ? (int)sizeof(vrt_triangle) : which == 1 ? (int)sizeof(vrt_voxelize_result) : (int)sizeof(VoxEntry); }

}  // extern "C"

#if defined(VOX_EMUL_MAIN)
// A band of triangles winding through a 128^3 grid, some degenerate, some invalid, into an unaligned box: whole batches, chunks of 3
// with grabs of 1, and batches of 3 resolved once must leave the same bytes.
int main() {
    const int G = 128;
    const size_t n3 = (size_t)G * G * G;
    uint32_t rng = 2463534242u;
    auto u = [&]() { rng = rng * 747796405u + 2891336453u; return (float)((rng >> 8) & 0xffffu) / 65536.0f; };
    std::vector<vrt_triangle> tris;
    for (int i = 0; i < 300; i++) {
        vrt_triangle t;
        memset(&t, 0, sizeof(t));
        const float c[3] = {u() * 1.6f - 0.8f, u() * 1.6f - 0.8f, u() * 1.6f - 0.8f}, r = (i % 5 == 0) ? 1.5f : 0.2f;
        for (int a = 0; a < 3; a++) { t.v0[a] = c[a] + (u() - 0.5f) * r; t.v1[a] = c[a] + (u() - 0.5f) * r; t.v2[a] = c[a] + (u() - 0.5f) * r; }
        if (i % 7 == 0) for (int a = 0; a < 3; a++) t.v2[a] = t.v1[a];
        if (i % 13 == 0) for (int a = 0; a < 3; a++) t.v0[a] = t.v1[a] = t.v2[a] = (float)(int)(c[a] * 64.0f) / 64.0f;
        if (i % 17 == 0) t.v1[1] = 9.0f;
        t.voxel = rng | 0x01000000u;
        if (i % 11 == 0) t.voxel &= 0x00ffffffu;
        tris.push_back(t);
    }
    const int lo[3] = {3, 5, 62}, hi[3] = {90, 70, 101};
    std::vector<std::vector<unsigned char>> got;
    vrt_voxelize_result res[3];
    const long long chunks[3] = {1 << 20, 3, 3};
    const int grabs[3] = {8, 1, 1}, once[3] = {0, 0, 1};
    for (int k = 0; k < 3; k++) {
        std::vector<int8_t> mat(n3, 0);
        std::vector<uint8_t> rgb(n3 * 3, 0);
        std::vector<uint32_t> grid(n3, 0);
        std::vector<unsigned long long> l0(n3 / 64, 0), l1(n3 / 4096, 0), l2(8, 0), l3(1, 0);
        if (vox_emul_call(G, (long long)tris.size(), tris.data(), lo, hi, chunks[k], grabs[k], once[k], mat.data(), rgb.data(), grid.data(), l0.data(), l1.data(), l2.data(),
                          l3.data(), &res[k]) != 0) { printf("FAIL call %d\n", k); return 1; }
        std::vector<unsigned char> all(n3 * 8 + l0.size() * 8);
        memcpy(all.data(), mat.data(), n3); memcpy(all.data() + n3, rgb.data(), n3 * 3); memcpy(all.data() + n3 * 4, grid.data(), n3 * 4);
        memcpy(all.data() + n3 * 8, l0.data(), l0.size() * 8);
        got.push_back(all);
    }
    if (got[0] != got[1] || got[0] != got[2] || memcmp(&res[0], &res[1], sizeof(res[0])) != 0 || memcmp(&res[0], &res[2], sizeof(res[0])) != 0) { printf("FAIL: chunking changed the outcome\n"); return 1; }
    printf("ok: %zu triangles, %lld voxels written, %lld invalid\n", tris.size(), (long long)res[0].voxels, (long long)res[0].invalid);
    return (res[0].voxels > 0 && res[0].invalid > 0) ? 0 : 2;
}
#endif
