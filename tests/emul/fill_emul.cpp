// fill_emul.cpp -- TEST TOOLING: the loops of the k_fill_* kernels (voxel_rt2_amd/csrc/vrt_scene_kernels.hip) and of vrt_fill_triangles
// (vrt_scene_ops.hip) run on the host over the functions of voxel_rt2_amd/csrc/vrt_fill.h: the set-up pass triangle by triangle, the
// rasterise pass grab by grab with the 64 lanes of a wave one after the other, ONE resolve voxel by voxel after every batch, then
// launch_edit's loops (vrt_edit.h) -- in batches whose size the caller chooses.  tests/fill.py compiles this with g++ and calls it
// through ctypes.
// -DFILL_EMUL_MAIN: a stand-alone program (its own main, no Python) over a small generated mesh -- what a sanitizer build runs.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../voxel_rt2_amd/csrc/vrt_fill.h"
#include "edit_emul.h"
#include "../../voxel_rt2_amd/csrc/vrt_plan.h"

using namespace vrt;

// k_fill_setup + k_fill_raster over one batch
static void batch(int G, const EditBox& clip, long long m, const vrt_triangle* tris, int grab, std::vector<uint32_t>& toggles, long long& invalid) {
    std::vector<VoxEntry> entries;
    unsigned long long total = 0;
    for (long long i = 0; i < m; i++) {
        bool valid;
        const uint32_t items = fill_tri_items(tris[i], G, clip, valid);
        if (!valid) invalid++;
        if (items) { entries.push_back(VoxEntry{total, (uint32_t)i, items}); total += items; }
    }
    for (unsigned long long g0 = 0; g0 < total; g0 += (unsigned long long)grab) {   // one grab of one wave
        unsigned long long g = g0;
        const unsigned long long g1 = g + grab < total ? g + grab : total;
        long long e = vox_find_entry(entries.data(), (long long)entries.size(), g);
        while (g < g1 && e < (long long)entries.size()) {
            const VoxEntry en = entries[(size_t)e++];
            FillTri s;
            fill_setup(tris[en.tri], G, s);
            const EditCells cells = fill_cells(s, clip), tiles = fill_tiles(cells);
            const unsigned long long end = en.first + en.items < g1 ? en.first + en.items : g1;
            for (; g < end; g++) {
                int tx, ty, tz;
                edit_cell(tiles, (int)(g - en.first), tx, ty, tz);
                for (int lane = 0; lane < 64; lane++)
                    for (int k = 0; k < 4; k++) {
                        int cx, cy;
                        if (!fill_lane_column(s, cells, tx, ty, lane, k, cx, cy)) continue;
                        uint32_t bit;
                        const int at = fill_toggle_at(clip, cx, cy, fill_first_cell(s, cx, cy), bit);
                        if (at >= 0) toggles.at((size_t)at) ^= bit;
                    }
            }
        }
    }
}

extern "C" {

// vrt_fill_triangles on host arrays (tests/edit.py's HostGrid): 0 = VRT_OK, -1 = VRT_E_INVALID.  chunk: triangles a batch (the host
// path's chunks and the device path's batches are the same thing here: toggle, toggle, ..., resolve once); grab: items a wave reserves at
// a time.  result: a vrt_voxelize_result.
int fill_emul_call(int G, long long n, const vrt_triangle* tris, const int* lo, const int* hi, unsigned voxel, long long chunk, int grab, int8_t* mat, uint8_t* rgb,
                   uint32_t* grid, unsigned long long* l0, unsigned long long* l1, unsigned long long* l2, unsigned long long* l3, vrt_voxelize_result* result) {
    EditBox box;
    if (const int go = emul_tri_checks(G, n, tris, lo, hi, chunk, grab, box, result); go <= 0) return go;
    const int nv = edit_box_voxels(box);
    std::vector<uint32_t> toggles((size_t)fill_words(box), 0u);
    std::vector<int8_t> box_mat((size_t)nv, (int8_t)0x55);
    std::vector<uint8_t> box_rgb((size_t)nv * 3, (uint8_t)0x55);
    EmulTally tally;
    for (long long at = 0; at < n; at += chunk) batch(G, box, chunk < n - at ? chunk : n - at, tris + at, grab, toggles, tally.invalid);
    for (int i = 0; i < nv; i++)   // k_fill_resolve
        if (fill_resolve_voxel(box, G, i, toggles.data(), voxel, mat, rgb, box_mat.data(), box_rgb.data())) tally.add(box, i);
    emul_edit(G, box, box_mat.data(), box_rgb.data(), mat, rgb, grid, l0, l1, l2, l3);   // launch_edit
    tally.store(result);
    return 0;
}
// fill_column_in / fill_first_cell for one triangle and n columns (int32[n][2]): in[i] = 1 / 0 (-1 throughout for an invalid triangle),
// first[i] = the first cell of a column that is in (untouched otherwise)
int fill_emul_columns(int G, const vrt_triangle* t, long long n, const int32_t* cols, int8_t* in, long long* first) {
    if (!vox_tri_valid(*t)) { for (long long i = 0; i < n; i++) in[i] = -1; return 0; }
    FillTri s;
    fill_setup(*t, G, s);
    for (long long i = 0; i < n; i++) {
        in[i] = fill_column_in(s, cols[2 * i], cols[2 * i + 1]) ? 1 : 0;
        if (in[i]) first[i] = fill_first_cell(s, cols[2 * i], cols[2 * i + 1]);
    }
    return 1;
}
// the set-up record flattened to int64: v[9], bmin[3], bmax[3], nn[3], sigma, then per edge (3 of them) dx, dy, e0, etie, then
// fx, fy, f0, slope, ftie -- 19 + 12 + 5 = 36 values
int fill_emul_setup(const vrt_triangle* t, int G, long long* out) {
    FillTri s;
    fill_setup(*t, G, s);
    int o = 0;
    for (int i = 0; i < 3; i++) for (int a = 0; a < 3; a++) out[o++] = s.v[i][a];
    for (int a = 0; a < 3; a++) out[o++] = s.bmin[a];
    for (int a = 0; a < 3; a++) out[o++] = s.bmax[a];
    for (int a = 0; a < 3; a++) out[o++] = s.nn[a];
    out[o++] = s.sigma;
    for (int i = 0; i < 3; i++) { out[o++] = s.dx[i]; out[o++] = s.dy[i]; out[o++] = s.e0[i]; out[o++] = s.etie[i] ? 1 : 0; }
    out[o++] = s.fx; out[o++] = s.fy; out[o++] = s.f0; out[o++] = s.slope; out[o++] = s.ftie ? 1 : 0;
    return o;
}
// the clipped columns of a triangle and its tiles: lo[2], n[2] of each, and its item count
void fill_emul_cells(const vrt_triangle* t, int G, const int* lo, const int* hi, int* out) {
    EditBox box;
    for (int a = 0; a < 3; a++) { box.lo[a] = lo[a]; box.hi[a] = hi[a]; }
    FillTri s;
    fill_setup(*t, G, s);
    const EditCells c = fill_cells(s, box), tl = fill_tiles(c);
    for (int a = 0; a < 2; a++) { out[a] = c.lo[a]; out[2 + a] = c.n[a]; out[4 + a] = tl.lo[a]; out[6 + a] = tl.n[a]; }
    bool valid;
    out[8] = (int)fill_tri_items(*t, G, box, valid);
}
// the prefix-XOR of n words of one column, in place
void fill_emul_prefix(long long n, uint32_t* words) {
    uint32_t carry = 0u;
    for (long long i = 0; i < n; i++) words[i] = fill_prefix_word(words[i], carry);
}
long long fill_emul_plan(int which) { return which == 0 ? plan_voxelize_chunk() : which == 1 ? plan_voxelize_batch() : VRT_FILL_ITEMS_PER_GRAB; }

}  // extern "C"

#if defined(FILL_EMUL_MAIN)
// Closed tetrahedra, some with a duplicated or an invalid face, scattered through a 128^3 grid and filled into an unaligned box: one
// batch, batches of 3 with grabs of 1, and batches of 7 with grabs of 64 must leave the same bytes.
int main() {
    const int G = 128;
    const size_t n3 = (size_t)G * G * G;
    uint32_t rng = 2463534242u;
    auto u = [&]() { rng = rng * 747796405u + 2891336453u; return (float)((rng >> 8) & 0xffffu) / 65536.0f; };
    std::vector<vrt_triangle> tris;
    for (int i = 0; i < 60; i++) {
        float p[4][3];
        const float r = (i % 5 == 0) ? 1.4f : 0.35f;
        float c[3] = {u() * 1.4f - 0.7f, u() * 1.4f - 0.7f, u() * 1.4f - 0.7f};
        for (int k = 0; k < 4; k++) for (int a = 0; a < 3; a++) p[k][a] = c[a] + (u() - 0.5f) * r;
        if (i % 9 == 0) for (int k = 0; k < 4; k++) for (int a = 0; a < 3; a++) p[k][a] = (float)(int)(p[k][a] * 64.0f) / 64.0f + 1.0f / 128.0f;   // on cell centres
        const int f[4][3] = {{0, 1, 2}, {0, 3, 1}, {1, 3, 2}, {2, 3, 0}};
        for (int k = 0; k < 4; k++) {
            vrt_triangle t;
            memset(&t, 0, sizeof(t));
            for (int a = 0; a < 3; a++) { t.v0[a] = p[f[k][0]][a]; t.v1[a] = p[f[k][1]][a]; t.v2[a] = p[f[k][2]][a]; }
            if (i % 17 == 0 && k == 2) t.v1[1] = 9.0f;
            tris.push_back(t);
            if (i % 13 == 0 && k == 1) tris.push_back(t);
        }
    }
    const int lo[3] = {3, 5, 30}, hi[3] = {90, 70, 101};
    std::vector<std::vector<unsigned char>> got;
    vrt_voxelize_result res[3];
    const long long chunks[3] = {1 << 20, 3, 7};
    const int grabs[3] = {8, 1, 64};
    for (int k = 0; k < 3; k++) {
        std::vector<int8_t> mat(n3, 0);
        std::vector<uint8_t> rgb(n3 * 3, 0);
        std::vector<uint32_t> grid(n3, 0);
        std::vector<unsigned long long> l0(n3 / 64, 0), l1(n3 / 4096, 0), l2(8, 0), l3(1, 0);
        if (fill_emul_call(G, (long long)tris.size(), tris.data(), lo, hi, 0x0b5aa03cu, chunks[k], grabs[k], mat.data(), rgb.data(), grid.data(), l0.data(), l1.data(), l2.data(),
                           l3.data(), &res[k]) != 0) { printf("FAIL call %d\n", k); return 1; }
        std::vector<unsigned char> all(n3 * 8 + l0.size() * 8);
        memcpy(all.data(), mat.data(), n3); memcpy(all.data() + n3, rgb.data(), n3 * 3); memcpy(all.data() + n3 * 4, grid.data(), n3 * 4);
        memcpy(all.data() + n3 * 8, l0.data(), l0.size() * 8);
        got.push_back(all);
    }
    if (got[0] != got[1] || got[0] != got[2] || memcmp(&res[0], &res[1], sizeof(res[0])) != 0 || memcmp(&res[0], &res[2], sizeof(res[0])) != 0) { printf("FAIL: batching changed the outcome\n"); return 1; }
    printf("ok: %zu triangles, %lld voxels inside, %lld invalid\n", tris.size(), (long long)res[0].voxels, (long long)res[0].invalid);
    return (res[0].voxels > 0 && res[0].invalid > 0) ? 0 : 2;
}
#endif
