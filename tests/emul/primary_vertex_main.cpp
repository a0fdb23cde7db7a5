// primary_vertex_main.cpp -- TEST TOOLING: a stand-alone program around primary_vertex_emul.cpp, for sanitizer builds of the host build
// of vrt_primary.h (tests/test_primary_vertex_host.py compiles it with -fsanitize=address,undefined and runs it; nothing is preloaded,
// nothing here touches a GPU).
//     primary_vertex_main CASE_FILE
// CASE_FILE: vrt_config, vrt_scene_params, vrt_camera, uint32 n_samples, int8 mat[G^3], uint8 rgb[G^3][3], float materials[128][14] -- the
// structs as include/vrt_api.h lays them out.  The frame is rendered three times -- by the emulated pool alone, behind the primary-vertex
// stage with the rule's queue, and with eight records a head and every eleventh record spoilt -- and the program exits 1 unless the HDR
// frames and both histories of all three are the same bytes.
#include <cstdio>
#include "primary_vertex_emul.cpp"

template <class T>
static bool read_all(FILE* f, T* at, size_t n) { return fread(at, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASE_FILE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    vrt_config cfg;
    vrt_scene_params scene;
    vrt_camera cam;
    uint32_t n_samples = 0;
    if (!read_all(f, &cfg, 1) || !read_all(f, &scene, 1) || !read_all(f, &cam, 1) || !read_all(f, &n_samples, 1) || n_samples == 0 || n_samples > 16) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t nv = (size_t)cfg.grid_res * cfg.grid_res * cfg.grid_res;
    std::vector<int8_t> mat(nv);
    std::vector<uint8_t> rgb(3 * nv);
    std::vector<float> table(128 * 14);
    if (!read_all(f, mat.data(), nv) || !read_all(f, rgb.data(), 3 * nv) || !read_all(f, table.data(), table.size())) { fprintf(stderr, "short file\n"); return 2; }
    fclose(f);
    setenv("VRT_EMU_POOL", "1", 1);
    setenv("VRT_EMU_CULL", "1", 1);
    const size_t n = (size_t)cfg.width * cfg.height;
    std::vector<float> hdr[3], hd[3], hs[3];
    unsigned long long counts[3][3] = {{0}};
    for (int k = 0; k < 3; k++) {
        Emu* c = emu_create(&cfg);
        if (!c) { fprintf(stderr, "emu_create failed\n"); return 2; }
        emu_upload_voxels(c, mat.data(), rgb.data());
        emu_upload_materials(c, table.data());
        emu_set_scene(c, &scene);
        emu_set_camera(c, &cam);
        emu_prepare(c);
        if (k == 0) emu_accumulate(c, (int)n_samples);
        else if (emu_accumulate_primary(c, (int)n_samples, 1, k == 2 ? 64 : 0, k == 2, counts[k]) != 0) return 2;
        hdr[k].resize(3 * n); hd[k].resize(4 * n); hs[k].resize(4 * n);
        emu_fetch_hdr(c, hdr[k].data());
        emu_fetch_buffer(c, VRT_BUF_HISTORY_DIFFUSE, hd[k].data());
        emu_fetch_buffer(c, VRT_BUF_HISTORY_SPECULAR, hs[k].data());
        emu_destroy(c);
    }
    int bad = 0;
    for (int k = 1; k < 3; k++)
        bad += memcmp(hdr[0].data(), hdr[k].data(), 12 * n) != 0 || memcmp(hd[0].data(), hd[k].data(), 16 * n) != 0 || memcmp(hs[0].data(), hs[k].data(), 16 * n) != 0;
    printf("samples %u finished %llu sent on %llu leftovers %llu; bounded: finished %llu sent on %llu leftovers %llu; frames that differ %d\n", n_samples,
           counts[1][0], counts[1][1], counts[1][2], counts[2][0], counts[2][1], counts[2][2], bad);
    return bad ? 1 : 0;
}
