// primary_records_main.cpp -- TEST TOOLING: a stand-alone program around primary_emul.cpp, for sanitizer builds of the host build of
// primary_record_walk() (tests/test_primary_records_host.py compiles it with -fsanitize=address,undefined and runs it; nothing is
// preloaded, nothing here touches a GPU).
//     primary_records_main CASE_FILE
// CASE_FILE: vrt_config, vrt_scene_params, uint32 n, n x vrt_camera, int8 mat[G^3], uint8 rgb[G^3][3] -- the structs as include/vrt_api.h
// lays them out.  Every camera's frame is worked with the scene's culling box and with the open one; the program prints what it
// compared and exits 1 if a record made by primary_record_walk() differs from the one the emulated pooled schedule leaves.
#include <cstdio>
#include "primary_emul.cpp"

template <class T>
static bool read_all(FILE* f, T* at, size_t n) { return fread(at, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASE_FILE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    vrt_config cfg;
    vrt_scene_params scene;
    uint32_t n_cams = 0;
    if (!read_all(f, &cfg, 1) || !read_all(f, &scene, 1) || !read_all(f, &n_cams, 1) || n_cams == 0 || n_cams > 64) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<vrt_camera> cams(n_cams);
    const size_t nv = (size_t)cfg.grid_res * cfg.grid_res * cfg.grid_res;
    std::vector<int8_t> mat(nv);
    std::vector<uint8_t> rgb(3 * nv);
    if (!read_all(f, cams.data(), cams.size()) || !read_all(f, mat.data(), nv) || !read_all(f, rgb.data(), 3 * nv)) { fprintf(stderr, "short file\n"); return 2; }
    fclose(f);
    Emu* c = emu_create(&cfg);
    if (!c) { fprintf(stderr, "emu_create failed\n"); return 2; }
    emu_upload_voxels(c, mat.data(), rgb.data());
    emu_set_scene(c, &scene);
    emu_prepare(c);
    const size_t n = c->n;
    std::vector<PrimaryRecord> a(n), b(n);
    std::vector<uint8_t> walked(n);
    size_t records = 0, n_walked = 0, bad = 0;
    for (uint32_t k = 0; k < n_cams; k++)
        for (int cull = 1; cull >= 0; cull--) {
            emu_set_camera(c, &cams[k]);
            const uint32_t tag = 7u + 3u * k;
            memset(a.data(), 0, n * sizeof(PrimaryRecord));
            memset(b.data(), 0, n * sizeof(PrimaryRecord));
            if (emu_primary_records(c, cull, tag, a.data(), b.data(), walked.data()) != 0) return 2;
            for (size_t i = 0; i < n; i++) {
                records++;
                n_walked += walked[i];
                if (memcmp(&a[i], &b[i], sizeof(PrimaryRecord)) != 0 || !primary_record_valid(a[i], tag) || primary_record_valid(a[i], tag + 1u)) bad++;
            }
        }
    emu_destroy(c);
    printf("frames %u records %zu walked %zu mismatches %zu\n", 2u * n_cams, records, n_walked, bad);
    return bad ? 1 : 0;
}
