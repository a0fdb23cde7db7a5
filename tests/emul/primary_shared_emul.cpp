// primary_shared_emul.cpp -- TEST TOOLING: primary_vertex_emul.cpp plus the two forms of a pixel's depth-0 shading side by side, on the host.
// k_primary_vertex builds the shading point of a pixel's primary vertex once (primary_vertex_surf) and hands it to every fused sample
// (primary_vertex_sample<..., true>); the form it replaces built it inside path_shade for every sample.  emu_primary_shared_check walks
// every pixel of the frame: the camera ray's record, the hit, the shading point both ways -- once a pixel, and as path_shade builds it
// from a path begun for the sample -- and samples 0 .. n-1 through both forms into sample planes of their own.  It counts what differs:
// the words of the shading point, the words a path that goes on is left in (the continuation record, emitting-sun layout: every field
// either form could have touched, and whether it goes on at all), and afterwards the bytes of the colour and reflection-depth planes the
// finished paths stored.
// With -DPRIMARY_SHARED_MAIN the file is a stand-alone program over a CASE_FILE as primary_vertex_main.cpp reads it, for sanitizer
// builds (tests/test_primary_shared_host.py; nothing is preloaded, nothing here touches a GPU).
#include "primary_vertex_emul.cpp"

struct PsCounts { unsigned long long surfaces, samples, sent_on, surf_words, path_words, plane_bytes; };

struct PsPlanes {
    std::vector<f3> color_d, color_s;
    std::vector<float> refl;
    PsPlanes(size_t n) : color_d(n, mk3(-1.0f)), color_s(n, mk3(-1.0f)), refl(n, -1.0f) {}
    void bind(PixelBuffers& out, int stride) {
        memset(&out, 0, sizeof(out));
        out.color_d = color_d.data(); out.color_s = color_s.data(); out.gb_refl_depth = refl.data();
        out.sample_stride = stride;
    }
};

template <int G, bool BLACK_SUN, bool CULL>
static void ps_check(Emu* c, const FrameParams& fp, const SceneData& sc, int n_samples, PsCounts& n) {
    GlobalPyramid<G> P;
    P.p = sc.pyr;
    const int rows = fp.row1 - fp.row0, stride = rows * fp.W;
    PsPlanes each((size_t)stride * n_samples), shared((size_t)stride * n_samples);
    PixelBuffers out_each, out_shared;
    each.bind(out_each, stride);
    shared.bind(out_shared, stride);
    const uint32_t tag = fp.frame + 1u;
    for (int v = fp.row0; v < fp.row1; v++)
        for (int u = 0; u < fp.W; u++) {
            if (!launch_renders_row(fp, v) || outside_render_area(fp, (float)u, (float)v)) continue;
            const PrimaryRecord rec = primary_record_walk<G, CULL>(fp, P, sc.cull, u, v, tag);
            Hit h;
            const int state = primary_vertex_hit<G>(fp, sc, rec, h, c->ts);
            Surf once;
            memset(&once, 0, sizeof(once));
            const bool built = primary_vertex_surf<GlobalPyramid<G>>(sc, rec, h, state, once);
            if (built) {   // what path_shade builds for a sample of this pixel: from the path's own direction
                Path<false> q;
                path_begin_along(fp, q, u, v, 0, mk3(dm_u2f(rec.dx), dm_u2f(rec.dy), dm_u2f(rec.dz)));
                Surf per_sample;
                memset(&per_sample, 0, sizeof(per_sample));
                path_surf<GlobalPyramid<G>>(sc, h, q.d, per_sample);
                uint32_t a[sizeof(Surf) / 4], b[sizeof(Surf) / 4];
                static_assert(sizeof(Surf) % 4 == 0, "a shading point is 32-bit words");
                memcpy(a, &once, sizeof(Surf));
                memcpy(b, &per_sample, sizeof(Surf));
                for (size_t k = 0; k < sizeof(Surf) / 4; k++) n.surf_words += a[k] != b[k];
                n.surfaces++;
            }
            for (int sample = 0; sample < n_samples; sample++) {
                Path<false> pa, pb;
                const bool on_a = primary_vertex_sample<G, BLACK_SUN, CULL>(fp, sc, P, out_each, u, v, sample, rec, h, state, pa, c->ts);
                const bool on_b = primary_vertex_sample<G, BLACK_SUN, CULL, true>(fp, sc, P, out_shared, u, v, sample, rec, h, state, pb, c->ts, &once);
                n.samples++;
                if (on_a != on_b) { n.path_words++; continue; }
                if (!on_a) continue;
                n.sent_on++;
                uint32_t ea[PV_COUNT_SUN], eb[PV_COUNT_SUN];
                primary_cont_pack<false>(ea, pa);
                primary_cont_pack<false>(eb, pb);
                for (int k = 0; k < PV_COUNT_SUN; k++) n.path_words += ea[k] != eb[k];
                n.path_words += (pa.depth != pb.depth) + (pa.sky_primary != pb.sky_primary) + (dm_f2u(pa.refl_dist) != dm_f2u(pb.refl_dist));
                n.path_words += (dm_f2u(pa.contrib.x) != dm_f2u(pb.contrib.x)) + (dm_f2u(pa.contrib.y) != dm_f2u(pb.contrib.y)) + (dm_f2u(pa.contrib.z) != dm_f2u(pb.contrib.z));
            }
        }
    const size_t m = (size_t)stride * n_samples;
    const unsigned char *a[3] = {(const unsigned char*)each.color_d.data(), (const unsigned char*)each.color_s.data(), (const unsigned char*)each.refl.data()};
    const unsigned char *b[3] = {(const unsigned char*)shared.color_d.data(), (const unsigned char*)shared.color_s.data(), (const unsigned char*)shared.refl.data()};
    const size_t bytes[3] = {m * sizeof(f3), m * sizeof(f3), m * sizeof(float)};
    for (int k = 0; k < 3; k++)
        for (size_t i = 0; i < bytes[k]; i++) n.plane_bytes += a[k][i] != b[k][i];
}

template <int G>
static void ps_run(Emu* c, int n_samples, int cull, PsCounts& n) {
    FrameParams fp = frame_params(c);
    SceneData sc;
    memset(&sc, 0, sizeof(sc));
    sc.pyr.l0 = c->l0.data(); sc.pyr.l1 = c->l1.data(); sc.pyr.l2 = c->l2.data(); sc.pyr.l3 = c->l3.data();
    sc.pyr.l0c = c->l0c.data(); sc.pyr.l0c_base = c->l0c_base.data(); sc.pyr.l0c_count = c->l0c_base.data() + 512;
    sc.pyr.ref_oob = 0;
    sc.grid = c->grid.data(); sc.mats = c->mats.data();
    sc.sky.scattering = c->sky_scat.data(); sc.sky.transmittance = c->sky_trans.data();
    sc.sky.res = c->cfg.sky_res; sc.sky.fres = c->cfg.sky_res > 0 ? (float)(1.0 / (double)c->cfg.sky_res) : 0.0f;
    sc.counters = nullptr;
    sc.cull = c->cull + (cull ? 0 : 8);
    const bool black_sun = !((fp.light_color.x != 0.0f || fp.light_color.y != 0.0f || fp.light_color.z != 0.0f) && fp.light_weight != 0.0f);
    if (black_sun) { if (cull) ps_check<G, true, true>(c, fp, sc, n_samples, n); else ps_check<G, true, false>(c, fp, sc, n_samples, n); }
    else { if (cull) ps_check<G, false, true>(c, fp, sc, n_samples, n); else ps_check<G, false, false>(c, fp, sc, n_samples, n); }
}

extern "C" {
// Samples 0 .. n_samples-1 of every pixel through both forms (above).  counts[6]: pixels with a shading point, pixel-samples run, of them
// sent on; then what differs -- words of the shading point, words of the paths that go on, bytes of the stored planes.
int emu_primary_shared_check(Emu* c, int n_samples, int cull, unsigned long long* counts) {
    if (c->cfg.use_restir || c->cam.render_scale != 1.0f || n_samples < 1 || n_samples > 16) return VRT_E_INVALID;
    PsCounts n{0ULL, 0ULL, 0ULL, 0ULL, 0ULL, 0ULL};
    if (c->cfg.grid_res == 256) ps_run<256>(c, n_samples, cull, n); else ps_run<128>(c, n_samples, cull, n);
    counts[0] = n.surfaces; counts[1] = n.samples; counts[2] = n.sent_on; counts[3] = n.surf_words; counts[4] = n.path_words; counts[5] = n.plane_bytes;
    return 0;
}
}

#ifdef PRIMARY_SHARED_MAIN
#include <cstdio>
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
    Emu* c = emu_create(&cfg);
    if (!c) { fprintf(stderr, "emu_create failed\n"); return 2; }
    emu_upload_voxels(c, mat.data(), rgb.data());
    emu_upload_materials(c, table.data());
    emu_set_scene(c, &scene);
    emu_set_camera(c, &cam);
    emu_prepare(c);
    unsigned long long n[6] = {0};
    if (emu_primary_shared_check(c, (int)n_samples, 1, n) != 0) return 2;
    emu_destroy(c);
    printf("surfaces %llu samples %llu sent on %llu; words of the shading point that differ %llu, of the paths %llu, bytes of the planes %llu\n",
           n[0], n[1], n[2], n[3], n[4], n[5]);
    return (n[3] || n[4] || n[5]) ? 1 : 0;
}
#endif
