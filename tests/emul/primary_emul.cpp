// primary_emul.cpp -- TEST TOOLING: the camera-ray records of a launch made two ways on the host build of the device headers
// (tests/test_primary_records_host.py, tests/emul/primary_records_main.cpp):
//   * primary_record_walk() (voxel_rt2_amd/csrc/vrt_pool.h), what k_primary_records stores ahead of a launch;
//   * the pooled schedule as emul.cpp's render_all_pool steps it: BEGIN (pool_begin) into a slot, then the WALK stage over the
//     slot's packed fields, suspended into the slot and resumed every third step, and primary_record() of the slot where sample 0
//     leaves it -- in BEGIN when there was nothing to walk, else when the walk ends.
// Everything else -- the context, its pyramid, the frame parameters, the emu_* calls a session is driven through -- is emul.cpp's.
#include "emul.cpp"

template <int G, bool CULL>
static void primary_records_g(Emu* c, uint32_t tag, PrimaryRecord* by_walk, PrimaryRecord* by_schedule, uint8_t* walked) {
    const FrameParams fp = frame_params(c);
    GlobalPyramid<G> P;
    P.p.l0 = c->l0.data(); P.p.l1 = c->l1.data(); P.p.l2 = c->l2.data(); P.p.l3 = c->l3.data();
    P.p.l0c = c->l0c.data(); P.p.l0c_base = c->l0c_base.data(); P.p.l0c_count = c->l0c_base.data() + 512;
    P.p.ref_oob = 0;
    const float* cull = c->cull + (CULL ? 0 : 8);   // (make_scene_data, vrt_api.hip: the open box where the variant does not cull)
    for (int v = fp.row0; v < fp.row1; v++)
        for (int u = 0; u < fp.W; u++) {
            if (outside_render_area(fp, (float)u, (float)v)) continue;
            const int idx = (v - fp.row0) * fp.W + u;
            by_walk[idx] = primary_record_walk<G, CULL>(fp, P, cull, u, v, tag);
            uint32_t slot[PF_COUNT] = {0};
            SlotRef s{slot, 1};
            TraceStats ts;
            stats_zero(ts);
            const int st = pool_begin<G, CULL>(fp, cull, s, u, v, 0, ts);
            walked[idx] = st == SLOT_RAY ? 1 : 0;
            if (st == SLOT_RAY) {
                RayWalk w;
                walk_load<G>(s, w);
                BrickCache bc{-1, 0ULL};
                CoarseWords cw;
                coarse_fetch(P, w.ix, w.iy, w.iz, cw);
                for (int k = 1;; k++) {
                    int nq;
                    if (walk_trip(P, w, bc, cw, nq)) break;
                    if (k % 3 == 0) { walk_store(s, w); walk_load<G>(s, w); bc.key = -1; coarse_fetch(P, w.ix, w.iy, w.iz, cw); }
                }
                walk_store(s, w);
            }
            by_schedule[idx] = primary_record(s, tag);
        }
}

extern "C" {

// by_walk, by_schedule: (buf1 - buf0) x W records of 8 words, rows from the context's first buffered row (left alone outside the
// render area); walked: 1 where BEGIN found something to walk.  cull: the variant's (the scene's grown box, or the open one).
int emu_primary_records(Emu* c, int cull, uint32_t tag, void* by_walk, void* by_schedule, uint8_t* walked) {
    if (!c || !by_walk || !by_schedule || !walked) return VRT_E_INVALID;
    PrimaryRecord* a = (PrimaryRecord*)by_walk;
    PrimaryRecord* b = (PrimaryRecord*)by_schedule;
    if (c->cfg.grid_res == 256) { if (cull) primary_records_g<256, true>(c, tag, a, b, walked); else primary_records_g<256, false>(c, tag, a, b, walked); }
    else { if (cull) primary_records_g<128, true>(c, tag, a, b, walked); else primary_records_g<128, false>(c, tag, a, b, walked); }
    return 0;
}
int emu_primary_record_valid(const void* rec, uint32_t tag) { return primary_record_valid(*(const PrimaryRecord*)rec, tag) ? 1 : 0; }

}  // extern "C"
