// vrt_probe.h -- TEST HOOK: one ray through the closest-hit walk, the way each render path runs it (vrt_trace_probe,
// include/vrt_api.h; the host build of tests/emul/emul.cpp steps the same function).  Only k_trace_probe calls it.
#ifndef VRT_PROBE_H
#define VRT_PROBE_H

#include "vrt_trace.h"
#include "vrt_pool.h"

namespace vrt {

// `mode` of vrt_trace_probe: the walk in its low two bits, PROBE_CULL_BOX on top
enum { PROBE_WALK_BRANCHY = 0,   // raytrace() with descend(): the fused kernel's walk, the dense variants' shadow rays
       PROBE_WALK_FLAT = 1,      // raytrace() with descend_flat(): shadow rays of the pooled kernel's SHADE stage
       PROBE_WALK_RECORD = 2,    // walk_prepare / walk_trip / walk_result through the packed slot fields: the pooled kernel's WALK stage
       PROBE_WALK_COUNT = 3,
       PROBE_CULL_BOX = 4 };     // test rays against the context's grown box (cull_ray); without it the box holds everything

struct ProbeOut { float dist; int cell[3]; float normal[3]; int iters; };   // the record of one ray in `out`: 32 bytes

template <int G, int WALK>
VRT_DEV void probe_ray(const GlobalPyramid<G>& P, f3 o, f3 d, const float* cull, ProbeOut& r) {
    TraceOut tr;
    int nq;
    if constexpr (WALK == PROBE_WALK_RECORD) {
        // as pool_launch_ray / the WALK stage / pool_shade pass a ray on: the loop-carried state goes through the slot's
        // packed fields when the walk is set up, every third step (a suspended walk) and when it ends.  The origin is
        // kept beside the slot: a slot holds the world position, the probe is given voxel units.
        uint32_t slot[PF_COUNT];
        for (int i = 0; i < PF_COUNT; i++) slot[i] = 0u;
        const SlotRef s{slot, 1};
        s.sv(PF_DIR, d);
        RayWalk w;
        const bool alive = walk_prepare<G, true>(o, d, w, cull);
        walk_store(s, w);
        walk_store_constants(s, w);
        if (alive) {
            BrickCache bc;
            bc.key = -1; bc.word = 0ULL;
            CoarseWords cw;
            walk_load<G>(s, w);
            w.o = o;
            coarse_fetch(P, w.ix, w.iy, w.iz, cw);
            for (int k = 1;; k++) {
                if (walk_trip(P, w, bc, cw, nq)) break;
                if (k % 3 == 0) {
                    walk_store(s, w);
                    walk_load<G>(s, w);
                    w.o = o;
                    bc.key = -1;
                    coarse_fetch(P, w.ix, w.iy, w.iz, cw);
                }
            }
            walk_store(s, w);
        }
        const uint32_t a = s.u(PF_CELL_XY), b = s.u(PF_CELL_Z);
        walk_result(d, s.f(PF_T), (int)(int16_t)(a & 0xffffu), (int)(int16_t)(a >> 16), (int)(int16_t)(b & 0xffffu), normal_decode(b >> 20),
                    (int)s.u(PF_ITERS), tr);
    } else {
        raytrace<GlobalPyramid<G>, WALK == PROBE_WALK_FLAT>(P, o, d, tr, nq, cull);
    }
    r.dist = tr.dist;
    r.cell[0] = tr.ix; r.cell[1] = tr.iy; r.cell[2] = tr.iz;
    r.normal[0] = tr.normal.x; r.normal[1] = tr.normal.y; r.normal[2] = tr.normal.z;
    r.iters = tr.iters;
}

}  // namespace vrt
#endif
