// vrt_views.h -- the staged view of the pyramid that the render unit (vrt_kernels.hip) and the query unit (vrt_query_kernels.hip) share.
#ifndef VRT_VIEWS_H
#define VRT_VIEWS_H

#include "vrt_trace.h"

namespace vrt {

// OOB: the instantiation can read cells outside the grid the reference's way (oob_capable_of, vrt_trace.h).  It is the INSTRUMENTED
// instantiations that can (a context with vrt_set_reference_indexing launches those): the timed kernels carry no test for it.
template <int G_, bool OOB_ = false>
struct LdsPyramid {  // coarse levels in LDS, fine level through L2
    static constexpr int G = G_;
    static constexpr bool flat_descend = false;  // its kernels walk with few active lanes: descend()'s early outs win
    static constexpr bool cull = true;
    static constexpr bool oob_capable = OOB_;
    bool oob;   // wave-uniform: Pyramid::ref_oob
    __device__ __forceinline__ bool oob_ref() const { return oob; }
    const unsigned long long* l0;
    const unsigned long long* l1;
    const unsigned long long* l2;
    unsigned long long w3;   // the top word (G = 256), wave-uniform
    __device__ __forceinline__ unsigned long long load_l0(int i) const { return l0[i]; }
    __device__ __forceinline__ unsigned long long load_l1(int i) const { return l1[i]; }
    __device__ __forceinline__ unsigned long long load_l2(int i) const { return l2[i]; }
    __device__ __forceinline__ unsigned long long load_l3() const { return w3; }
};

}  // namespace vrt
#endif
