// vrt_query.h -- what a sampled query is: vrt_trace_radiance, vrt_gather_irradiance and vrt_gather_probes as three instances of one shape.  A sampled query
// takes n input records and n_samples, works on (record, sample) items -- item i of a launch is record i % n, sample s0 + i / n -- leaves
// each item's value in a scratch plane and folds the plane into one output record per input in sample order.  A traits struct names the
// record types and the plane's bound and gives the query's arithmetic (vrt_radiance.h, vrt_sensor.h, vrt_probe_sh.h: it stays there) one spelling;
// against it are written ONE fold kernel and ONE launcher (k_fold_query, launch_sampled_query: vrt_query_kernels.hip), ONE entry-point body
// (sampled_query: vrt_scene_ops.hip) and ONE host loop (query_block: tests/emul/query_emul.h).  What a query keeps for itself is its per-item
// header and the kernel that steps its items.  Plain structs of static functions, in the style of vrt_cast.h / vrt_radiance.h.
#pragma once
#include "vrt_radiance.h"
#include "vrt_sensor.h"
#include "vrt_probe_sh.h"
#include "vrt_plan.h"

namespace vrt {

struct RadianceQuery {
    typedef vrt_path_ray In;     // the caller's input record
    typedef f3 Item;             // an item's value in the scratch plane
    typedef f3 Sum;              // the running sums over a record's items
    typedef vrt_radiance Out;    // the caller's output record; between a call's chunks its rgb carries the running sum (t is the trace kernel's)
    static constexpr long long max_items = VRT_RADIANCE_ITEMS;   // of one launch: the plane's bound
    static constexpr bool has_reserved = true;                   // In has a `reserved` field the host path refuses unless 0
    static VRT_DEV Item zero() { return mk3(0.0f); }             // an item that is not traced
    static VRT_DEV Sum zero_sum() { return mk3(0.0f); }          // the sums before the first chunk
    static VRT_DEV Item sum_of(const Out& o) { return mk3(o.rgb[0], o.rgb[1], o.rgb[2]); }
    static VRT_DEV void keep_sum(Out& o, const Item& s) { o.rgb[0] = s.x; o.rgb[1] = s.y; o.rgb[2] = s.z; }
    static VRT_DEV Item fold(Item acc, const Item* values, long long stride, int count) { return radiance_fold(acc, values, stride, count); }
    static VRT_DEV Item mean(Item sum, int n_samples) { return radiance_mean(sum, n_samples); }
};

struct SensorQuery {
    typedef vrt_sensor In;
    typedef vrt_irradiance Item;   // the four terms of one sample
    typedef vrt_irradiance Sum;
    typedef vrt_irradiance Out;    // ... and their running sums
    static constexpr long long max_items = VRT_SENSOR_ITEMS;
    static constexpr bool has_reserved = true;
    static VRT_DEV Item zero() { return sensor_zero(); }
    static VRT_DEV Sum zero_sum() { return sensor_zero(); }
    static VRT_DEV Item sum_of(const Out& o) { return o; }
    static VRT_DEV void keep_sum(Out& o, const Item& s) { o = s; }
    static VRT_DEV Item fold(Item acc, const Item* values, long long stride, int count) { return sensor_fold(acc, values, stride, count); }
    static VRT_DEV Item mean(Item sum, int n_samples) { return sensor_mean(sum, n_samples); }
};

// The probes' item is not their sum: an item is the compact record of one sample (ProbeItem, 48 bytes), the sums are the 32 floats of the
// output record -- probe_fold forms the basis and the products on the way.
struct ProbeQuery {
    typedef vrt_probe In;
    typedef ProbeItem Item;
    typedef vrt_sh_probe Sum;
    typedef vrt_sh_probe Out;
    static constexpr long long max_items = VRT_PROBE_ITEMS;
    static constexpr bool has_reserved = false;
    static VRT_DEV Item zero() { return probe_item_zero(); }
    static VRT_DEV Sum zero_sum() { return probe_zero(); }
    static VRT_DEV Sum sum_of(const Out& o) { return o; }
    static VRT_DEV void keep_sum(Out& o, const Sum& s) { o = s; }
    static VRT_DEV Sum fold(Sum acc, const Item* values, long long stride, int count) { return probe_fold(acc, values, stride, count); }
    static VRT_DEV Sum mean(Sum sum, int n_samples) { return probe_mean(sum, n_samples); }
};

// One output record's part of a chunk: the chunk's `count` values of the record (values[s * stride]: the plane holds a sample's records
// side by side) added in sample order to the sum the chunks before left in `out` (first: to zero), and with the call's last chunk the
// division by its number of samples.  How the samples are cut into chunks cannot change a bit.
template <class Q>
VRT_DEV void query_fold(typename Q::Out& out, const typename Q::Item* values, long long stride, int count, bool first, bool last, int n_samples) {
    typename Q::Sum acc = first ? Q::zero_sum() : Q::sum_of(out);
    acc = Q::fold(acc, values, stride, count);
    if (last) acc = Q::mean(acc, n_samples);
    Q::keep_sum(out, acc);
}

}  // namespace vrt
