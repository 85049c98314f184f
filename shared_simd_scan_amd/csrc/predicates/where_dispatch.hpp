// predicates/where_dispatch.hpp -- host-side launch request of the shared scans over range / comparison predicates, shared
// by capi.hip and the where_group translation units (one per group of four widths, as width_group.hip).
#pragma once

#include "../dispatch.hpp"
#include "where.hpp"

namespace mi355 {

// kernel families of a shared where-scan (mi355_shared_where_kernel); P = 1 never comes here (the single-predicate scan)
enum WhereChoice { kWhereLut = 0, kWhereLutMulti = 1, kWhereChain = 2 };

struct WhereReq {
    LaunchReq l;  // c, stream, device, num_cus, max_blocks_per_cu, scan_nt_stores, record, choice_out; l.scan is not used
    WhereArgs w;  // what the kernel receives
};

MI355_DECLARE_GROUPS(launch_where_group_, WhereReq);

} // namespace mi355
