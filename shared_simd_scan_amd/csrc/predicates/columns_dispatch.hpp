// predicates/columns_dispatch.hpp -- host-side launch request of the column-against-column scan, shared by capi.hip and the
// columns_group translation units (one per group of four widths of column 1, as where_group.hip).
#pragma once

#include "../dispatch.hpp"
#include "columns.hpp"

namespace mi355 {

struct ColumnsReq {
    LaunchReq l;   // c (column 1's width), stream, device, num_cus, max_blocks_per_cu, scan_nt_stores, record; l.scan is not used
    ColumnsArgs k; // what the kernel receives
};

MI355_DECLARE_GROUPS(launch_columns_group_, ColumnsReq);

} // namespace mi355
