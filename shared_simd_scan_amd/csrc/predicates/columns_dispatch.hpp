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

hipError_t launch_columns_group_0(const ColumnsReq &);
hipError_t launch_columns_group_1(const ColumnsReq &);
hipError_t launch_columns_group_2(const ColumnsReq &);
hipError_t launch_columns_group_3(const ColumnsReq &);
hipError_t launch_columns_group_4(const ColumnsReq &);
hipError_t launch_columns_group_5(const ColumnsReq &);
hipError_t launch_columns_group_6(const ColumnsReq &);
hipError_t launch_columns_group_7(const ColumnsReq &);

} // namespace mi355
