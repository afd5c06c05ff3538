// h2hip_trace_seek: trace_place.cuh's walk for a caller that lays out cells of its own behind a fill's (include/h2hip.h states the form).
// Host only, pure: no context, no device.
#include "internal.h"
#include "trace_place.cuh"

using namespace h2;

extern "C" int h2hip_trace_seek(const uint32_t *break_points_host, size_t num_columns, uint32_t column, uint32_t row, uint64_t offset, uint32_t *column_out,
                                uint32_t *row_out) {
    H2_REQUIRE(column_out && row_out, "NULL argument");
    H2_REQUIRE(column < num_columns, "the column index is out of range");
    // (more than 2^32 columns: the walk never reaches the last one's index)
    trace_walk(break_points_host, (uint32_t)std::min<size_t>(num_columns - 1, 0xFFFFFFFFu), column, row, offset);
    H2_REQUIRE(offset <= 0xFFFFFFFFull - row, "the cell lies past every row");
    *column_out = column;
    *row_out = (uint32_t)(row + offset);
    return H2HIP_OK;
}
