// Where the cells of a run go: assign_witnesses' walk down a column (threads/single_phase.rs:273-312), as host and device code.  Down the
// column; the cell written at the column's break point is written again at row 0 of the next column and the run goes on at row 1 (the copy
// itself is never a break cell: assign_witnesses goes on at row 1 without looking).  The one statement of the rule: the fills' kernels write
// through TraceOut, h2hip_trace_seek (trace_place.hip) reports trace_walk's result, trace_host.h's run_byte_ranges is the host's view of it.
#pragma once
#include "internal.h"

namespace h2 {

// the gate columns of one call: last_col break points (or NULL: no column breaks), the last column never breaks
struct TraceCols {
    Fr *const *cols;
    const uint32_t *bps;
    uint32_t last_col;
};
// what the call structs of the fused fills (FpCall, EcCall, CmpCall) begin with, as their base: trace_host.h's fused_fill sets these five
struct TraceCall {
    TraceCols tc;
    const Fr *values, *consts;
    Fr *results, *rec;
};
// A kernel argument's words stay where they are (one moved word has cost SGPRs and the alignment of the modulus words): each call struct
// states the offset of every member.  (offsetof through a base is conditionally supported; the compilers this builds with support it)
#define H2_OFFSET_IS(Call, member, at)                                                          \
    _Pragma("clang diagnostic push") _Pragma("clang diagnostic ignored \"-Winvalid-offsetof\"") \
    static_assert(offsetof(Call, member) == (at), #Call "." #member " moved");                  \
    _Pragma("clang diagnostic pop")
#define H2_CALL_LEADS(Call)        \
    H2_OFFSET_IS(Call, tc, 0)      \
    H2_OFFSET_IS(Call, values, 24) \
    H2_OFFSET_IS(Call, consts, 32) \
    H2_OFFSET_IS(Call, results, 40) \
    H2_OFFSET_IS(Call, rec, 48)

constexpr uint32_t TRACE_NO_BREAK = 0xFFFFFFFFu;
// the cells from `row` up to and including the break cell of column `col` (a unit has fewer than 2^31 cells: without a break ahead the
// count never reaches zero)
H2_HD bool trace_break_ahead(const uint32_t *bps, uint32_t last_col, uint32_t col, uint32_t row) { return bps && col < last_col && bps[col] >= row; }
H2_HD uint32_t trace_left(const uint32_t *bps, uint32_t last_col, uint32_t col, uint32_t row) {
    return trace_break_ahead(bps, last_col, col, row) ? bps[col] - row + 1 : TRACE_NO_BREAK;
}
// (col, row, off) <- the column of cell `off` of the run that starts at (col, row), the row the run enters that column at, and the cell's
// distance from there; whole columns at a time, no column is touched.  -> trace_left at (col, row)
template <class Off>
H2_HD uint32_t trace_walk(const uint32_t *bps, uint32_t last_col, uint32_t &col, uint32_t &row, Off &off) {
    for (;;) {
        const uint32_t left = trace_left(bps, last_col, col, row);
        if (!trace_break_ahead(bps, last_col, col, row) || off < left) return left;   // (Off may have 64 bits: h2hip_trace_seek's)
        off -= left;
        ++col;
        row = 1;
    }
}

// a lane's position in its run: p = the next cell, left = trace_left there
struct TraceOut {
    TraceCols tc;
    Fr *p;
    uint32_t col, left;
    H2_HD void seek(uint32_t row) {
        p = tc.cols[col] + row;
        left = trace_left(tc.bps, tc.last_col, col, row);
    }
    H2_HD void put(const Fr &v) {
        *p++ = v;
        if (--left == 0) {
            ++col;
            tc.cols[col][0] = v;
            seek(1);
        }
    }
};
// at the first cell of the run that starts at (col, row)
H2_HD TraceOut trace_at(const TraceCols &tc, uint32_t col, uint32_t row) {
    TraceOut o;
    o.tc = tc;
    o.col = col;
    o.seek(row);
    return o;
}
// at cell `off` of that run (on a break cell: its first position)
H2_HD TraceOut trace_at(const TraceCols &tc, uint32_t col, uint32_t row, uint32_t off) {
    TraceOut o;
    o.tc = tc;
    o.left = trace_walk(tc.bps, tc.last_col, col, row, off);
    o.col = col;
    o.p = tc.cols[col] + row + off;
    if (o.left != TRACE_NO_BREAK) o.left -= off;
    return o;
}

}  // namespace h2
