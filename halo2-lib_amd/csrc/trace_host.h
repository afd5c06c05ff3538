// The host prologue the device trace fills share (poseidon_trace.hip, range_fill.hip, fp_mul.hip, ec_fill.hip; gate_chains.hip takes the
// table packer alone): the checks of the column arguments, the address intervals a unit's run and its operands cover, the sweep that finds two
// of them at one address, and the upload of a call's small tables.  Host only.  An entry point reads: its parameters, a loop over the units
// (TraceRuns::run, operand_range), the clash checks, then pack_tables and the launches.  The fused fills (fp_mul.hip, ec_fill.hip,
// fp_cmp.hip, ec_select.hip) have all of that in one place, fused_fill at the end of this file.
#pragma once
#include "internal.h"
#include "trace_place.cuh"

namespace h2 {

// Address intervals [lo, hi) of the fills that write cells from operands lying in the same columns: the written intervals must be pairwise
// disjoint, and no operand interval (first to last address read, whatever the stride) may meet one.  Sorted (a layout engine's pieces mostly
// arrive sorted) and swept; nullptr when all is well, else the reason.
struct ByteRange {
    uintptr_t lo, hi;
    bool operator<(const ByteRange &o) const { return lo < o.lo; }
};
inline const char *byte_ranges_clash(std::vector<ByteRange> &written, std::initializer_list<std::vector<ByteRange> *> reads, const char *written_msg) {
    auto sorted = [](std::vector<ByteRange> &v) {
        if (!std::is_sorted(v.begin(), v.end())) std::sort(v.begin(), v.end());
    };
    sorted(written);
    const size_t count = written.size();
    for (size_t j = 1; j < count; ++j)
        if (written[j - 1].hi > written[j].lo) return written_msg;
    for (std::vector<ByteRange> *rd : reads) {
        sorted(*rd);
        size_t w = 0;
        for (const ByteRange &r : *rd) {
            while (w < count && written[w].hi <= r.lo) ++w;   // (the reads' starts ascend: what ends before this one ends before every later one)
            if (w < count && written[w].lo < r.hi) return "an operand range overlaps cells this call writes";
        }
    }
    return nullptr;
}
// The address intervals of a run of `cells` gate cells laid down from (column c, row r), appended to `written`: trace_place.cuh's walk with
// the columns' addresses and the usable rows in view, the copies at row 0 included.  nullptr when the run fits, else the reason.
// break_points: num_columns - 1 entries, each < usable_rows (TraceRuns::args_bad), or NULL.
inline const char *run_byte_ranges(void *const *columns_dev, size_t num_columns, size_t usable_rows, const uint32_t *break_points, size_t c, uint64_t r,
                                   uint64_t cells, std::vector<ByteRange> &written) {
    while (cells) {   // (zero only behind a break on the run's last cell)
        if (r >= usable_rows) return "a unit's cells leave the usable rows";
        const bool brk = break_points && c + 1 < num_columns && break_points[c] >= r;
        const uint64_t room = brk ? break_points[c] - r + 1 : usable_rows - r, take = cells < room ? cells : room;
        const uintptr_t w = (uintptr_t)columns_dev[c] + sizeof(Fr) * r;
        written.push_back(ByteRange{w, w + sizeof(Fr) * (uintptr_t)take});
        cells -= take;
        if (!brk || take < room) {
            if (cells) return break_points && c + 1 == num_columns ? "a unit's cells leave the last column" : "a unit's cells leave the usable rows";
            break;
        }
        // the cell at the break point was written: it is written again at row 0 of the next column, and the run goes on at row 1
        ++c;
        if (!columns_dev[c]) return "a unit's column index is out of range (or the column is NULL)";
        written.push_back(ByteRange{(uintptr_t)columns_dev[c], (uintptr_t)columns_dev[c] + sizeof(Fr)});
        r = 1;
    }
    return nullptr;
}

// the gate columns of one call as the host sees them, and what the call's units write into them.  Every function: nullptr, or the reason
struct TraceRuns {
    void *const *columns_dev;
    size_t num_columns, usable_rows;
    const uint32_t *break_points;
    std::vector<ByteRange> written;
    // the column, row and break-point arguments (rows_max: the fills that keep rows in 32 bits bound usable_rows)
    const char *args_bad(size_t rows_max = 0xFFFFFFFFu) const {
        if (num_columns < 1 || num_columns >= 0xFFFFFFFFu) return "num_columns out of range";
        if (usable_rows > rows_max) return "usable_rows out of range";
        if (break_points)
            for (size_t c = 0; c + 1 < num_columns; ++c)
                if (break_points[c] >= usable_rows) return "a break point >= usable_rows";
        return nullptr;
    }
    // one unit's run of `cells` cells from (column, row), column by column, as the kernel's TraceOut walks it
    const char *run(uint32_t column, uint32_t row, uint64_t cells) {
        if (column >= num_columns || !columns_dev[column]) return "a unit's column index is out of range (or the column is NULL)";
        return run_byte_ranges(columns_dev, num_columns, usable_rows, break_points, column, row, cells, written);
    }
};
// one operand: elements offset .. offset + span of the `len` elements at base, first to last address read.  false: it leaves them
inline bool operand_range(const void *base, size_t len, uint64_t offset, uint64_t span, std::vector<ByteRange> &reads) {
    if (offset >= len || span >= len - offset) return false;
    reads.push_back(ByteRange{(uintptr_t)base + sizeof(Fr) * offset, (uintptr_t)base + sizeof(Fr) * (offset + span + 1)});
    return true;
}

// A call's small tables: laid out in WS_TMP1 in the order given, each at a multiple of 256 bytes (one of no bytes takes no room), reserved
// once, uploaded through upload_jobs.  -> their device addresses and, from the COLUMNS and the BREAKS entry, the kernels' view of the columns
struct HostTable {
    const void *host;
    size_t bytes;
    enum Kind { PLAIN, COLUMNS, BREAKS } kind = PLAIN;   // COLUMNS: the gate columns' pointers; BREAKS: their break points
};
struct DevTables {
    char *at[6];
    TraceCols tc;
};
inline int pack_tables(h2hip_ctx *ctx, std::initializer_list<HostTable> tables, DevTables &out) {
    size_t end = 0, n = 0;
    for (const HostTable &t : tables)
        if (t.bytes) end = (end + 255) / 256 * 256 + t.bytes;
    char *base = nullptr;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_TMP1, end, (void **)&base));
    out.tc = TraceCols{nullptr, nullptr, 0};
    end = 0;
    for (const HostTable &t : tables) {
        char *dev = base + (end + 255) / 256 * 256;
        H2_CHK(upload_jobs(ctx, dev, t.host, t.bytes));
        if (t.kind == HostTable::COLUMNS) {
            out.tc.cols = (Fr *const *)dev;
            out.tc.last_col = t.bytes ? (uint32_t)(t.bytes / sizeof(void *) - 1) : 0;
        } else if (t.kind == HostTable::BREAKS && t.bytes)
            out.tc.bps = (const uint32_t *)dev;
        out.at[n++] = dev;
        end = (size_t)(dev - base) + t.bytes;
    }
    return H2HIP_OK;
}
inline HostTable columns_table(const TraceRuns &r) { return HostTable{r.columns_dev, sizeof(void *) * r.num_columns, HostTable::COLUMNS}; }
inline HostTable breaks_table(const TraceRuns &r) {
    return HostTable{r.break_points, r.break_points ? sizeof(uint32_t) * (r.num_columns - 1) : 0, HostTable::BREAKS};
}

// ---- the fused fills (fp_mul.hip, ec_fill.hip, fp_cmp.hip, ec_select.hip): a solve kernel, one lane per unit, leaves a record per unit; a place kernel, one
// lane per (unit, slot), writes the cells.  What a kind states of itself; fused_fill is everything between its *_prepare and its kernels.
struct FusedKind {
    const char *func;                            // the entry point, for the messages
    uint32_t cells, slots, results, record;      // per unit: the run with its gaps, the place kernel's lanes, results entries, Fr of the record
    struct {
        bool read;
        uint32_t span;                           // elements offset .. offset + span of values_dev
    } operand[3];                                // (a kind of two operands leaves the third unread)
    HostTable consts, segs;                      // segs: of no bytes for a kind without a segment table
    const char *solve_name, *place_name;         // for prof_begin
    uint32_t solve_block, place_block;
};
inline uint64_t unit_operand(const h2hip_fp_mul &u, int i) { return i == 0 ? u.a_offset : i == 1 ? u.b_offset : 0; }
inline uint64_t unit_operand(const h2hip_ec_op &u, int i) { return i == 0 ? u.p_offset : i == 1 ? u.q_offset : 0; }
inline uint64_t unit_operand(const h2hip_ec_select &u, int i) { return i == 0 ? u.p_offset : i == 1 ? u.q_offset : u.sel_offset; }

// Every check of the column arguments, the operands and the results, before anything is uploaded or launched; the records in WS_TMP2; the
// tables [units][column pointers][break points][constants]([segments]) in WS_TMP1; call's five leading members; then solve(grid, units,
// segs) and, behind it, place(grid, units, slots, lanes) launch on ctx->stream, each between prof_begin and prof_end.  units, segs: the
// tables' device addresses (solve stores segs in its call struct where the kind has a segment table: place's launch finds it there).
// count >= 1.
template <class Unit, class Solve, class Place>
int fused_fill(h2hip_ctx *ctx, void *const *columns_dev, size_t num_columns, size_t usable_rows, const uint32_t *break_points_host, const void *values_dev,
               size_t values_len, void *results_dev, size_t results_len, const Unit *units_host, size_t count, const FusedKind &kind, TraceCall &call,
               Solve solve, Place place) {
    H2_REQUIRE_AS(kind.func, count <= ((uint64_t)1 << 32) / kind.slots, "more than 2^32 lanes of the place kernel (count * the unit's slots) in one call");
    TraceRuns runs{columns_dev, num_columns, usable_rows, break_points_host};
    const char *bad = runs.args_bad();
    H2_REQUIRE_AS(kind.func, !bad, bad);
    H2_REQUIRE_AS(kind.func, values_len <= SIZE_MAX / sizeof(Fr) && results_len <= SIZE_MAX / sizeof(Fr), "values_len / results_len is no count of field elements");
    H2_REQUIRE_AS(kind.func, !results_dev || results_len / kind.results >= count, "results_len < count * the results of a unit");
    std::vector<ByteRange> reads;
    runs.written.reserve(count + 9);
    reads.reserve(((size_t)kind.operand[0].read + kind.operand[1].read + kind.operand[2].read) * count);
    for (size_t j = 0; j < count; ++j) {
        const Unit &u = units_host[j];
        bad = runs.run(u.column, u.row, kind.cells);   // the unit's whole run, gaps included
        H2_REQUIRE_AS(kind.func, !bad, bad);
        for (int i = 0; i < 3; ++i)
            H2_REQUIRE_AS(kind.func, !kind.operand[i].read || operand_range(values_dev, values_len, unit_operand(u, i), kind.operand[i].span, reads),
                          "a unit's operand lies outside values_len");
    }
    // two units' cells are disjoint; the results lie in none of them; no operand lies in anything written.  Address intervals, sorted and swept.
    bad = byte_ranges_clash(runs.written, {}, "two units' cells overlap (break copies and the range checks' gaps included)");
    H2_REQUIRE_AS(kind.func, !bad, bad);
    if (results_dev) runs.written.push_back(ByteRange{(uintptr_t)results_dev, (uintptr_t)results_dev + sizeof(Fr) * kind.results * count});
    bad = byte_ranges_clash(runs.written, {&reads}, "the results overlap cells this call writes");
    H2_REQUIRE_AS(kind.func, !bad, bad);
    DevTables t;
    Fr *rec = nullptr;
    H2_CHK(ws_reserve(ctx, h2hip_ctx::WS_TMP2, sizeof(Fr) * kind.record * count, (void **)&rec));
    H2_CHK(pack_tables(ctx, {{units_host, sizeof(Unit) * count}, columns_table(runs), breaks_table(runs), kind.consts, kind.segs}, t));
    call.tc = t.tc;
    call.values = (const Fr *)values_dev;
    call.consts = (const Fr *)t.at[3];
    call.results = (Fr *)results_dev;
    call.rec = rec;
    const Unit *units = (const Unit *)t.at[0];
    const uint64_t lanes = (uint64_t)count * kind.slots;
    prof_begin(ctx, kind.solve_name);
    solve(dim3((uint32_t)((count + kind.solve_block - 1) / kind.solve_block)), units, (const void *)t.at[4]);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    prof_begin(ctx, kind.place_name);
    place(dim3((uint32_t)((lanes + kind.place_block - 1) / kind.place_block)), units, kind.slots, lanes);
    prof_end(ctx);
    H2_HIPCHK(hipGetLastError());
    return H2HIP_OK;
}

}  // namespace h2
