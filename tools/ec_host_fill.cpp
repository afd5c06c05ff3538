// tools/ec_time.py's host side (side (b) of DESIGN 3m's measurement): h2hip_ec_fill_dev's cells and the cells of the 9 k range checks computed on ONE host thread with the library's
// host field and the library's own per-unit and per-segment code (csrc/ec_fill.cuh, csrc/range_fill.cuh), into host columns, from points in
// host memory — what a caller had to do with the cells before the device fill existed, short of writing big integers of its own.  Built by
// the tool (hipcc, host only); not part of libh2hip.
//
// With -DEC_SELFTEST the file is a stand-alone program (its own main; build it with -fsanitize=address,undefined): it runs the same code over
// pools of coordinates (0, 1, 2, p - 1, p, 2^(n k) - 1, 3^i mod 2^(n k), one improper limb 2^n) for the tests' parameter sets and moduli and
// the three operations, and checks what must hold whatever the integers are: x3, y3, lambda < p from their limb cells; every subtraction's, addition's and
// scalar product's gate; every carry gate check_i + (-c_i) 2^n = -c_{i-1} of the two carry_mods where the coordinates are reduced; every own cell written, every gap
// and every cell outside the run untouched.
#include <stdlib.h>

#include "../halo2-lib_amd/csrc/ec_fill.cuh"
#include "../halo2-lib_amd/csrc/fp_cmp.cuh"

using namespace h2;

template <int K, uint32_t OP>
static void solve_all(const EcCall &ec, const h2hip_ec_op *units, size_t count) {
    for (size_t u = 0; u < count; ++u) ec_solve_unit<K, OP>(ec, units[u], (uint32_t)u);
}

// lookup_columns_host == NULL: the own cells only.  results: count (9 k + 3) elements (needed).  -> 0, or 1 when the parameters are refused
extern "C" int ec_host_fill(void *const *columns_host, size_t num_columns, const uint32_t *break_points, void *const *lookup_columns_host,
                            size_t num_lookup_columns, const h2hip_fp_params *params, uint32_t op, const void *values_host, void *results_host,
                            const h2hip_ec_op *units, const uint64_t *lookup_slots, size_t count) {
    EcShape sh;
    EcCall ec;
    Fr consts[EC_CONSTS];
    if (ec_prepare(*params, op, sh, &ec, consts)) return 1;
    const uint32_t k = sh.k;
    std::vector<Fr> rec((size_t)ec_record_len(k) * count);
    ec.tc = TraceCols{(Fr *const *)columns_host, break_points, (uint32_t)(num_columns - 1)};
    ec.values = (const Fr *)values_host;
    ec.consts = consts;
    ec.segs = sh.segs;
    ec.results = (Fr *)results_host;
    ec.rec = rec.data();
    if (k == 3 && op == H2HIP_EC_SUB_UNEQUAL)
        solve_all<3, H2HIP_EC_SUB_UNEQUAL>(ec, units, count);
    else if (op == H2HIP_EC_SUB_UNEQUAL)
        solve_all<4, H2HIP_EC_SUB_UNEQUAL>(ec, units, count);
    else if (k == 3 && op == H2HIP_EC_ADD_UNEQUAL)
        solve_all<3, H2HIP_EC_ADD_UNEQUAL>(ec, units, count);
    else if (k == 3)
        solve_all<3, H2HIP_EC_DOUBLE>(ec, units, count);
    else if (op == H2HIP_EC_ADD_UNEQUAL)
        solve_all<4, H2HIP_EC_ADD_UNEQUAL>(ec, units, count);
    else
        solve_all<4, H2HIP_EC_DOUBLE>(ec, units, count);
    for (size_t u = 0; u < count; ++u)
        for (uint32_t s = 0; s < sh.nsegs; ++s) ec_place_slot(ec, units[u], (uint32_t)u, s);
    if (!lookup_columns_host) return 0;
    uint64_t lk_before = 0;
    for (uint32_t j = 0; j < sh.ngaps; ++j) {   // the 9 k range checks per unit, gap by gap in context order
        RangeCall rc;
        std::vector<Fr> pows;
        if (range_prepare(sh.gaps[j].range_bits, sh.fp.lb, 0, 0, rc, &pows)) return 1;
        rc.tc = ec.tc;
        rc.lk_cols = (Fr *const *)lookup_columns_host;
        rc.values = (const Fr *)results_host;
        rc.num_lk_cols = (uint32_t)num_lookup_columns;
        for (size_t u = 0; u < count; ++u) {
            const TraceOut at = trace_at(ec.tc, units[u].column, units[u].row, sh.gaps[j].cell_offset);
            const h2hip_range_check chk{at.col, (uint32_t)(at.p - ec.tc.cols[at.col]), u * ec_result_len(k) + sh.gaps[j].result_index, 0, lookup_slots[u] + lk_before};
            for (uint32_t s = 0; s < range_unit_slots(rc.L, rc.rem); ++s) range_slot(rc, chk, s);
        }
        lk_before += sh.gap_lookups[j];
    }
    return 0;
}

// the same for h2hip_fp_cmp_fill_dev's unit (the comparison in front of a strict operation): its own cells by cmp_solve_unit / cmp_place_slot, the
// cells of its range checks by range_slot.  results: count results_per_unit elements (needed).  -> 0, or 1 when the parameters are refused
extern "C" int cmp_host_fill(void *const *columns_host, size_t num_columns, const uint32_t *break_points, void *const *lookup_columns_host,
                             size_t num_lookup_columns, const h2hip_fp_params *params, uint32_t op, const void *values_host, void *results_host,
                             const h2hip_fp_mul *units, const uint64_t *lookup_slots, size_t count) {
    CmpShape sh;
    CmpCall cc;
    Fr consts[CMP_CONSTS];
    if (cmp_prepare(*params, op, sh, &cc, consts)) return 1;
    const uint32_t k = sh.k, nres = cmp_result_len(k, op);
    std::vector<Fr> rec((size_t)cmp_record_len(k) * count);
    cc.tc = TraceCols{(Fr *const *)columns_host, break_points, (uint32_t)(num_columns - 1)};
    cc.values = (const Fr *)values_host;
    cc.consts = consts;
    cc.segs = sh.segs;
    cc.results = (Fr *)results_host;
    cc.rec = rec.data();
    for (size_t u = 0; u < count; ++u) cmp_solve_unit(cc, units[u], (uint32_t)u);
    for (size_t u = 0; u < count; ++u)
        for (uint32_t s = 0; s < sh.nsegs; ++s) cmp_place_slot(cc, units[u], (uint32_t)u, s);
    if (!lookup_columns_host || !sh.ngaps) return 0;
    RangeCall rc;
    std::vector<Fr> pows;
    if (range_prepare(sh.width, sh.fp.lb, 0, 0, rc, &pows)) return 1;
    rc.tc = cc.tc;
    rc.lk_cols = (Fr *const *)lookup_columns_host;
    rc.values = (const Fr *)results_host;
    rc.num_lk_cols = (uint32_t)num_lookup_columns;
    for (size_t u = 0; u < count; ++u)
        for (uint32_t j = 0; j < sh.ngaps; ++j) {
            const TraceOut at = trace_at(cc.tc, units[u].column, units[u].row, sh.gaps[j].cell_offset);
            const h2hip_range_check chk{at.col, (uint32_t)(at.p - cc.tc.cols[at.col]), u * nres + sh.gaps[j].result_index, 0, lookup_slots[u] + (uint64_t)j * sh.gap_lookups_each};
            for (uint32_t s = 0; s < range_unit_slots(rc.L, rc.rem); ++s) range_slot(rc, chk, s);
        }
    return 0;
}

#ifdef EC_SELFTEST
static void from_words(const uint32_t *w, uint32_t n, uint32_t k, Fr *out) {   // the k limbs and the native residue of an integer of 12 words
    uint32_t x[12];
    memcpy(x, w, sizeof x);
    Fr nat = Fr::zero();
    for (uint32_t i = 0; i < k; ++i) {
        Fr c = Fr::zero();
        for (int j = 0; j < 4; ++j) c.l[j] = x[j];
        out[i] = fe_to_mont(range_low_bits(c, n));
        nat = fe_add(nat, fe_mul(out[i], pow2_mont(n * i)));
        const uint32_t ws = n >> 5, s = n & 31;
        for (uint32_t j = 0; j < 12; ++j) {
            const uint32_t lo = j + ws < 12 ? x[j + ws] : 0, hi = j + ws + 1 < 12 ? x[j + ws + 1] : 0;
            x[j] = s ? (lo >> s) | (hi << (32 - s)) : lo;
        }
    }
    out[k] = nat;
}
static int fails = 0;
#define EXPECT(cond, ...)                \
    do {                                 \
        if (!(cond)) {                   \
            ++fails;                     \
            fprintf(stderr, __VA_ARGS__); \
        }                                \
    } while (0)

int main() {
    static const char *moduli[3] = {"fffffffffffffffffffffffffffffffffffffffffffffffffffffffefffffc2f", "fffffffffffffffffffffffffffffffebaaedce6af48a03bbfd25e8cd0364141",
                                    "30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47"};
    static const uint32_t sets[4][3] = {{88, 3, 8}, {88, 3, 18}, {90, 3, 15}, {64, 4, 8}};
    const Fr sentinel = pow2_mont(253);   // (no cell of a unit holds 2^253)
    size_t units_run = 0;
    for (const auto &set : sets)
        for (const char *hex : moduli)
            for (const uint32_t op : {(uint32_t)H2HIP_EC_ADD_UNEQUAL, (uint32_t)H2HIP_EC_DOUBLE, (uint32_t)H2HIP_EC_SUB_UNEQUAL}) {
                const uint32_t n = set[0], k = set[1], k1 = k + 1;
                h2hip_fp_params pr;
                memset(&pr, 0, sizeof pr);
                pr.limb_bits = n;
                pr.num_limbs = k;
                pr.lookup_bits = set[2];
                for (int i = 0; i < 32; ++i) {
                    unsigned byte = 0;
                    sscanf(hex + 62 - 2 * i, "%2x", &byte);
                    pr.modulus[i] = (uint8_t)byte;
                }
                EcShape sh;
                const char *bad = ec_prepare(pr, op, sh, nullptr, nullptr);
                EXPECT(!bad, "refused: %s\n", bad ? bad : "");
                if (bad) continue;
                // coordinates: 0, 1, 2, p - 1, p, 2^(n k) - 1, then 3^(40 i) mod 2^(n k) for i < 6
                uint32_t pool[12][12];
                memset(pool, 0, sizeof pool);
                pool[1][0] = 1;
                pool[2][0] = 2;
                memcpy(pool[3], pr.modulus, 48);
                pool[3][0] -= 1;
                memcpy(pool[4], pr.modulus, 48);
                for (uint32_t b = 0; b < n * k; ++b) pool[5][b >> 5] |= 1u << (b & 31);
                uint32_t acc[12] = {1};
                for (int e = 6; e < 12; ++e) {
                    for (int t = 0; t < 40 * (e - 4); ++t) {
                        uint64_t c = 0;
                        for (int j = 0; j < 12; ++j) {
                            c += (uint64_t)acc[j] * 3;
                            acc[j] = (uint32_t)c;
                            c >>= 32;
                        }
                    }
                    for (int j = 0; j < 12; ++j) pool[e][j] = acc[j] & pool[5][j];
                }
                std::vector<Fr> values;
                std::vector<h2hip_ec_op> units;
                std::vector<char> reduced;   // every coordinate of the unit is one of 0, 1, 2, p - 1
                const uint32_t cells = sh.total;
                Fr pt[4 * (FP_MAX_K + 1)];
                for (int a = 0; a < 12; ++a)
                    for (int b = 0; b < 12; b += 1 + (a % 3)) {
                        from_words(pool[a], n, k, pt);
                        from_words(pool[(a + b) % 12], n, k, pt + k1);
                        from_words(pool[b], n, k, pt + 2 * k1);
                        from_words(pool[(a * b + 7) % 12], n, k, pt + 3 * k1);
                        h2hip_ec_op u;
                        u.column = 0;
                        u.row = 2 + (uint32_t)units.size() * (cells + 1);
                        u.p_offset = values.size();
                        u.q_offset = values.size() + 2 * k1;
                        values.insert(values.end(), pt, pt + 4 * k1);
                        units.push_back(u);
                        reduced.push_back(a < 4 && (a + b) % 12 < 4 && b < 4 && (a * b + 7) % 12 < 4);
                    }
                values[units[0].p_offset + 1] = pow2_mont(n);   // an improper limb: 2^n
                reduced[0] = 0;
                const size_t count = units.size(), rows = 2 + count * (cells + 1) + 3;
                std::vector<Fr> column(rows, sentinel), results(count * ec_result_len(k), sentinel);
                void *cols[1] = {column.data()};
                EXPECT(ec_host_fill(cols, 1, nullptr, nullptr, 0, &pr, op, values.data(), results.data(), units.data(), nullptr, count) == 0, "the fill refused\n");
                std::vector<char> own(cells, 1);
                for (uint32_t j = 0; j < sh.ngaps; ++j)
                    for (uint32_t c = 0; c < sh.gaps[j].num_cells; ++c) own[sh.gaps[j].cell_offset + c] = 0;
                size_t written = 0;
                for (size_t r = 0; r < rows; ++r) written += column[r] != sentinel;
                EXPECT(written == count * sh.own, "%zu cells written, %zu own cells\n", written, count * (size_t)sh.own);
                uint32_t pw[12];
                memcpy(pw, pr.modulus, 48);
                for (size_t u = 0; u < count; ++u) {
                    const Fr *run = column.data() + units[u].row;
                    for (uint32_t c = 0; c < cells; ++c) EXPECT((run[c] != sentinel) == (own[c] != 0), "unit %zu cell %u: own / gap mismatch\n", u, c);
                    const Fr *res = results.data() + u * ec_result_len(k);
                    for (uint32_t v = 0; v < 3; ++v) {   // x3, y3, lambda < p from their limbs' cells: recompose into words
                        uint32_t O[12] = {0};
                        for (uint32_t i = k; i-- > 0;) {
                            const uint32_t ws = n >> 5, s = n & 31;
                            for (int j = 11; j >= 0; --j) {
                                const uint32_t hi = j >= (int)ws ? O[j - ws] : 0, lo = j >= (int)ws + 1 ? O[j - ws - 1] : 0;
                                O[j] = s ? (hi << s) | (lo >> (32 - s)) : hi;
                            }
                            const Fr c = fe_from_mont(res[v * k1 + i]);
                            for (int j = 0; j < 4; ++j) O[j] |= c.l[j];
                        }
                        unsigned br = 0;
                        for (int j = 0; j < 12; ++j) subb32(O[j], pw[j], br);
                        EXPECT(br == 1, "unit %zu: value %u >= p\n", u, v);
                    }
                    for (uint32_t s = 0; s < sh.nsegs; ++s) {
                        const EcSeg &sg = sh.segs[s];
                        const Fr *c = run + sg.off;
                        if (sg.type == EC_SUB || sg.type == EC_ADD || sg.type == EC_SMUL)
                            for (uint32_t j = 0; j <= k; ++j) EXPECT(fe_add(c[4 * j], fe_mul(c[4 * j + 1], c[4 * j + 2])) == c[4 * j + 3], "unit %zu segment %u: gate %u\n", u, s, j);
                        if (sg.type == EC_CARRY && sg.red >= 1 && reduced[u]) {   // (the zero check has a remainder where the denominator is 0)
                            EXPECT(fe_add(c[0], fe_mul(c[1], c[2])) == c[3], "unit %zu segment %u: the carry does not divide exactly\n", u, s);
                            EXPECT(fe_add(c[4], fe_mul(c[5], c[6])) == c[7], "unit %zu segment %u: the shifted carry\n", u, s);
                        }
                    }
                }
                // once more with the range checks (range_prepare's RangeCall per gap): every cell of every run and every lookup cell written
                std::vector<Fr> lk(count * sh.num_lookups + 1, sentinel);
                std::vector<uint64_t> lk_slots(count);
                for (size_t u = 0; u < count; ++u) lk_slots[u] = u * sh.num_lookups;
                void *lks[1] = {lk.data()};
                EXPECT(ec_host_fill(cols, 1, nullptr, lks, 1, &pr, op, values.data(), results.data(), units.data(), lk_slots.data(), count) == 0, "the fill with range checks refused\n");
                size_t filled = 0, looked = 0;
                for (size_t r = 0; r < rows; ++r) filled += column[r] != sentinel;
                for (const Fr &c : lk) looked += c != sentinel;
                EXPECT(filled == count * cells && looked + 1 == lk.size() && lk.back() == sentinel, "%zu cells and %zu lookup cells written with the range checks\n", filled, looked);
                units_run += count;
            }
    // ---- the comparison unit: every mask over pairs of the same coordinates and of limbs that are no limbs; what must hold whatever the cells
    // are: every own cell written, every gap and every cell outside the run untouched; each gate of gate.add / is_less_than / gate.sub /
    // is_zero / gate.and; with the range checks every cell of every run and every lookup cell written, and l_i is the range fill's last limb
    size_t cmp_units_run = 0;
    for (const auto &set : sets)
        for (const char *hex : moduli)
            for (uint32_t op = 1; op < 8; ++op) {
                const uint32_t n = set[0], k = set[1], k1 = k + 1;
                h2hip_fp_params pr;
                memset(&pr, 0, sizeof pr);
                pr.limb_bits = n;
                pr.num_limbs = k;
                pr.lookup_bits = set[2];
                for (int i = 0; i < 32; ++i) {
                    unsigned byte = 0;
                    sscanf(hex + 62 - 2 * i, "%2x", &byte);
                    pr.modulus[i] = (uint8_t)byte;
                }
                CmpShape sh;
                const char *bad = cmp_prepare(pr, op, sh, nullptr, nullptr);
                EXPECT(!bad, "refused: %s\n", bad ? bad : "");
                if (bad) continue;
                uint32_t pool[8][12];
                memset(pool, 0, sizeof pool);
                pool[1][0] = 1;
                memcpy(pool[2], pr.modulus, 48);
                pool[2][0] -= 1;
                memcpy(pool[3], pr.modulus, 48);
                memcpy(pool[4], pr.modulus, 48);
                pool[4][0] += 1;
                for (uint32_t b = 0; b < n * k; ++b) pool[5][b >> 5] |= 1u << (b & 31);
                memcpy(pool[6], pr.modulus, 48);
                pool[6][n >> 5] ^= 1u << (n & 31);   // p with bit 0 of limb 1 flipped
                for (int j = 0; j < 12; ++j) pool[7][j] = (0x9E3779B9u * (j + 1)) & pool[5][j];
                std::vector<Fr> values;
                std::vector<h2hip_fp_mul> units;
                const uint32_t cells = sh.total, nres = cmp_result_len(k, op);
                Fr x[2 * (FP_MAX_K + 1)];
                for (int a = 0; a < 8; ++a)
                    for (int b = 0; b < 8; ++b) {
                        from_words(pool[a], n, k, x);
                        from_words(pool[b], n, k, x + k1);
                        if (a == 7 && b < 4) x[b % k] = b == 0 ? pow2_mont(n) : b == 1 ? pow2_mont(sh.pad) : b == 2 ? fe_sub(pow2_mont(sh.width), Fr::one()) : fe_neg(Fr::one());
                        h2hip_fp_mul u;
                        u.column = 0;
                        u.row = 2 + (uint32_t)units.size() * (cells + 1);
                        u.a_offset = values.size();
                        u.b_offset = values.size() + k1;
                        values.insert(values.end(), x, x + 2 * k1);
                        units.push_back(u);
                    }
                const size_t count = units.size(), rows = 2 + count * (cells + 1) + 3;
                std::vector<Fr> column(rows, sentinel), results(count * nres, sentinel);
                void *cols[1] = {column.data()};
                EXPECT(cmp_host_fill(cols, 1, nullptr, nullptr, 0, &pr, op, values.data(), results.data(), units.data(), nullptr, count) == 0, "the comparison fill refused\n");
                std::vector<char> own(cells, 1);
                for (uint32_t j = 0; j < sh.ngaps; ++j)
                    for (uint32_t c = 0; c < sh.gaps[j].num_cells; ++c) own[sh.gaps[j].cell_offset + c] = 0;
                size_t written = 0;
                for (size_t r = 0; r < rows; ++r) written += column[r] != sentinel;
                EXPECT(written == count * sh.own, "%zu cells written, %zu own cells\n", written, count * (size_t)sh.own);
                for (const Fr &r : results) EXPECT(r != sentinel, "a results entry was not written\n");
                const auto gate = [](const Fr *c) { return fe_add(c[0], fe_mul(c[1], c[2])) == c[3]; };
                for (size_t u = 0; u < count; ++u) {
                    const Fr *run = column.data() + units[u].row;
                    for (uint32_t c = 0; c < cells; ++c) EXPECT((run[c] != sentinel) == (own[c] != 0), "comparison unit %zu cell %u: own / gap mismatch\n", u, c);
                    for (uint32_t s = 0; s < sh.nsegs; ++s) {
                        const CmpSeg &sg = sh.segs[s];
                        const Fr *c = run + sg.off;
                        if (sg.type == CMP_LT) {
                            if (sg.i) {
                                EXPECT(gate(c), "comparison unit %zu segment %u: the borrow's add\n", u, s);
                                c += 4;
                            }
                            EXPECT(gate(c) && gate(c + 3), "comparison unit %zu segment %u: is_less_than's gates\n", u, s);
                        } else {
                            if (sg.type == CMP_EQ) {
                                EXPECT(gate(c), "comparison unit %zu segment %u: the sub\n", u, s);
                                c += 4;
                            }
                            EXPECT(gate(c) && gate(c + 4) && c[0] == c[6] && c[3] == Fr::one(), "comparison unit %zu segment %u: is_zero\n", u, s);
                            if (sg.type == CMP_EQ && sg.i) EXPECT(gate(c + 8), "comparison unit %zu segment %u: the and\n", u, s);
                        }
                    }
                }
                std::vector<Fr> lk(count * sh.num_lookups + 1, sentinel);
                std::vector<uint64_t> lk_slots(count);
                for (size_t u = 0; u < count; ++u) lk_slots[u] = u * sh.num_lookups;
                void *lks[1] = {lk.data()};
                EXPECT(cmp_host_fill(cols, 1, nullptr, lks, 1, &pr, op, values.data(), results.data(), units.data(), lk_slots.data(), count) == 0, "the comparison fill with range checks refused\n");
                size_t filled = 0, looked = 0;
                for (size_t r = 0; r < rows; ++r) filled += column[r] != sentinel;
                for (const Fr &c : lk) looked += c != sentinel;
                EXPECT(filled == count * cells && looked + 1 == lk.size() && lk.back() == sentinel, "%zu cells and %zu lookup cells written with the comparison's range checks\n", filled, looked);
                for (size_t u = 0; u < count; ++u)   // is_zero's cell is the copy of the range check's last limb cell (three cells before the gap's end)
                    for (uint32_t j = 0; j < sh.ngaps; ++j) {
                        const Fr *g = column.data() + units[u].row + sh.gaps[j].cell_offset + sh.gaps[j].num_cells;
                        EXPECT(g[-3] == g[1], "comparison unit %zu gap %u: l_i is not the range check's last limb\n", u, j);
                    }
                cmp_units_run += count;
            }
    printf("ec selftest: %zu curve units, %zu comparison units, %d failures\n", units_run, cmp_units_run, fails);
    return fails ? 1 : 0;
}
#endif
