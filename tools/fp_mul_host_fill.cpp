// tools/fp_mul_time.py's host side: h2hip_fp_mul_fill_dev's cells and the cells of the nine range checks computed on ONE host thread with
// the library's host field and the library's own per-unit and per-slot code (csrc/fp_mul.cuh, csrc/range_fill.cuh), into host columns, from
// operands in host memory — what a caller had to do with the cells before the device fill existed, short of writing big integers of its own.
// Built by the tool (hipcc, host only); not part of libh2hip.
//
// With -DFP_MUL_SELFTEST the file is a stand-alone program (its own main; build it with -fsanitize=address,undefined): it runs the same code
// over the tests' operand pools (every pair of 0, 1, p - 1, p, p + 1, 2^(n k) - 1, two improper units) for the tests' parameter sets and
// moduli, and checks what must hold whatever the integers are: O < p; for proper operands check_i - c_i 2^n = -c_{i-1} in Fr (the carries
// divide exactly); where Q has at most k limbs out_native + m_nat quot_native = N; every own cell written, every gap and every cell
// outside the run untouched.
#include <stdlib.h>

#include "../halo2-lib_amd/csrc/fp_mul.cuh"

using namespace h2;

template <int K>
static void solve_all(const FpCall &fc, const h2hip_fp_mul *units, size_t count) {
    for (size_t u = 0; u < count; ++u) fp_solve_unit<K>(fc, units[u], (uint32_t)u);
}

// lk_cols == NULL: the own cells only.  results: count (3 k + 1) elements (needed).  -> 0, or 1 when the parameters are refused
extern "C" int fp_mul_host_fill(void *const *columns_host, size_t num_columns, const uint32_t *break_points, void *const *lookup_columns_host,
                                size_t num_lookup_columns, const h2hip_fp_params *params, const void *values_host, void *results_host,
                                const h2hip_fp_mul *units, const uint64_t *lookup_slots, size_t count) {
    FpShape sh;
    FpCall fc;
    Fr consts[FP_CONSTS];
    if (fp_prepare(*params, sh, &fc, consts)) return 1;
    const uint32_t k = sh.k;
    std::vector<Fr> rec((size_t)fp_record_len(k) * count);
    fc.tc = TraceCols{(Fr *const *)columns_host, break_points, (uint32_t)(num_columns - 1)};
    fc.values = (const Fr *)values_host;
    fc.consts = consts;
    fc.results = (Fr *)results_host;
    fc.rec = rec.data();
    if (k == 2)
        solve_all<2>(fc, units, count);
    else if (k == 3)
        solve_all<3>(fc, units, count);
    else
        solve_all<4>(fc, units, count);
    for (size_t u = 0; u < count; ++u)
        for (uint32_t s = 0; s < fp_unit_slots(k); ++s) fp_place_slot(fc, units[u], (uint32_t)u, s);
    if (!lookup_columns_host) return 0;
    // the nine range checks per unit, gap by gap in context order (the table of powers is the one the library uploads per range call)
    uint64_t lk_before = 0;
    for (uint32_t j = 0; j < 3 * k; ++j) {
        RangeCall rc;
        std::vector<Fr> pows;
        if (range_prepare(sh.gaps[j].range_bits, sh.lb, 0, 0, rc, &pows)) return 1;
        rc.tc = fc.tc;
        rc.lk_cols = (Fr *const *)lookup_columns_host;
        rc.values = (const Fr *)results_host;
        rc.num_lk_cols = (uint32_t)num_lookup_columns;
        for (size_t u = 0; u < count; ++u) {
            const TraceOut at = trace_at(fc.tc, units[u].column, units[u].row, sh.gaps[j].cell_offset);
            const h2hip_range_check chk{at.col, (uint32_t)(at.p - fc.tc.cols[at.col]), u * fp_result_len(k) + sh.gaps[j].result_index, 0, lookup_slots[u] + lk_before};
            for (uint32_t s = 0; s < range_unit_slots(rc.L, rc.rem); ++s) range_slot(rc, chk, s);
        }
        lk_before += sh.gap_lookups[j];
    }
    return 0;
}

#ifdef FP_MUL_SELFTEST
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
static void add_small(uint32_t *w, int d) {   // w += d, d in {-1, 0, 1}, over 12 words
    for (int j = 0; j < 12 && d; ++j) {
        if (d > 0 && ++w[j]) break;
        if (d < 0 && w[j]--) break;
    }
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
    static const uint32_t sets[5][3] = {{88, 3, 8}, {88, 3, 18}, {90, 3, 15}, {91, 3, 13}, {64, 4, 8}};
    const Fr sentinel = pow2_mont(253);   // (no cell of a unit holds 2^253)
    size_t units_run = 0;
    for (const auto &set : sets)
        for (const char *hex : moduli) {
            const uint32_t n = set[0], k = set[1];
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
            FpShape sh;
            FpCall fc;
            Fr consts[FP_CONSTS];
            const char *bad = fp_prepare(pr, sh, &fc, consts);
            EXPECT(!bad, "refused: %s\n", bad ? bad : "");
            if (bad) continue;
            // the pool: 0, 1, p - 1, p, p + 1, 2^(n k) - 1
            uint32_t pool[6][12];
            memset(pool, 0, sizeof pool);
            pool[1][0] = 1;
            for (int e = 2; e < 5; ++e) {
                memcpy(pool[e], pr.modulus, 48);
                add_small(pool[e], e - 3);
            }
            for (uint32_t b = 0; b < n * k; ++b) pool[5][b >> 5] |= 1u << (b & 31);
            std::vector<Fr> values;
            std::vector<h2hip_fp_mul> units;
            const uint32_t cells = sh.lay.total;
            auto add_unit = [&](const Fr *a, const Fr *b) {
                h2hip_fp_mul u;
                u.column = 0;
                u.row = 2 + (uint32_t)units.size() * (cells + 1);
                u.a_offset = values.size();
                values.insert(values.end(), a, a + k + 1);
                u.b_offset = values.size();
                values.insert(values.end(), b, b + k + 1);
                units.push_back(u);
            };
            Fr a[FP_MAX_K + 1], b[FP_MAX_K + 1];
            for (int x = 0; x < 6; ++x)
                for (int y = 0; y < 6; ++y) {
                    from_words(pool[x], n, k, a);
                    from_words(pool[y], n, k, b);
                    add_unit(a, b);
                }
            const size_t proper = units.size();
            from_words(pool[2], n, k, a);
            from_words(pool[5], n, k, b);
            a[1] = pow2_mont(n);   // an improper limb: 2^n
            add_unit(a, b);
            from_words(pool[5], n, k, a);
            a[0] = fe_neg(Fr::one());   // r - 1
            add_unit(a, b);
            const size_t count = units.size(), rows = 2 + count * (cells + 1) + 3;
            std::vector<Fr> column(rows, sentinel), results(count * fp_result_len(k), sentinel);
            void *cols[1] = {column.data()};
            EXPECT(fp_mul_host_fill(cols, 1, nullptr, nullptr, 0, &pr, values.data(), results.data(), units.data(), nullptr, count) == 0, "the fill refused\n");
            // cells: own cells written, gaps and the rest untouched
            std::vector<char> own(cells, 1);
            for (uint32_t j = 0; j < 3 * k; ++j)
                for (uint32_t c = 0; c < sh.gaps[j].num_cells; ++c) own[sh.gaps[j].cell_offset + c] = 0;
            size_t written = 0;
            for (size_t r = 0; r < rows; ++r) written += column[r] != sentinel;
            EXPECT(written == count * sh.own, "%zu cells written, %zu own cells\n", written, count * sh.own);
            for (size_t u = 0; u < count; ++u) {
                const Fr *run = column.data() + units[u].row;
                for (uint32_t c = 0; c < cells; ++c) EXPECT((run[c] != sentinel) == (own[c] != 0), "unit %zu cell %u: own / gap mismatch\n", u, c);
                const Fr *res = results.data() + u * fp_result_len(k);
                // O < p from its limbs' cells: recompose into words
                uint32_t O[12] = {0};
                for (uint32_t i = k; i-- > 0;) {
                    const uint32_t ws = n >> 5, s = n & 31;
                    for (int j = 11; j >= 0; --j) {
                        const uint32_t hi = j >= (int)ws ? O[j - ws] : 0, lo = j >= (int)ws + 1 ? O[j - ws - 1] : 0;
                        O[j] = s ? (hi << s) | (lo >> (32 - s)) : hi;
                    }
                    const Fr c = fe_from_mont(res[i]);
                    for (int j = 0; j < 4; ++j) O[j] |= c.l[j];
                }
                unsigned br = 0;
                uint32_t pw[12];
                memcpy(pw, pr.modulus, 48);
                for (int j = 0; j < 12; ++j) subb32(O[j], pw[j], br);
                EXPECT(br == 1, "unit %zu: O >= p\n", u);
                if (u >= proper) continue;
                // the carries divide exactly: check_i + (-c_i) 2^n = -c_{i-1}, the gate of S6_i
                Fr prev = Fr::zero();
                for (uint32_t i = 0; i < k; ++i) {
                    const Fr *s6 = run + sh.lay.base6 + i * (8 + sh.gap[4]);
                    EXPECT(fe_add(s6[0], fe_mul(s6[1], s6[2])) == s6[3] && s6[3] == prev, "unit %zu: carry %u does not divide exactly\n", u, i);
                    prev = s6[1];
                }
                // the native identity where Q has at most k limbs (both operands at most p + 1 here)
                const size_t x = u / 6, y = u % 6;
                if (x < 5 && y < 5) {
                    const Fr *s9 = run + sh.lay.off9;
                    EXPECT(fe_add(run[sh.lay.off9 - 1], fe_mul(s9[0], s9[1])) == s9[2], "unit %zu: out_native + m_nat quot_native != N\n", u);
                }
            }
            // once more with the range checks (range_prepare's RangeCall per gap): every cell of every run and every lookup cell written
            std::vector<Fr> lk(count * sh.num_lookups + 1, sentinel);
            std::vector<uint64_t> lk_slots(count);
            for (size_t u = 0; u < count; ++u) lk_slots[u] = u * sh.num_lookups;
            void *lks[1] = {lk.data()};
            EXPECT(fp_mul_host_fill(cols, 1, nullptr, lks, 1, &pr, values.data(), results.data(), units.data(), lk_slots.data(), count) == 0, "the fill with range checks refused\n");
            size_t filled = 0, looked = 0;
            for (size_t r = 0; r < rows; ++r) filled += column[r] != sentinel;
            for (const Fr &c : lk) looked += c != sentinel;
            EXPECT(filled == count * cells && looked + 1 == lk.size() && lk.back() == sentinel, "%zu cells and %zu lookup cells written with the range checks\n", filled, looked);
            units_run += count;
        }
    printf("fp_mul selftest: %zu units, %d failures\n", units_run, fails);
    return fails ? 1 : 0;
}
#endif
