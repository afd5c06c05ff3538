// tools/ec_select_time.py's host side (side (b) of DESIGN 3q's measurement): h2hip_ec_select_fill_dev's and h2hip_num_to_bits_fill_dev's cells
// computed on ONE host thread with the library's host field and the library's own per-unit, per-segment and per-bit code
// (csrc/ec_select.cuh), into host columns, from tables, bits and scalars in host memory — what a caller had to do with the cells before the
// device fills existed.  Built by the tool (hipcc, host only); not part of libh2hip.
//
// With -DEC_SELECT_SELFTEST the file is a stand-alone program (its own main; build it with -fsanitize=address,undefined): it runs the same code
// of all three units over a few thousand units — tables, points, selectors and bits from {0, 1, 2, r - 1, 2^n} and a multiplicative sequence,
// both ops, every window 1 .. 8 at k = 3 and 4, break points inside the runs; every width of num_to_bits from values 0, 1, r - 1, 2^nb - 1 —
// and checks what must hold whatever the values are: every gate of every run (a + b c = d at the gate offsets), the copies inside a select
// and an assert_bit, the results being the layout's result cells, every cell of a run written and every cell outside it untouched.
#include <stdlib.h>

#include "../halo2-lib_amd/csrc/ec_select.cuh"

using namespace h2;

// results (or NULL): count 2 (k + 1) elements.  -> 0, or 1 when the call is refused
extern "C" int ec_select_host_fill(void *const *columns_host, size_t num_columns, const uint32_t *break_points, const h2hip_fp_params *params, uint32_t op,
                                   uint32_t window_bits, const void *values_host, void *results_host, const h2hip_ec_select *units, size_t count) {
    SelShape sh;
    SelCall sc;
    Fr consts[FP_CONSTS];
    if (sel_prepare(*params, op, window_bits, sh, &sc, consts)) return 1;
    std::vector<Fr> rec((size_t)sel_record_len(sc) * count);
    sc.tc = TraceCols{(Fr *const *)columns_host, break_points, (uint32_t)(num_columns - 1)};
    sc.values = (const Fr *)values_host;
    sc.consts = consts;
    sc.results = (Fr *)results_host;
    sc.rec = rec.data();
    const uint32_t slots = sel_unit_slots(sc);
    for (size_t u = 0; u < count; ++u) sel_solve_unit(sc, units[u], (uint32_t)u);
    for (size_t u = 0; u < count; ++u)
        for (uint32_t s = 0; s < slots; ++s) sel_place_slot(sc, units[u], (uint32_t)u, s);
    return 0;
}

// results (or NULL): count num_bits elements.  -> 0, or 1 when num_bits is refused
extern "C" int num_to_bits_host_fill(void *const *columns_host, size_t num_columns, const uint32_t *break_points, const void *values_host, void *results_host,
                                     uint32_t num_bits, const h2hip_bits_unit *units, size_t count) {
    if (num_bits < 1 || num_bits > BITS_MAX) return 1;
    const BitsCall bc{TraceCols{(Fr *const *)columns_host, break_points, (uint32_t)(num_columns - 1)}, (const Fr *)values_host, (Fr *)results_host, num_bits};
    for (size_t u = 0; u < count; ++u)
        for (uint32_t i = 0; i < num_bits; ++i) bits_slot(bc, units[u], (uint32_t)u, i);
    return 0;
}

#ifdef EC_SELECT_SELFTEST
static int fails = 0;
#define EXPECT(cond, ...)                \
    do {                                 \
        if (!(cond)) {                   \
            ++fails;                     \
            fprintf(stderr, __VA_ARGS__); \
        }                                \
    } while (0)

static bool gate(const Fr *c) { return fe_add(c[0], fe_mul(c[1], c[2])) == c[3]; }

// a run of `cells` cells laid from (0, row) over two columns with a break at `bp` in column 0, read back in run order (the copy at row 0 of
// column 1 must equal the break cell)
static std::vector<Fr> read_run(const std::vector<Fr> &c0, const std::vector<Fr> &c1, uint32_t row, uint32_t bp, uint32_t cells) {
    std::vector<Fr> run;
    for (uint32_t i = 0; i < cells; ++i) {
        if (row + i <= bp)
            run.push_back(c0[row + i]);
        else
            run.push_back(c1[row + i - bp]);   // the cell behind the break lies at row 1
    }
    if (row <= bp && bp < row + cells) EXPECT(c1[0] == c0[bp], "the break copy differs from the break cell\n");
    return run;
}

int main() {
    static const char *moduli[2] = {"fffffffffffffffffffffffffffffffffffffffffffffffffffffffefffffc2f", "30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47"};
    static const uint32_t sets[2][3] = {{88, 3, 8}, {64, 4, 8}};
    const Fr sentinel = fe_add(pow2_mont(253), pow2_mont(7));   // (no cell below holds 2^253 + 2^7)
    size_t sel_units = 0, bits_units = 0;
    for (const auto &set : sets)
        for (const char *hex : moduli)
            for (uint32_t w = 0; w <= SEL_MAX_WINDOW; ++w) {
                const uint32_t n = set[0], k = set[1], pt = 2 * (k + 1), op = w ? H2HIP_EC_SELECT_FROM_BITS : H2HIP_EC_SELECT, m = 1u << w;
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
                SelShape sh;
                const char *bad = sel_prepare(pr, op, w, sh, nullptr, nullptr);
                EXPECT(!bad, "refused: %s\n", bad ? bad : "");
                if (bad) continue;
                const uint32_t cells = sh.total, count = w >= 6 ? 12 : 96;
                // the values: specials, then a multiplicative sequence
                const Fr specials[5] = {Fr::zero(), Fr::one(), fe_add(Fr::one(), Fr::one()), fe_neg(Fr::one()), pow2_mont(n)};
                std::vector<Fr> values;
                Fr x = pow2_mont(77);
                const Fr step = fe_add(pow2_mont(131), specials[2]);
                std::vector<h2hip_ec_select> units;
                for (uint32_t u = 0; u < count; ++u) {
                    h2hip_ec_select un;
                    un.column = 0;
                    un.row = 1 + u * (cells + 1);
                    un.p_offset = values.size();
                    for (uint32_t i = 0; i < (w ? m * pt : pt); ++i) {
                        x = fe_mul(x, step);
                        values.push_back((i + u) % 7 == 3 ? specials[(i + u) % 5] : x);
                    }
                    un.q_offset = values.size();
                    if (!w)
                        for (uint32_t i = 0; i < pt; ++i) {
                            x = fe_mul(x, step);
                            const Fr same = values[un.p_offset + i];   // (Q's cell equal to P's: a - b = 0)
                            values.push_back(i % 5 == 1 ? same : x);
                        }
                    un.sel_offset = values.size();
                    for (uint32_t i = 0; i < (w ? w : 1); ++i) values.push_back(u % 3 == 2 ? specials[(u + i) % 5] : specials[(u >> i) & 1]);
                    units.push_back(un);
                }
                // two columns, the break inside the run of unit count / 2
                const uint32_t bp = units[count / 2].row + cells / 3, rows = 1 + count * (cells + 1) + 4;
                std::vector<Fr> c0(rows, sentinel), c1(rows, sentinel), results((size_t)count * pt, sentinel);
                void *cols[2] = {c0.data(), c1.data()};
                const uint32_t bps[1] = {bp};
                EXPECT(ec_select_host_fill(cols, 2, bps, &pr, op, w, values.data(), results.data(), units.data(), count) == 0, "the fill refused\n");
                size_t written = 0;
                for (uint32_t r = 0; r < rows; ++r) written += (c0[r] != sentinel) + (c1[r] != sentinel);
                EXPECT(written == (size_t)count * cells + 1, "(k, w) = (%u, %u): %zu cells written, %zu expected\n", k, w, written, (size_t)count * cells + 1);
                for (uint32_t u = 0; u < count; ++u) {
                    // the unit on the break goes on in column 1; every other lies in column 0 at its rows (a row behind the break point has no break ahead)
                    const bool on = units[u].row <= bp && units[u].row + cells > bp;
                    const std::vector<Fr> run = read_run(c0, c1, units[u].row, on ? bp : rows, cells);
                    for (uint32_t c = 0; c < cells; ++c) EXPECT(run[c] != sentinel, "unit %u cell %u not written\n", u, c);
                    for (uint32_t j = 0; j < pt; ++j) EXPECT(run[sh.out_offsets[j]] == results[(size_t)u * pt + j], "unit %u: result %u is not its cell\n", u, j);
                    if (!w) {
                        for (uint32_t j = 0; j < pt; ++j) {
                            const Fr *c = run.data() + 8 * j;
                            EXPECT(gate(c) && gate(c + 4) && c[0] == c[6] && c[2] == c[4] && c[1] == Fr::one(), "unit %u select %u\n", u, j);
                        }
                        continue;
                    }
                    EXPECT(gate(run.data()), "unit %u: the indicator's first gate\n", u);
                    for (uint32_t t = 0; t + 2 < m; ++t) EXPECT(gate(run.data() + 4 + 8 * t) && gate(run.data() + 8 + 8 * t), "unit %u: indicator node %u\n", u, t);
                    const uint32_t ind = sel_indicator_cells(w), chains = m > k ? k : k + 1;
                    for (uint32_t c = 0; c < 2; ++c) {
                        const Fr *base = run.data() + ind + c * sel_coord_cells(k, m);
                        for (uint32_t j = 0; j < chains; ++j) {
                            EXPECT(base[j * sel_chain_cells(m)] == Fr::zero(), "unit %u: a chain does not start at 0\n", u);
                            for (uint32_t i = 0; i < m; ++i) EXPECT(gate(base + j * sel_chain_cells(m) + 3 * i), "unit %u: chain %u gate %u\n", u, j, i);
                        }
                        if (m > k)
                            for (uint32_t j = 0; j + 1 < k; ++j) EXPECT(gate(base + k * sel_chain_cells(m) + 3 * j), "unit %u: evaluate_native gate %u\n", u, j);
                    }
                }
                sel_units += count;
            }
    // ---- num_to_bits: every width, four values each, a break inside the second unit
    for (uint32_t nb = 1; nb <= BITS_MAX; ++nb) {
        const uint32_t cells = bits_unit_cells(nb), count = 4;
        Fr top = Fr::zero();   // 2^nb - 1 (r - 1 at nb = 254)
        for (uint32_t i = 0; i < nb && i < 254; ++i) top = fe_add(top, pow2_mont(i));
        const Fr values[4] = {Fr::zero(), Fr::one(), fe_neg(Fr::one()), nb == 254 ? fe_neg(Fr::one()) : top};
        h2hip_bits_unit units[4];
        for (uint32_t u = 0; u < count; ++u) units[u] = h2hip_bits_unit{0, 2 + u * (cells + 1), u};
        const uint32_t bp = units[1].row + cells / 2, rows = 2 + count * (cells + 1) + 3;
        std::vector<Fr> c0(rows, sentinel), c1(rows, sentinel), results((size_t)count * nb, sentinel);
        void *cols[2] = {c0.data(), c1.data()};
        const uint32_t bps[1] = {bp};
        EXPECT(num_to_bits_host_fill(cols, 2, bps, values, results.data(), nb, units, count) == 0, "num_to_bits refused\n");
        size_t written = 0;
        for (uint32_t r = 0; r < rows; ++r) written += (c0[r] != sentinel) + (c1[r] != sentinel);
        EXPECT(written == (size_t)count * cells + 1, "num_bits %u: %zu cells written\n", nb, written);
        for (uint32_t u = 0; u < count; ++u) {
            const std::vector<Fr> run = read_run(c0, c1, units[u].row, u == 1 ? bp : rows, cells);
            for (uint32_t i = 0; i + 1 < nb; ++i) EXPECT(gate(run.data() + 3 * i), "num_bits %u unit %u: sum gate %u\n", nb, u, i);
            for (uint32_t i = 0; i < nb; ++i) {
                const Fr *c = run.data() + 3 * nb - 2 + 4 * i, bit = run[i ? 1 + 3 * (i - 1) : 0];
                EXPECT(gate(c) && c[1] == bit && c[2] == bit && c[3] == bit && results[(size_t)u * nb + i] == bit, "num_bits %u unit %u: bit %u\n", nb, u, i);
            }
            const Fr sum = run[3 * nb - 3];
            EXPECT((sum == values[u]) == (u != 2 || nb == 254), "num_bits %u unit %u: the sum and the value\n", nb, u);   // (r - 1 fits 254 bits only)
        }
        bits_units += count;
    }
    printf("ec_select selftest: %zu selection units, %zu num_to_bits units, %d failures\n", sel_units, bits_units, fails);
    return fails ? 1 : 0;
}
#endif
