// The constraint system of every circuit configuration, derived ONCE from its parameters: column numbering, queries in first-query order,
// permutation columns, lookups, phases and RLC columns.  The prover (plonk_internal.h), the verifier (verifier_internal.h) and the witness
// check read the same Shape; the initialisers below are the only place that orders a query or a permutation column.  Host code only.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "internal.h"

namespace h2 {
namespace plonk {

static const uint64_t ROOT_OF_UNITY[4] = {0xd34f1ed960c37c9cULL, 0x3215cf6dd39329c8ULL, 0x98865ea93dd31f74ULL, 0x03ddb9f5166d18b7ULL};   // 7^((r-1)/2^28)
static const uint64_t ZETA[4] = {0xb8ca0b2d36636f23ULL, 0xcc37a73fec2bc5e9ULL, 0x048b6e193fd84104ULL, 0x30644e72e131a029ULL};            // 7^(2(r-1)/3)
static const uint64_t DELTA[4] = {0x870e56bbe533e9a2ULL, 0x5b5f898e5e963f25ULL, 0x64ec26aad4c86e71ULL, 0x09226b6e22c6f0caULL};           // 7^(2^28)

struct ColumnRef {
    int kind;   // 0 = fixed, 1 = advice, 2 = instance
    int index;
};
using ColumnProduct = std::vector<ColumnRef>;   // an expression of a lookup: a product of columns at Rotation::cur()
struct Lookup {
    int q_col;   // fixed column of the complex selector, or -1
    int advice_col, table_col;
    std::vector<ColumnRef> in, tab;   // dynamic lookups (q_col = advice_col = table_col = -1): the expressions compressed by theta
};
struct Shape {
    h2hip_base_circuit_params p;
    uint32_t k, n;
    bool with_range, single;
    bool dyn = false;              // BasicDynLookupConfig + FlexGateConfig (init_dyn); otherwise BaseConfig (init)
    uint32_t key_cols = 0;         // dyn: KEY_COL; lookup expressions have key_cols + 1 columns
    uint32_t first_gate_advice = 0;   // advice index of gate column 0 (dyn: behind the table and key columns)
    bool from_phased = false;      // made by init_phased (h2hip_plonk_keygen_phased)
    bool phased = false;           // multi-phase BaseConfig (init_phased) with more than one used phase or a challenge
    std::vector<std::vector<int>> phase_cols;   // phased: the advice columns of every used phase, index order (gate, then lookup advice)
    uint32_t phase_challenges[H2HIP_MAX_PHASE] = {0, 0, 0};   // phased: challenges squeezed after each phase's commitments
    uint32_t num_rlc = 0;          // RLC columns (init_rlc): phase-1 advice columns behind every BaseConfig column, gate q_rlc * (a0 * gamma + a1 - a2)
    uint32_t first_rlc_advice = 0; // advice index of RLC column 0
    int first_q_rlc_col = -1;      // fixed column of RLC column 0's selector
    int table_col = -1, q_lookup_col = -1, first_constant_col = -1, first_q_enable_col = -1;
    uint32_t num_advice_total, num_fixed_total;
    std::vector<Lookup> lookups;
    std::vector<ColumnRef> perm_columns;
    std::vector<std::pair<int, int>> advice_queries, fixed_queries;   // (column, rotation) in first-query order
    uint32_t degree, blinding_factors, usable_rows, chunk_len, quotient_pieces, extended_k, num_perm_sets;

    int init(const h2hip_base_circuit_params &bp) {
        p = bp;
        k = bp.k;
        H2_REQUIRE(k >= 4 && k <= 26, "k out of range (4..26)");
        // the reference's configurations go up to 291 gate + 53 lookup advice columns (halo2-ecc/configs/secp256k1/bench_ecdsa.config:9)
        H2_REQUIRE(bp.num_advice >= 1 && bp.num_advice <= 1024 && bp.num_lookup_advice <= 256 && bp.num_fixed <= 16 && bp.num_instance <= 8,
                   "column counts out of range");
        H2_REQUIRE(bp.lookup_bits < (int32_t)k, "lookup_bits must be less than k");
        const bool range = bp.lookup_bits >= 0 && bp.num_lookup_advice != 0;
        const bool q_lookup = range && bp.num_advice == 1;   // range/mod.rs:93-95: the lookup sits on the gate column behind a complex selector
        return layout(bp, range, q_lookup, (q_lookup || !range) ? 0 : bp.num_lookup_advice);
    }
    // the columns, lookups and queries of FlexGateConfig + RangeConfig: bp.num_advice gate columns, `nla` dedicated lookup-advice columns,
    // the table iff `range`, the complex selector q_lookup on gate column 0 iff `q_lookup`
    int layout(const h2hip_base_circuit_params &bp, bool range, bool q_lookup, uint32_t nla) {
        n = 1u << k;
        with_range = range;
        single = q_lookup;
        int nf = 0;
        if (with_range) table_col = nf++;            // meta.lookup_table_column() is created first (range/mod.rs:82)
        first_constant_col = bp.num_fixed ? nf : -1;
        nf += (int)bp.num_fixed;                     // flex_gate/mod.rs:123-129
        // selectors are compressed into fixed columns after the circuit's own ones: the complex selector keeps a column of its own, and
        // the per-column gate selectors are enabled on common rows, so none of them can share a column either [UPSTREAM compress_selectors]
        if (single) q_lookup_col = nf++;
        first_q_enable_col = nf;
        nf += (int)bp.num_advice;
        if (num_rlc) first_q_rlc_col = nf;   // the RLC selectors are created after BaseConfig's
        nf += (int)num_rlc;
        num_fixed_total = (uint32_t)nf;
        first_rlc_advice = bp.num_advice + nla;
        num_advice_total = bp.num_advice + nla + num_rlc;
        if (single) lookups.push_back({q_lookup_col, 0, table_col});
        for (uint32_t i = 0; i < nla; ++i) lookups.push_back({-1, (int)(bp.num_advice + i), table_col});
        // enable_equality order: constants, gate advice, lookup advice, instance
        for (uint32_t i = 0; i < bp.num_fixed; ++i) perm_columns.push_back({0, first_constant_col + (int)i});
        for (uint32_t i = 0; i < first_rlc_advice; ++i) perm_columns.push_back({1, (int)i});
        for (uint32_t i = 0; i < bp.num_instance; ++i) perm_columns.push_back({2, (int)i});
        for (uint32_t i = 0; i < num_rlc; ++i) perm_columns.push_back({1, (int)(first_rlc_advice + i)});   // enable_equality is called on them last
        for (uint32_t a = 0; a < bp.num_advice; ++a)
            for (int r = 0; r < 4; ++r) advice_queries.push_back({(int)a, r});
        for (uint32_t i = 0; i < nla; ++i) advice_queries.push_back({(int)(bp.num_advice + i), 0});
        for (uint32_t i = 0; i < num_rlc; ++i)
            for (int r = 0; r < 3; ++r) advice_queries.push_back({(int)(first_rlc_advice + i), r});
        for (uint32_t i = 0; i < bp.num_fixed; ++i) fixed_queries.push_back({first_constant_col + (int)i, 0});
        if (with_range) fixed_queries.push_back({table_col, 0});
        if (single) fixed_queries.push_back({q_lookup_col, 0});
        for (uint32_t i = 0; i < bp.num_advice; ++i) fixed_queries.push_back({first_q_enable_col + (int)i, 0});
        for (uint32_t i = 0; i < num_rlc; ++i) fixed_queries.push_back({first_q_rlc_col + (int)i, 0});
        H2_CHK(finish(__func__));
        H2_REQUIRE(extended_k <= 28, "extended domain exceeds the 2-adicity of F_r");
        // range/mod.rs:117-121: the table must fit gate.max_rows = 2^k - meta.minimum_rows() = n - (blinding_factors + 3)
        if (bp.lookup_bits >= 0 && with_range) H2_REQUIRE(((uint64_t)1 << bp.lookup_bits) <= n - (blinding_factors + 3), "lookup table is too large for the circuit degree plus blinding factors");
        return H2HIP_OK;
    }
    // BasicDynLookupConfig::new(meta, || FirstPhase, lu_sets) then FlexGateConfig::configure (memory.rs:92-98); include/h2hip.h states the layout
    int init_dyn(const h2hip_dyn_circuit_params &dp) {
        H2_REQUIRE(dp.k >= 4 && dp.k <= 26, "k out of range (4..26)");
        H2_REQUIRE(dp.key_cols >= 1 && dp.key_cols <= 4, "key_cols out of range (1..4)");
        H2_REQUIRE(dp.lu_sets >= 1 && dp.lu_sets <= 48, "lu_sets out of range (1..48)");
        H2_REQUIRE(dp.num_advice >= 1 && dp.num_advice <= 1024 && dp.num_fixed <= 16, "column counts out of range");
        p = h2hip_base_circuit_params{dp.k, dp.num_advice, 0, dp.num_fixed, 0, -1};
        k = dp.k;
        n = 1u << k;
        dyn = true;
        with_range = single = false;
        key_cols = dp.key_cols;
        const uint32_t m = dp.key_cols, L = dp.lu_sets, ndyn = m * (1 + L);
        first_gate_advice = ndyn;
        num_advice_total = ndyn + dp.num_advice;
        first_constant_col = dp.num_fixed ? (int)(1 + L) : -1;
        first_q_enable_col = (int)(1 + L + dp.num_fixed);
        num_fixed_total = 1 + L + dp.num_fixed + dp.num_advice;
        for (uint32_t s = 0; s < L; ++s) {
            Lookup l{-1, -1, -1, {}, {}};
            for (uint32_t j = 0; j < m; ++j) {
                l.in.push_back({1, (int)(m * (1 + s) + j)});
                l.tab.push_back({1, (int)j});
            }
            l.in.push_back({0, (int)(1 + s)});   // key_is_enabled of the set
            l.tab.push_back({0, 0});             // table_is_enabled
            lookups.push_back(l);
        }
        for (uint32_t c = 0; c < ndyn; ++c) perm_columns.push_back({1, (int)c});
        for (uint32_t i = 0; i < dp.num_fixed; ++i) perm_columns.push_back({0, first_constant_col + (int)i});
        for (uint32_t a = 0; a < dp.num_advice; ++a) perm_columns.push_back({1, (int)(ndyn + a)});
        for (uint32_t c = 0; c < ndyn; ++c) advice_queries.push_back({(int)c, 0});
        for (uint32_t a = 0; a < dp.num_advice; ++a)
            for (int r = 0; r < 4; ++r) advice_queries.push_back({(int)(ndyn + a), r});
        for (uint32_t c = 0; c < num_fixed_total; ++c) fixed_queries.push_back({(int)c, 0});
        // degree 4 (single-column lookup expressions), three quotient pieces: extended_k = k + 2 <= 28 for every k this accepts, so layout's
        // check of the extended domain against the 2-adicity of F_r has nothing to catch here
        return finish(__func__);
    }
    // FlexGateConfig / RangeConfig::configure with num_advice_per_phase / num_lookup_advice_per_phase (flex_gate/mod.rs:121-137,
    // range/mod.rs:87-108); include/h2hip.h states the layout.  One used phase and no challenge is init() of that phase's BaseCircuitParams.
    // rlc != 0 (init_rlc): `rlc` RLC columns join phase 1 behind every column of this layout
    int init_phased(const h2hip_phased_circuit_params &pp, uint32_t rlc = 0) {
        from_phased = true;
        num_rlc = rlc;
        const uint32_t *g = pp.num_advice_per_phase, *la = pp.num_lookup_advice_per_phase;
        uint64_t G = 0, LA = 0, CH = 0;
        for (int ph = 0; ph < H2HIP_MAX_PHASE; ++ph) {
            G += g[ph];
            LA += la[ph];
            CH += pp.num_challenges_per_phase[ph];
        }
        H2_REQUIRE(G >= 1 && G <= 1024 && LA <= 256 && pp.num_fixed <= 16 && pp.num_instance <= 8, "column counts out of range");
        H2_REQUIRE(CH <= H2HIP_MAX_CHALLENGES, "more than 8 challenges");
        const bool range = pp.lookup_bits >= 0 && LA != 0;   // gates/circuit/mod.rs:74-85
        const bool q_lookup = range && g[0] == 1 && la[0] != 0;
        uint32_t ded[H2HIP_MAX_PHASE], cols[H2HIP_MAX_PHASE];
        for (int ph = 0; ph < H2HIP_MAX_PHASE; ++ph) {
            ded[ph] = !range || (ph == 0 && q_lookup) ? 0 : la[ph];   // range/mod.rs:93-95: later phases always get dedicated columns
            cols[ph] = g[ph] + ded[ph] + (ph == 1 ? rlc : 0);
        }
        uint32_t used = 0;
        for (int ph = 0; ph < H2HIP_MAX_PHASE; ++ph) {
            if (cols[ph]) {
                H2_REQUIRE(ph == 0 || cols[ph - 1], "a phase has advice columns but the phase before it has none (phases must be contiguous)");
                used = (uint32_t)ph + 1;
            }
            H2_REQUIRE(!pp.num_challenges_per_phase[ph] || cols[ph], "a challenge follows a phase that has no advice column");
        }
        if (used == 1 && CH == 0 && !rlc) {
            H2_CHK(init(h2hip_base_circuit_params{pp.k, g[0], la[0], pp.num_fixed, pp.num_instance, pp.lookup_bits}));
            phase_cols.push_back({});
            for (uint32_t c = 0; c < num_advice_total; ++c) phase_cols[0].push_back((int)c);
            return H2HIP_OK;
        }
        const uint32_t nd = ded[0] + ded[1] + ded[2];
        const h2hip_base_circuit_params bp{pp.k, (uint32_t)G, nd, pp.num_fixed, pp.num_instance, pp.lookup_bits};
        p = bp;
        k = pp.k;
        H2_REQUIRE(k >= 4 && k <= 26, "k out of range (4..26)");
        H2_REQUIRE(pp.lookup_bits < (int32_t)k, "lookup_bits must be less than k");
        H2_CHK(layout(bp, range, q_lookup, nd));
        phased = true;
        uint32_t go = 0, lo = (uint32_t)G;
        for (uint32_t ph = 0; ph < used; ++ph) {
            std::vector<int> c;
            for (uint32_t i = 0; i < g[ph]; ++i) c.push_back((int)(go + i));
            for (uint32_t i = 0; i < ded[ph]; ++i) c.push_back((int)(lo + i));
            if (ph == 1)
                for (uint32_t i = 0; i < rlc; ++i) c.push_back((int)(first_rlc_advice + i));
            go += g[ph];
            lo += ded[ph];
            phase_cols.push_back(c);
            phase_challenges[ph] = pp.num_challenges_per_phase[ph];
        }
        return H2HIP_OK;
    }
    // BaseConfig::configure(base) followed by num_rlc_advice RLC columns (downstream's RlcConfig); include/h2hip.h states the layout
    int init_rlc(const h2hip_rlc_circuit_params &rp) {
        H2_REQUIRE(rp.num_rlc_advice >= 1 && rp.num_rlc_advice <= 64, "num_rlc_advice out of range (1..64; a circuit without RLC columns uses h2hip_phased_circuit_params)");
        H2_REQUIRE(rp.base.num_challenges_per_phase[0] >= 1, "the RLC gate needs a challenge usable after phase 0 (num_challenges_per_phase[0] >= 1)");
        H2_CHK(init_phased(rp.base, rp.num_rlc_advice));
        // the gate has degree 2 + selector and three rotations: degree, extended_k and the blinding factors stay the base layout's
        H2_REQUIRE(blinding_factors == 6, "internal: the RLC columns changed the blinding factors");
        Shape base;
        if (base.init_phased(rp.base) == H2HIP_OK)   // (a base that is only legal with phase 1's RLC columns has nothing to compare with)
            H2_REQUIRE(degree == base.degree && extended_k == base.extended_k && blinding_factors == base.blinding_factors && usable_rows == base.usable_rows,
                       "internal: the RLC gate changed the degree, the extended domain or the blinding factors of the base layout");
        else
            set_error("");
        return H2HIP_OK;
    }
    uint32_t num_commitments() const {
        return num_advice_total + 3 * (uint32_t)lookups.size() + num_perm_sets + 1 + quotient_pieces + 2;
    }
    uint32_t num_evals() const {
        return (uint32_t)advice_queries.size() + (uint32_t)fixed_queries.size() + 1 + (uint32_t)perm_columns.size() +
               (num_perm_sets ? 3 * num_perm_sets - 1 : 0) + 5 * (uint32_t)lookups.size();
    }

    // ---- what the verifier and the witness check read beyond the lists above; the gates fold into h(X) in this order, `gates` first
    // (q_enable fixed column, advice column): q * (a + b*c - d) at rotations 0..3
    std::vector<std::pair<int, int>> gates() const {
        std::vector<std::pair<int, int>> g;
        for (uint32_t a = 0; a < p.num_advice; ++a) g.push_back({first_q_enable_col + (int)a, (int)(first_gate_advice + a)});
        return g;
    }
    // (q_rlc fixed column, advice column): q * (a * challenge 0 + a(wX) - a(w^2 X))
    std::vector<std::pair<int, int>> rlc_gates() const {
        std::vector<std::pair<int, int>> g;
        for (uint32_t j = 0; j < num_rlc; ++j) g.push_back({first_q_rlc_col + (int)j, (int)(first_rlc_advice + j)});
        return g;
    }
    // lookup li as (input, table) lists of expressions, compressed by Horner in theta (upstream's compress_expressions).  BaseConfig's
    // lookups have one expression each, so theta drops out there; a dynamic lookup has one single-column expression per tuple entry
    void lookup_exprs(size_t li, std::vector<ColumnProduct> &in, std::vector<ColumnProduct> &tab) const {
        const Lookup &l = lookups[li];
        in.clear();
        tab.clear();
        if (dyn) {
            for (const ColumnRef &c : l.in) in.push_back(ColumnProduct{c});
            for (const ColumnRef &c : l.tab) tab.push_back(ColumnProduct{c});
        } else {
            in.push_back(l.q_col >= 0 ? ColumnProduct{{0, l.q_col}, {1, l.advice_col}} : ColumnProduct{{1, l.advice_col}});
            tab.push_back(ColumnProduct{{0, l.table_col}});
        }
    }

private:
    // what every layout ends with, once its lookups and permutation columns are known.  `who`: the initialiser the error text names
    int finish(const char *who) {
        degree = 3;   // gate and permutation argument; the RLC gate is selector * degree 2 as well
        for (const Lookup &l : lookups) degree = std::max<uint32_t>(degree, std::max<uint32_t>(4, 2 + (l.q_col >= 0 ? 2 : 1) + 1));
        blinding_factors = std::max<uint32_t>(3, 4) + 2;   // a gate column is queried at four rotations (an RLC column at three)
        H2_REQUIRE_AS(who, n > blinding_factors + 8, "k too small for the blinding rows");
        usable_rows = n - (blinding_factors + 1);
        chunk_len = degree - 2;
        quotient_pieces = degree - 1;
        extended_k = k;
        while (((uint64_t)1 << extended_k) < (uint64_t)n * quotient_pieces) ++extended_k;
        num_perm_sets = (uint32_t)((perm_columns.size() + chunk_len - 1) / chunk_len);
        return H2HIP_OK;
    }
};

// the Shape of a configuration named by its H2HIP_CIRCUIT_* kind; params: that kind's parameter struct
inline int shape_of_kind(int kind, const void *params, Shape &out) {
    H2_REQUIRE(kind == H2HIP_CIRCUIT_BASE || kind == H2HIP_CIRCUIT_DYN || kind == H2HIP_CIRCUIT_PHASED || kind == H2HIP_CIRCUIT_RLC,
               "unknown circuit kind (H2HIP_CIRCUIT_BASE / _DYN / _PHASED / _RLC)");
    if (kind == H2HIP_CIRCUIT_BASE) return out.init(*(const h2hip_base_circuit_params *)params);
    if (kind == H2HIP_CIRCUIT_DYN) return out.init_dyn(*(const h2hip_dyn_circuit_params *)params);
    if (kind == H2HIP_CIRCUIT_PHASED) return out.init_phased(*(const h2hip_phased_circuit_params *)params);
    return out.init_rlc(*(const h2hip_rlc_circuit_params *)params);
}

}  // namespace plonk
}  // namespace h2
