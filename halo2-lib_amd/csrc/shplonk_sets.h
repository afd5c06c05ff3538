// SHPLONK's grouping of the opening queries into rotation sets: the one copy that ProverSHPLONK (plonk_prove.hip) and VerifierSHPLONK
// (verifier.hip: derive) both run, so the two sides cannot order a set, a point or a commitment differently.  Host code only.
#pragma once
#include <algorithm>
#include <vector>

#include "host_field.h"

namespace h2 {
namespace plonk {

struct Query {
    int poly;   // index into the caller's list: the prover's polynomials, the verifier's commitments
    Fr point, eval;
};
struct RotationSet {
    std::vector<Fr> points;                          // ascending
    std::vector<int> polys;                          // in order of first appearance
    std::vector<std::vector<Fr>> evals;              // [poly][point]
};
// poly/kzg/multiopen/shplonk.rs::construct_intermediate_sets [UPSTREAM-RECALL]
inline void construct_intermediate_sets(const std::vector<Query> &queries, std::vector<RotationSet> &sets, std::vector<Fr> &super_points) {
    // A proof asks ~1000 queries at a handful of points (x and its rotations): every point gets a small index first, every polynomial a bit
    // mask of the points it is opened at — sets are then found by comparing masks, without a container per polynomial.
    std::vector<Fr> distinct;                  // in order of first appearance
    std::vector<uint32_t> point_of(queries.size());
    int max_poly = -1;
    for (size_t qi = 0; qi < queries.size(); ++qi) {
        uint32_t pi = 0;
        while (pi < distinct.size() && fr_cmp(distinct[pi], queries[qi].point) != 0) ++pi;
        if (pi == distinct.size()) distinct.push_back(queries[qi].point);
        point_of[qi] = pi;
        if (queries[qi].poly > max_poly) max_poly = queries[qi].poly;
    }
    const size_t np = distinct.size();
    std::vector<uint32_t> by_value(np);        // point indices in ascending order of the field element
    for (uint32_t i = 0; i < np; ++i) by_value[i] = i;
    std::sort(by_value.begin(), by_value.end(), [&](uint32_t a, uint32_t b) { return fr_cmp(distinct[a], distinct[b]) < 0; });
    super_points.clear();
    for (uint32_t i : by_value) super_points.push_back(distinct[i]);
    if (np > 64) {   // cannot happen for halo2-base's constraint system (rotations -1..3 and the last row); keep the masks honest
        sets.clear();
        return;
    }
    const size_t P = (size_t)max_poly + 1;
    std::vector<uint64_t> mask(P, 0);
    std::vector<int> first_query(P, -1), order;
    std::vector<size_t> eval_at(P * np, (size_t)-1);   // [poly][point] -> first query asking it
    for (size_t qi = 0; qi < queries.size(); ++qi) {
        const int poly = queries[qi].poly;
        if (first_query[poly] < 0) {
            first_query[poly] = (int)qi;
            order.push_back(poly);
        }
        mask[poly] |= 1ull << point_of[qi];
        size_t &slot = eval_at[(size_t)poly * np + point_of[qi]];
        if (slot == (size_t)-1) slot = qi;
    }
    sets.clear();
    std::vector<uint64_t> set_mask;
    for (int poly : order) {
        size_t si = 0;
        while (si < set_mask.size() && set_mask[si] != mask[poly]) ++si;
        if (si == set_mask.size()) {
            set_mask.push_back(mask[poly]);
            sets.push_back(RotationSet());
            for (uint32_t i : by_value)
                if (mask[poly] >> i & 1) sets.back().points.push_back(distinct[i]);
        }
        RotationSet &rs = sets[si];
        rs.polys.push_back(poly);
        rs.evals.emplace_back();
        std::vector<Fr> &ev = rs.evals.back();
        ev.reserve(rs.points.size());
        for (uint32_t i : by_value)
            if (mask[poly] >> i & 1) ev.push_back(queries[eval_at[(size_t)poly * np + i]].eval);
    }
}

}  // namespace plonk
}  // namespace h2
