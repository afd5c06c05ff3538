// verify_proof for many proofs under ONE verifying key (upstream's BatchVerifier / AccumulatorStrategy seam [UPSTREAM-RECALL]; only the verdict
// matters, no bytes are shared with upstream).  Each proof's check is e(W'_i, s_g2) == e(outer_i, g2); with random combiners rho_i
//     e(sum rho_i W'_i, s_g2) * e(-sum rho_i outer_i, g2) == 1
// holds for honest proofs and fails for a batch with a bad one except with probability ~ 1/r.  The flow:
//   1. the word indices of a proof's points follow from the shape (verifier_internal.h: proof_words);
//   2. all proofs of the right length are uploaded and ALL their points decompressed in one launch (h2hip_g1_decompress_checked_dev: one
//      verdict per point, so a malformed proof is a rejection, not an error);
//   3. derive (verifier.hip) replays each transcript on the host and returns (commitment, scalar) pairs;
//   4. the scalars are folded: the key's fixed and sigma commitments and g[0] appear ONCE with scalars summed over the proofs, every proof's own
//      points once; identity commitments of the key are skipped;
//   5. one temporary base set, the existing MSM over it for R = sum rho_i outer_i and again for L = sum rho_i W'_i (the MSM kernels are tested
//      on arbitrary, degenerate base sets; a second MSM implementation would only add surface);
//   6. one pairing on the host.
#include <chrono>
#include <vector>

#include "verifier_internal.h"

using namespace h2;
using namespace h2::verifier;

namespace {

struct DevMem {   // a temporary device allocation of this call
    void *p = nullptr;
    ~DevMem() {
        if (p) hipFree(p);
    }
    int alloc(size_t bytes) {
        hipError_t e = hipMalloc(&p, bytes ? bytes : 256);
        if (e != hipSuccess) {
            p = nullptr;
            set_error("h2hip_plonk_verify_batch: hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
            return H2HIP_ERR_NOMEM;
        }
        return H2HIP_OK;
    }
};
// With the context's profile on, the wall time of each stage is added to the profile under "verify_batch_stage:<name>" (one "launch" per
// call), next to the kernels' own entries: tools/verify_batch_times.py reads the split from there.
struct StageClock {
    h2hip_ctx *ctx;
    std::chrono::steady_clock::time_point t0;
    explicit StageClock(h2hip_ctx *c) : ctx(c), t0(std::chrono::steady_clock::now()) {}
    void lap(const char *name) {
        if (!ctx->profiling) return;
        const auto t1 = std::chrono::steady_clock::now();
        h2::KernelStat &st = ctx->stats[std::string("verify_batch_stage:") + name];
        st.total_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
        st.launches += 1;
        t0 = t1;
    }
};
struct TempBases {
    h2hip_ctx *ctx;
    h2hip_bases *b = nullptr;
    explicit TempBases(h2hip_ctx *c) : ctx(c) {}
    ~TempBases() {
        if (b) h2hip_bases_free(ctx, b);
    }
};

int batch_impl(h2hip_ctx *ctx, const plonk::Shape &sh, const VKey &vk, size_t num_proofs, const void *const *instances_host, const size_t *instance_lens,
               const uint8_t *const *proofs, const size_t *proof_lens, const std::vector<Fr> &rho, int *accepted, uint8_t *rejected_out, void *acc_out) {
    const size_t ni = sh.p.num_instance, num_perm_columns = sh.perm_columns.size();
    std::vector<uint32_t> point_words;
    const size_t words = proof_words(sh, &point_words), npts = point_words.size();
    std::vector<uint8_t> bad(num_proofs, 0);
    StageClock clock(ctx);
    // ---- upload every proof of the right length; decompress all their points at once
    std::vector<size_t> live;   // proofs that reach the decompressor
    for (size_t i = 0; i < num_proofs; ++i) {
        if (proofs[i] && proof_lens[i] == 32 * words)
            live.push_back(i);
        else
            bad[i] = 1;   // truncated, or trailing bytes
    }
    H2_REQUIRE(live.size() * words < ((size_t)1 << 31), "too many proof words for one batch");
    std::vector<G1Affine> pts(live.size() * npts);
    std::vector<uint32_t> status(live.size() * npts);
    if (!live.empty()) {
        std::vector<uint8_t> table(live.size() * words * 32);
        std::vector<uint32_t> slots(live.size() * npts);
        for (size_t j = 0; j < live.size(); ++j) {
            memcpy(table.data() + j * words * 32, proofs[live[j]], words * 32);
            for (size_t t = 0; t < npts; ++t) slots[j * npts + t] = (uint32_t)(j * words + point_words[t]);
        }
        DevMem d_words, d_slots, d_pts, d_status;
        H2_CHK(d_words.alloc(table.size()));
        H2_CHK(d_slots.alloc(sizeof(uint32_t) * slots.size()));
        H2_CHK(d_pts.alloc(sizeof(G1Affine) * pts.size()));
        H2_CHK(d_status.alloc(sizeof(uint32_t) * status.size()));
        H2_HIPCHK(hipMemcpyAsync(d_words.p, table.data(), table.size(), hipMemcpyHostToDevice, ctx->stream));
        H2_HIPCHK(hipMemcpyAsync(d_slots.p, slots.data(), sizeof(uint32_t) * slots.size(), hipMemcpyHostToDevice, ctx->stream));
        H2_CHK(h2hip_g1_decompress_checked_dev(ctx, d_words.p, (const uint32_t *)d_slots.p, slots.size(), d_pts.p, (uint32_t *)d_status.p));
        H2_HIPCHK(hipMemcpyAsync(pts.data(), d_pts.p, sizeof(G1Affine) * pts.size(), hipMemcpyDeviceToHost, ctx->stream));
        H2_HIPCHK(hipMemcpyAsync(status.data(), d_status.p, sizeof(uint32_t) * status.size(), hipMemcpyDeviceToHost, ctx->stream));
        H2_HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    clock.lap("upload_decompress");
    // ---- derive per proof; fold the scalars
    const size_t nvk = (size_t)sh.num_fixed_total + num_perm_columns;
    std::vector<G1Affine> vk_pts(nvk);
    memcpy(vk_pts.data(), vk.fixed_commitments, sizeof(G1Affine) * sh.num_fixed_total);
    if (num_perm_columns) memcpy(vk_pts.data() + sh.num_fixed_total, vk.permutation_commitments, sizeof(G1Affine) * num_perm_columns);
    std::vector<Fr> vk_scalars(nvk, Fr::zero());
    Fr g0_scalar = Fr::zero();
    std::vector<G1Affine> base_pts;   // the proofs' own points, then (below) the key's and g[0]
    std::vector<Fr> right_scalars, left_scalars;
    std::vector<size_t> good;
    for (size_t j = 0; j < live.size(); ++j) {
        const size_t i = live[j];
        const DecodedPoints pre = {pts.data() + j * npts, status.data() + j * npts, npts};
        Derived d;
        int well_formed = 0;
        H2_CHK(derive(sh, vk, ni ? instances_host + i * ni : nullptr, ni ? instance_lens + i * ni : nullptr, proofs[i], proof_lens[i], &pre, &d, &well_formed));
        if (!well_formed) {
            bad[i] = 1;
            continue;
        }
        good.push_back(i);
        g0_scalar = fe_add(g0_scalar, fe_mul(rho[i], d.g0_scalar));
        for (const Term &t : d.terms) {
            const Fr s = fe_mul(rho[i], t.s);
            if (t.vk_slot >= 0) {
                vk_scalars[t.vk_slot] = fe_add(vk_scalars[t.vk_slot], s);
            } else {
                base_pts.push_back(t.p);
                right_scalars.push_back(s);
                left_scalars.push_back(Fr::zero());
            }
        }
        left_scalars.back() = rho[i];   // the last term of every proof is (h2, u): W' = h2
    }
    clock.lap("derive");
    G1Affine left, right;
    left.x = left.y = right.x = right.y = Fq::zero();
    if (!good.empty()) {
        for (size_t c = 0; c < nvk; ++c) {
            if (vk_pts[c].is_identity()) continue;
            base_pts.push_back(vk_pts[c]);
            right_scalars.push_back(vk_scalars[c]);
            left_scalars.push_back(Fr::zero());
        }
        G1Affine g0;
        memcpy(&g0, vk.g1, sizeof(G1Affine));
        if (!g0.is_identity()) {
            base_pts.push_back(g0);
            right_scalars.push_back(g0_scalar);
            left_scalars.push_back(Fr::zero());
        }
        // ---- the MSMs: a temporary plain base set, freed when this call returns
        TempBases tb(ctx);
        H2_CHK(h2hip_bases_upload(ctx, base_pts.data(), base_pts.size(), 0, &tb.b));
        H2_CHK(h2hip_msm_g1(ctx, tb.b, right_scalars.data(), right_scalars.size(), H2HIP_POINT_AFFINE, &right));
        H2_CHK(h2hip_msm_g1(ctx, tb.b, left_scalars.data(), left_scalars.size(), H2HIP_POINT_AFFINE, &left));
    }
    if (acc_out) {
        memcpy(acc_out, &left, sizeof(G1Affine));
        memcpy((uint8_t *)acc_out + sizeof(G1Affine), &right, sizeof(G1Affine));
    }
    clock.lap("msm");
    // ---- one pairing
    int pairing_ok = 1;
    if (!good.empty()) H2_CHK(pairing_verdict(vk, left, right, &pairing_ok));
    clock.lap("pairing");
    if (!pairing_ok && rejected_out) {   // the slow path, on failure only: which of the well-formed proofs is it?
        for (size_t i : good) {
            int ok = 0;
            H2_CHK(verify_one(sh, vk, ni ? instances_host + i * ni : nullptr, ni ? instance_lens + i * ni : nullptr, proofs[i], proof_lens[i], &ok));
            if (!ok) bad[i] = 1;
        }
    }
    bool any_bad = false;
    for (uint8_t b : bad) any_bad |= b != 0;
    if (rejected_out) memcpy(rejected_out, bad.data(), num_proofs);
    *accepted = pairing_ok && !any_bad ? 1 : 0;
    return H2HIP_OK;
}

}  // namespace

extern "C" {

int h2hip_plonk_verify_batch(h2hip_ctx *ctx, int kind, const void *params, const void *fixed_commitments, const void *permutation_commitments,
                             const void *transcript_repr, const void *g1, const void *g2, const void *s_g2, size_t num_proofs,
                             const void *const *instances_host, const size_t *instance_lens, const uint8_t *const *proofs, const size_t *proof_lens,
                             h2hip_rng_fill_fn rng, void *rng_user, int *accepted, uint8_t *rejected_out, void *acc_out) {
    H2_DEVICE_GUARD(ctx);
    H2_REQUIRE(ctx && params && fixed_commitments && transcript_repr && g1 && g2 && s_g2 && rng && accepted && (num_proofs == 0 || (proofs && proof_lens)),
               "NULL argument");
    *accepted = 0;
    // RLC keys are not batched (include/h2hip.h): the single verifier and the transcript entry take them
    H2_REQUIRE(kind == H2HIP_CIRCUIT_BASE || kind == H2HIP_CIRCUIT_DYN || kind == H2HIP_CIRCUIT_PHASED, "unknown circuit kind (H2HIP_CIRCUIT_BASE / _DYN / _PHASED)");
    plonk::Shape sh;
    H2_CHK(plonk::shape_of_kind(kind, params, sh));
    const VKey vk = {fixed_commitments, permutation_commitments, transcript_repr, g1, g2, s_g2};
    if (acc_out) memset(acc_out, 0, 2 * sizeof(G1Affine));
    if (rejected_out && num_proofs) memset(rejected_out, 0, num_proofs);
    if (num_proofs == 0) {   // nothing to check, no device work
        *accepted = 1;
        return H2HIP_OK;
    }
    H2_CHK(check_key(sh, vk, instances_host, instance_lens));
    for (size_t i = 0; i < num_proofs; ++i) H2_REQUIRE(proofs[i] || proof_lens[i] == 0, "NULL argument");
    std::vector<Fr> rho(num_proofs);
    rng(rng_user, rho.data(), num_proofs);   // ONE call
    for (const Fr &r : rho) H2_REQUIRE(canonical(r) && !r.is_zero(), "the rng returned a zero (or non-canonical) combiner: that proof would go unchecked");
    return batch_impl(ctx, sh, vk, num_proofs, instances_host, instance_lens, proofs, proof_lens, rho, accepted, rejected_out, acc_out);
}

}  // extern "C"
