// plonk::create_proof, one proof: ProofRun (a method per prover round, in upstream's order [UPSTREAM-RECALL, SURVEY.md §3.2 and Appendix A])
// and ProverSHPLONK's O(#openings) bookkeeping.  Host code: all vector work goes through the kernels behind the C ABI (include/h2hip.h).
// The shape, the proving key and the transcript are in plonk_internal.h; keygen and the C entry points in plonk.hip.
#include "plonk_internal.h"
#include "shplonk_sets.h"

namespace h2 {
namespace plonk {

// ---------------------------------------------------------------------------------------------- SHPLONK bookkeeping (the grouping: shplonk_sets.h)
constexpr size_t SHPLONK_MAX_OPENINGS = 64;   // (rotation set, point) pairs of one proof: the slots of the sharded prover's carry exchange
// Lagrange basis of a point set: basis[j] = coefficients (low to high) of L_j(X) = prod_{i != j} (X - x_i) / (x_j - x_i).  Computed once
// per rotation set (its m field inversions are the expensive part on the host), then shared by all polynomials opened on that set.
static std::vector<std::vector<Fr>> lagrange_basis(const std::vector<Fr> &points, std::vector<Fr> &weights) {
    const size_t m = points.size();
    std::vector<std::vector<Fr>> basis(m);
    weights.assign(m, Fr::one());   // weights[j] = 1 / prod_{i != j} (x_j - x_i)
    for (size_t j = 0; j < m; ++j) {
        std::vector<Fr> num(1, Fr::one());
        Fr den = Fr::one();
        for (size_t i = 0; i < m; ++i) {
            if (i == j) continue;
            std::vector<Fr> nxt(num.size() + 1, Fr::zero());
            for (size_t t = 0; t < num.size(); ++t) {
                nxt[t] = fe_sub(nxt[t], fe_mul(num[t], points[i]));
                nxt[t + 1] = fe_add(nxt[t + 1], num[t]);
            }
            num.swap(nxt);
            den = fe_mul(den, fe_sub(points[j], points[i]));
        }
        const Fr scale = m == 1 ? Fr::one() : fe_inv(den);
        weights[j] = scale;
        for (Fr &c : num) c = fe_mul(c, scale);
        basis[j] = num;
    }
    return basis;
}
// coefficients (low to high) of the polynomial of degree < m through (points[j], evals[j])
static std::vector<Fr> lagrange_interpolate(const std::vector<std::vector<Fr>> &basis, const std::vector<Fr> &evals) {
    const size_t m = basis.size();
    std::vector<Fr> out(m, Fr::zero());
    for (size_t j = 0; j < m; ++j)
        for (size_t t = 0; t < m; ++t) out[t] = fe_add(out[t], fe_mul(basis[j][t], evals[j]));
    return out;
}
static Fr eval_small(const std::vector<Fr> &c, const Fr &x) {
    Fr acc = Fr::zero();
    for (size_t i = c.size(); i-- > 0;) acc = fe_add(fe_mul(acc, x), c[i]);
    return acc;
}

// ---------------------------------------------------------------------------------------------- create_proof
static const char *STAGE_NAMES[H2HIP_PLONK_STAGES] = {
    "advice_upload_blinding", "lookup_permute", "commit_advice_lookup_permuted", "grand_products", "ntt_round1_columns_and_commit_products_random",
    "lagrange_to_coeff", "coeff_to_extended", "quotient_terms", "quotient_to_coeff", "commit_h_pieces", "evaluations", "multiopen_shplonk"};
enum { ST_UPLOAD = 0, ST_LOOKUP_PERMUTE, ST_COMMIT_ROUND1, ST_PRODUCTS, ST_COMMIT_PRODUCTS, ST_TO_COEFF, ST_TO_EXT, ST_QUOTIENT, ST_H_COEFF, ST_COMMIT_H,
       ST_EVALS, ST_MULTIOPEN };

struct Laps {
    h2hip_ctx *ctx;
    double *ms;
    std::chrono::steady_clock::time_point t;
    Laps(h2hip_ctx *c, double *m) : ctx(c), ms(m) {
        if (ms) {
            for (int i = 0; i < H2HIP_PLONK_STAGES; ++i) ms[i] = 0;
            t = std::chrono::steady_clock::now();
        }
    }
    void lap(int stage) {
        if (!ms) return;
        hipStreamSynchronize(ctx->stream);
        auto now = std::chrono::steady_clock::now();
        ms[stage] += std::chrono::duration<double, std::milli>(now - t).count();
        t = now;
    }
};

// ---------------------------------------------------------------------------------------------- helpers of one proof
// Blinding rows of MANY columns: drawn back to back they sit `stride` apart in the staging buffer, so one upload and one scatter launch per
// 32 columns replace a small copy per column (a wide shape has hundreds).  reserve() makes room for the whole run first (it may
// synchronise and rewind the buffer); runs longer than the buffer fall back to one copy per column.
struct TailRun {
    std::vector<Fr *> dst;
    const Fr *first = nullptr;
    size_t stride = 0, len = 0;
    bool batched = false;
};
// RNG staging.  The RNG writes straight into the key's pinned host buffer, from where the DMA engine takes it.  Bump allocation: a draw's
// values stay where they are until the buffer wraps, so the (asynchronous) uploads that read them need no synchronisation per draw — wide
// circuits draw hundreds of small tails
struct RngStage {
    h2hip_ctx *ctx;
    h2hip_plonk_pk *pk;
    Scope *sc;
    h2hip_rng_fill_fn rng;
    void *rng_user;
    size_t off = 0;   // the next free element of pk->host_stage
    void make_room(size_t cnt) {
        if (off + cnt > pk->host_stage_elems) {
            hipStreamSynchronize(ctx->stream);
            off = 0;
        }
    }
    const Fr *draw(size_t cnt) {
        make_room(cnt);
        Fr *p = pk->host_stage + off;
        if (cnt) rng(rng_user, p, cnt);   // cnt <= n <= capacity by construction
        off += cnt;
        return p;
    }
    int put(Fr *dst, const Fr *src, size_t cnt) {   // pageable host -> device; the copy returns once `src` is consumed
        if (cnt) H2_HIPCHK(hipMemcpyAsync(dst, src, sizeof(Fr) * cnt, hipMemcpyHostToDevice, ctx->stream));
        return H2HIP_OK;
    }
    void reserve(TailRun &t, size_t columns, size_t stride, size_t len) {
        t.stride = stride;
        t.len = len;
        t.batched = columns >= 4 && columns * stride <= pk->host_stage_elems;
        if (t.batched) make_room(columns * stride);
    }
    int add(TailRun &t, Fr *dst, const Fr *src) {   // src: the draw holding this column's `len` rows
        if (!t.batched) return put(dst, src, t.len);
        if (t.dst.empty()) t.first = src;
        t.dst.push_back(dst);
        return H2HIP_OK;
    }
    int flush(TailRun &t) {
        if (!t.batched || t.dst.empty() || !t.len) return H2HIP_OK;
        const size_t span = (t.dst.size() - 1) * t.stride + t.len;
        Fr *tmp = nullptr;
        H2_CHK(sc->take(span, &tmp));
        H2_HIPCHK(hipMemcpyAsync(tmp, t.first, sizeof(Fr) * span, hipMemcpyHostToDevice, ctx->stream));
        H2_CHK(fr_scatter_rows(ctx, t.dst.data(), t.dst.size(), tmp, t.stride, t.len));
        // (the few KiB stay with this proof's scope: a buffer handed back now could be picked up by the copy stream's upload while the scatter still reads it)
        t.dst.clear();
        return H2HIP_OK;
    }
};

// Shard link: the multi-GPU host exchanges.  Host payloads travel as [8-byte status][payload] per rank; a non-zero status of any rank aborts
// the proof on every rank at the same exchange (H2HIP_ERR_PEER), so nobody is left waiting in the next collective.
struct ShardLink {
    h2hip_ctx *ctx;
    h2hip_plonk_pk *pk;
    std::vector<std::pair<uint64_t, uint64_t>> rank_ranges;   // (offset, len) of every rank's coefficient / point range, by rank (from the hello exchange on)
    bool on() const { return pk->comm != nullptr; }   // (set only for world > 1, or for a forced single-rank run of the sharded path)
    // this rank's point / coefficient range [lo, hi) of a column of `len` elements (one GPU: all of it)
    size_t lo(size_t len) const { return on() ? std::min(pk->shard_offset, len) : 0; }
    size_t hi(size_t len) const { return on() ? std::min(pk->shard_offset + pk->shard_len, len) : len; }
    void schedule(const Shape &sh, bool qshard) {
        pk->exch_sizes.clear();
        pk->exch_next = 0;
        if (!on()) return;   // the proof's host exchanges in order (payload bytes): hello, the five commitment rounds, the quotient's go-ahead
        const size_t P = sizeof(G1Jac);
        pk->exch_sizes = {9 * sizeof(uint64_t), P * (sh.num_advice_total + 2 * sh.lookups.size())};
        if (pk->shard_products) pk->exch_sizes.push_back(sizeof(Fr) * (sh.num_perm_sets + sh.lookups.size()));   // the row ranges' total products
        if (pk->shard_ntt) pk->exch_sizes.push_back(0);   // go-ahead of the column-dealt lagrange_to_coeff of the first-round columns (queued before round 2's commitments) ...
        pk->exch_sizes.push_back(P * (sh.num_perm_sets + sh.lookups.size() + 1));
        if (pk->shard_ntt) pk->exch_sizes.push_back(0);   // ... and of the product columns
        if (qshard) pk->exch_sizes.push_back(0);
        pk->exch_sizes.push_back(P * sh.quotient_pieces);
        pk->exch_sizes.push_back(sizeof(Fr) * (sh.num_evals() + 1));   // the evaluations: partial sums over this rank's coefficient range
        pk->exch_sizes.push_back(sizeof(Fr) * SHPLONK_MAX_OPENINGS);   // SHPLONK by coefficient range: the rotation sets' partial evaluations (carries)
        pk->exch_sizes.push_back(P);
        pk->exch_sizes.push_back(sizeof(Fr));                          // ... and the linearisation's
        pk->exch_sizes.push_back(P);
    }
    int exchange(const void *payload, size_t bytes, std::vector<uint8_t> &all) {
        H2_REQUIRE(pk->exch_next < pk->exch_sizes.size() && pk->exch_sizes[pk->exch_next] == bytes, "internal: exchange out of schedule");
        std::vector<uint8_t> send(8 + bytes, 0);
        if (bytes) memcpy(send.data() + 8, payload, bytes);
        all.assign((8 + bytes) * (size_t)pk->shard_world, 0);
        H2_CHK(h2hip_comm_allgather_host(pk->comm, ctx, send.data(), send.size(), all.data()));
        pk->exch_next++;
        for (uint32_t r = 0; r < pk->shard_world; ++r) {
            uint64_t status;
            memcpy(&status, all.data() + (size_t)r * (8 + bytes), 8);
            if (status) {
                set_error("create_proof: rank %u of the sharded proof reported an error; all ranks abort", r);
                return H2HIP_ERR_PEER;
            }
        }
        return H2HIP_OK;
    }
    int go_ahead() {   // a status-only exchange: what follows it cannot fail on one rank alone
        std::vector<uint8_t> all;
        return exchange(nullptr, 0, all);
    }
    // carry of this rank's range (ending at `hi`) for root p: sum over the ranges above of E_s(p) * p^(lo_s - hi), E_s = rank s's partial evaluation relative to lo_s
    Fr carry_from(const std::vector<uint8_t> &all, size_t slot_bytes, size_t idx, const Fr &p, size_t hi) const {
        Fr c = Fr::zero();
        for (uint32_t r = 0; r < pk->shard_world; ++r) {
            if (rank_ranges[r].second == 0 || rank_ranges[r].first < hi) continue;
            Fr e;
            memcpy(&e, all.data() + (size_t)r * slot_bytes + 8 + sizeof(Fr) * idx, sizeof(Fr));
            c = fe_add(c, fe_mul(e, fe_pow_u64(p, rank_ranges[r].first - hi)));
        }
        return c;
    }
};

// Commit helpers: columns -> affine points (-> the transcript)
struct Commit {
    h2hip_ctx *ctx;
    h2hip_plonk_pk *pk;
    ShardLink *link;
    ProverTranscript *tr;
    // `bases_per_col`: empty = all columns over `bases`.  `hooks` (optional; BatchMsmHooks, internal.h): every hook given to a commitment that
    // succeeds has run exactly once when it returns
    int points_multi(const h2hip_bases *bases, const std::vector<const h2hip_bases *> &bases_per_col, const std::vector<const void *> &cols, size_t len,
                     std::vector<G1Affine> &pts, const BatchMsmHooks *hooks = nullptr) {
        std::vector<G1Jac> jac(cols.size());
        const bool sharded = link->on();
        std::vector<const h2hip_bases *> bpc(cols.size());
        for (size_t i = 0; i < cols.size(); ++i) {
            const h2hip_bases *b = bases_per_col.empty() ? bases : bases_per_col[i];
            bpc[i] = sharded ? (b == pk->g ? pk->g_shard : pk->g_lagrange_shard) : b;
        }
        // sharded: point-range sharding: this rank's partial MSM over its resident slice of the SRS, one all-gather of the
        // 96-byte partials per round (RCCL has no group-law reduction), the N-term sums on the host.  Every rank ends up with every
        // commitment, so the replicated transcripts stay in lock step and all ranks emit the same proof bytes.
        const size_t lo = link->lo(len), hi = link->hi(len);
        std::vector<const void *> local(cols.size());
        for (size_t i = 0; i < cols.size(); ++i) local[i] = (const Fr *)cols[i] + lo;
        // (r05 ran a lone commitment — SHPLONK's W and W' — as 2 / 4 point-range parts on the batch API's lanes, co-running accumulations and shorter
        // sorts against one more join: the k = 19 proof 13.2-13.4 / 13.5-13.7 vs 13.0-13.1 ms, k = 21 51.6-52.5 vs 49.8-51.8: slower, removed —
        // profiles/r05_split_single_msm_ab.log)
        if (cols.size() >= 2) {
            H2_CHK(msm_batch(ctx, nullptr, bpc.data(), local.data(), false, hi - lo, cols.size(), H2HIP_POINT_JACOBIAN, jac.data(), hooks));
        } else {   // the lone MSM has no lanes to join: `tail` runs behind what the main stream holds after it
            H2_REQUIRE(!hooks || (!hooks->mid && !hooks->col), "internal: `mid` / `col` need a batch of two or more columns");
            if (cols.size() == 1) H2_CHK(h2hip_msm_g1_dev(ctx, bpc[0], local[0], hi - lo, H2HIP_POINT_JACOBIAN, jac.data()));
            if (hooks && hooks->tail) {
                if (!ctx->tail_ev) H2_HIPCHK(hipEventCreateWithFlags(&ctx->tail_ev, hipEventDisableTiming));
                H2_HIPCHK(hipEventRecord(ctx->tail_ev, ctx->stream));
                H2_CHK(hooks->tail(ctx->tail_ev));
            }
        }
        pts.resize(cols.size());
        if (sharded) {
            std::vector<uint8_t> all;
            H2_CHK(link->exchange(jac.data(), sizeof(G1Jac) * cols.size(), all));
            const size_t slot = 8 + sizeof(G1Jac) * cols.size();
            for (size_t i = 0; i < cols.size(); ++i) {
                XYZZ acc = XYZZ::identity();
                for (uint32_t r = 0; r < pk->shard_world; ++r) {
                    G1Jac p;
                    memcpy(&p, all.data() + (size_t)r * slot + 8 + sizeof(G1Jac) * i, sizeof(G1Jac));
                    if (p.z.is_zero()) continue;
                    XYZZ q;
                    q.x = p.x;
                    q.y = p.y;
                    q.zz = fe_sqr(p.z);
                    q.zzz = fe_mul(q.zz, p.z);
                    xyzz_add(acc, q);
                }
                pts[i] = xyzz_to_affine(acc);
            }
            return H2HIP_OK;
        }
        // commitments come back as Jacobian points (C::Curve, like best_multiexp) and are normalised here: one field inversion on the
        // host costs microseconds, on a single GPU lane ~0.1 ms of an otherwise idle chip
        for (size_t i = 0; i < jac.size(); ++i) pts[i] = jacobian_to_affine(jac[i]);
        return H2HIP_OK;
    }
    int points(const h2hip_bases *bases, const std::vector<const void *> &cols, size_t len, std::vector<G1Affine> &pts, const BatchMsmHooks *hooks = nullptr) {
        return points_multi(bases, std::vector<const h2hip_bases *>(), cols, len, pts, hooks);
    }
    int batch(const h2hip_bases *bases, const std::vector<const void *> &cols, size_t len) {   // ... each point written to the transcript
        std::vector<G1Affine> pts;
        H2_CHK(points(bases, cols, len, pts));
        for (const G1Affine &p : pts) H2_CHK(tr->write_point(p));
        return H2HIP_OK;
    }
};

// Side stream.  Tail overlap (r04): a commitment round ends with the MSMs' bucket reduction: ~0.25 ms of dependent point additions on a few
// waves while the rest of the chip idles.  Rounds 1 and 3 are followed by transforms that do not depend on the round's challenge (the
// coefficient and extended forms of the columns just committed): they are queued on a side stream (a child context: own NTT scratch and
// twiddle cache) behind the event the batch MSM records once its accumulations are done, read the Lagrange values the MSM also reads and
// write NEW buffers, so they run next to the reduction and to the pointwise kernels that follow.  Single GPU only.
// r05, sharded proofs: lagrange_to_coeff (with its all-gather of the coefficient forms when the columns are dealt to the ranks) and the cosets'
// coeff_to_extended of the FIRST-ROUND columns run on the side context next to round 2's commitments instead of in front of them.
// (r04 also computed the random polynomial's COMMITMENT ahead — its scalars depend on nothing once the generator is counter-mode — as one
// MSM on a second side context behind round 1's accumulations: 14.72-14.99 vs 14.71-14.98 ms, profiles/archive/r04_tail_overlap_ab.log.  The
// chip is busy with something ~97 % of the time; only work moved into LOW-occupancy stretches gains, and that MSM is not such work.  Removed.)
// Which contexts run the side work.  The device serves its streams through a handful of hardware queues (4 by default: with more,
// measured, everything gets slower), and the batch MSM's lanes already hold as many: a further stream shares a queue with one of them.
// After a round's accumulations the lanes idle until the next round, so by default the side work runs ON the last lane's context
// (a full context: own stream, NTT scratch, twiddle cache); a separate context only where that lane does not exist (one lane from 2^20
// points on) or with plonk_side_on_lanes = 0.
struct SideBatch {   // columns transformed out of place on the side stream: Lagrange sources, new coefficient and extended forms
    std::vector<Fr *> src, coef, cos;
};
struct SideStream {
    h2hip_ctx *ctx;
    h2hip_plonk_pk *pk;
    Scope *sc;
    h2hip_ctx *c = nullptr;             // the context the side work runs on; chosen once per proof: join() waits for ONE stream's event
    bool busy = false;                  // work is queued on the side stream that the main stream has not waited for yet
    bool r1_recorded = false;           // side_ev1 marks the end of the first-round columns' transforms on the side stream
    std::vector<Fr *> deferred;         // helpers of work queued here: back to the pool only after join() (the pool hands buffers out in the order of the MAIN stream)
    std::vector<Fr *> lagrange_done;    // Lagrange-form buffers the side stream may still be reading: released after join()
    int pick(h2hip_ctx *lane) {
        if (!c) {
            c = (ctx->plonk_side_on_lanes && lane) ? lane : pk->side;
            if (!c && h2hip_init(ctx->device, nullptr, &pk->side) == H2HIP_OK) c = pk->side;
            if (c) inherit_knobs(c, ctx);
        }
        H2_REQUIRE(c, "create_proof: no side context");
        return H2HIP_OK;
    }
    int wait_for_main() {   // what is queued here next runs after everything the main stream holds so far
        if (!ctx->tail_ev) H2_HIPCHK(hipEventCreateWithFlags(&ctx->tail_ev, hipEventDisableTiming));
        H2_HIPCHK(hipEventRecord(ctx->tail_ev, ctx->stream));
        H2_HIPCHK(hipStreamWaitEvent(c->stream, ctx->tail_ev, 0));
        return H2HIP_OK;
    }
    int queued() {   // side_ev: everything queued on the side stream so far
        H2_HIPCHK(hipEventRecord(pk->side_ev, c->stream));
        busy = true;
        return H2HIP_OK;
    }
    // a commitment's BatchMsmHooks::tail that queues `fn` on the side stream behind the batch MSM's accumulations (or, if the commitment took
    // a path without lanes, behind what the main stream holds after it)
    std::function<int(hipEvent_t)> behind_commit(std::function<int()> fn, bool first_round = false) {
        return [this, fn, first_round](hipEvent_t ev) -> int {
            H2_CHK(pick(ctx->lane[2]));
            H2_HIPCHK(hipStreamWaitEvent(c->stream, ev, 0));
            H2_CHK(fn());
            H2_HIPCHK(hipEventRecord(pk->side_ev, c->stream));
            if (first_round) {
                H2_HIPCHK(hipEventRecord(pk->side_ev1, c->stream));
                r1_recorded = true;
            }
            busy = true;
            return H2HIP_OK;
        };
    }
    int join() {   // the main stream continues after everything queued on the side stream
        if (busy) H2_HIPCHK(hipStreamWaitEvent(ctx->stream, pk->side_ev, 0));
        busy = false;
        return H2HIP_OK;
    }
    // out-of-place lagrange_to_coeff + coeff_to_extended of b.src on the side context: b.coef[i] / b.cos[i] are taken here
    // (two halves: plonk_early_intt queues the first in front of a round's commitments and only the second behind their accumulations)
    int to_coeff(SideBatch &b) {
        const Shape &sh = pk->sh;
        const Domain &dom = pk->dom;
        b.coef.assign(b.src.size(), nullptr);
        for (size_t i = 0; i < b.src.size(); ++i) H2_CHK(sc->take(sh.n, &b.coef[i]));
        const Fr out3[3] = {dom.ifft_divisor, dom.ifft_divisor, dom.ifft_divisor};
        return ntt_run_batch(c, b.coef.data(), (const Fr *const *)b.src.data(), b.src.size(), sh.k, dom.omega_inv, sh.n, nullptr, out3);
    }
    int to_ext(SideBatch &b) {
        const Shape &sh = pk->sh;
        b.cos.assign(b.coef.size(), nullptr);
        for (size_t i = 0; i < b.coef.size(); ++i) H2_CHK(sc->take((size_t)1 << sh.extended_k, &b.cos[i]));
        return h2hip_coeff_to_extended_batch_dev(c, (const void *const *)b.coef.data(), sh.k, (void *const *)b.cos.data(), sh.extended_k, b.coef.size(),
                                                 &pk->dom.ext_omega, &pk->dom.zeta);
    }
    int transforms(SideBatch &b) {
        H2_CHK(to_coeff(b));
        return to_ext(b);
    }
};

// One column of the proof in the forms it takes.  A form that does not exist (yet, or any more) is nullptr.
struct Forms {
    Fr *lagrange = nullptr;   // 2^k values, until the column's lagrange_to_coeff (in place: the buffer becomes `coeff`; on the side stream: released after the join)
    Fr *coeff = nullptr;      // 2^k coefficients, from then to the end of the proof
    Fr *coset = nullptr;      // extended-domain evaluations (sharded quotient: [this rank's cosets][n]), until h(X)'s numerator is complete
};
struct LookupColumns {
    Fr *inp = nullptr;         // the compressed input, Lagrange: the advice column itself or (own_inp) a buffer of its own, held until the grand products are done
    bool own_inp = false;
    Fr *inp_coset = nullptr;   // q_lookup * a / the dynamic compression on the extended domain; nullptr: the advice column's coset serves
    Forms ap, sp, z;           // permuted input a', permuted table s', grand product
};
static std::vector<Fr *> lagrange_of(const std::vector<Forms *> &cols) {
    std::vector<Fr *> v(cols.size());
    for (size_t i = 0; i < cols.size(); ++i) v[i] = cols[i]->lagrange;
    return v;
}

// ---------------------------------------------------------------------------------------------- create_proof
// One proof: what crosses a round boundary is a member, every prover round a method (create_proof_impl calls them in order).
struct ProofRun {
    h2hip_ctx *const ctx;
    h2hip_plonk_pk *const pk;
    const Shape &sh;
    const Domain &dom;
    const void *const *const advice;   // the caller's witness columns (phased keys: phase 0's)
    const bool advice_on_device;
    const void *const *const instances;
    const size_t *const instance_lens;
    const h2hip_rng_fill_fn rng;
    void *const rng_user;
    double *const stage_ms;            // non-null: a timed run (every lap synchronises the stream)
    const h2hip_phase_witness *const witness;
    const uint32_t n, k, ek, bf, u;
    const size_t ne;
    const hipStream_t st;
    Scope sc;
    Laps laps;
    ProverTranscript &tr;
    RngStage stage;
    ShardLink link;
    Commit commit;
    SideStream side;
    // ---- the schedule of this proof
    const bool sharded_any, qshard, pshard;
    // (dynamic lookups: the permuted columns wait for theta, so the round-1 overlap schedule does not apply)
    // (multi-phase keys: the later phases' columns exist only after the phase boundaries, so neither does the round-1 overlap)
    const bool overlap;          // single GPU: rounds 1 and 3 hand their columns' transforms to the side stream
    bool side_sharded = false;   // sharded: the first-round columns' transforms run on the side stream (decided in set_up)
    const bool lazy_upload;      // host-resident advice columns behind the first are uploaded inside round 1's commitment batch
    const size_t ncm;            // cosets of the extended domain evaluated here (sharded quotient)
    const size_t ne_loc;         // extended-domain evaluations of a column held by this rank
    // ---- columns
    std::vector<Forms> inst, adv, perm_z;   // instance, advice, permutation grand products
    std::vector<LookupColumns> lks;
    Fr *dyn_table = nullptr;                // dynamic lookups: the compressed table over the 2^k rows (one table for all sets), Lagrange
    Fr *dyn_table_cos = nullptr;            // ... and on the extended domain
    const void *table_sorted;               // sorted keys of the lookup table: the key's, or (dynamic) this proof's
    SideBatch r1, r3;                       // overlap: the first-round columns' / the grand products' transforms on the side stream
    bool products_join_late = false;        // (plonk_gate_before_join) the grand products' transforms are joined inside the quotient pass, behind the gate identities
    Fr *random_poly = nullptr;              // the vanishing argument's random polynomial (coefficients)
    bool rng_ahead = false;                 // ... generated at set-up, on the copy stream, at RNG position rng_ahead_pos
    uint64_t rng_ahead_pos = 0;
    Fr *acc = nullptr;                      // h(X): numerator on the extended domain, then coefficients (quotient_pieces pieces of n)
    Fr *acc_loc = nullptr;                  // = acc, or (sharded quotient) [coset][n] numerators of this rank's cosets (max_cosets slots: the all-gather's send buffer)
    // ---- challenges
    Fr theta = Fr::zero(), beta, gamma, y, x;
    std::vector<Fr> challenges;             // multi-phase keys: the phases' challenges in squeeze order ([0] is the RLC gates' gamma)
    // ---- evaluations -> SHPLONK
    std::vector<const Fr *> polys;          // SHPLONK's polynomial list; Query.poly indexes it
    std::vector<Query> queries;             // the multiopen's queries in upstream's order

    ProofRun(h2hip_ctx *ctx_, h2hip_plonk_pk *pk_, const void *const *advice_, bool advice_on_device_, const void *const *instances_,
             const size_t *instance_lens_, h2hip_rng_fill_fn rng_, void *rng_user_, ProverTranscript &tr_, double *stage_ms_,
             const h2hip_phase_witness *witness_)
        : ctx(ctx_), pk(pk_), sh(pk_->sh), dom(pk_->dom), advice(advice_), advice_on_device(advice_on_device_), instances(instances_),
          instance_lens(instance_lens_), rng(rng_), rng_user(rng_user_), stage_ms(stage_ms_), witness(witness_), n(sh.n), k(sh.k), ek(sh.extended_k),
          bf(sh.blinding_factors), u(sh.usable_rows), ne((size_t)1 << ek), st(ctx_->stream), sc(&pk_->pool), laps(ctx_, stage_ms_), tr(tr_),
          stage{ctx_, pk_, &sc, rng_, rng_user_}, link{ctx_, pk_}, commit{ctx_, pk_, &link, &tr}, side{ctx_, pk_, &sc},
          sharded_any(link.on()), qshard(sharded_any && pk_->shard_quotient), pshard(sharded_any && pk_->shard_products),
          overlap(!sharded_any && ctx_->plonk_tail_overlap != 0 && !sh.dyn && !sh.phased),
          lazy_upload(!advice_on_device_ && overlap && ctx_->plonk_lazy_upload != 0 && sh.num_advice_total >= 2 &&
                      (sh.lookups.empty() || ctx_->plonk_permute_in_commit != 0)),
          ncm(qshard ? pk_->my_cosets.size() : 0), ne_loc(qshard ? std::max<size_t>(ncm * (size_t)n, 1) : ne), inst(sh.p.num_instance),
          adv(sh.num_advice_total), perm_z(sh.num_perm_sets), lks(sh.lookups.size()), table_sorted(pk_->table_sorted) {}

    // ---- column lists and views
    std::vector<Forms *> first_round_columns() {   // advice, instance, then a' / s' per lookup: the order their transforms are batched in
        std::vector<Forms *> c;
        for (Forms &f : adv) c.push_back(&f);
        for (Forms &f : inst) c.push_back(&f);
        for (LookupColumns &s : lks) {
            c.push_back(&s.ap);
            c.push_back(&s.sp);
        }
        return c;
    }
    std::vector<Forms *> product_columns() {   // the permutation sets' grand products, then the lookups'
        std::vector<Forms *> c;
        for (Forms &f : perm_z) c.push_back(&f);
        for (LookupColumns &s : lks) c.push_back(&s.z);
        return c;
    }
    const Fr *column_values(const ColumnRef &c) const {   // Lagrange
        return c.kind == 0 ? pk->fixed_values[c.index] : c.kind == 1 ? adv[c.index].lagrange : inst[c.index].lagrange;
    }
    const Fr *table_values(size_t li) const { return sh.dyn ? dyn_table : pk->fixed_values[sh.lookups[li].table_col]; }
    // the proving key's extended-domain arrays as this rank holds them
    const Fr *fixed_cos(int col) const { return qshard ? pk->fixed_cosets_sh[col] : pk->fixed_cosets[col]; }
    const Fr *sigma_cos(size_t col) const { return qshard ? pk->sigma_cosets_sh[col] : pk->sigma_cosets[col]; }
    const Fr *column_coset(const ColumnRef &c) const {
        return c.kind == 0 ? fixed_cos(c.index) : c.kind == 1 ? adv[c.index].coset : inst[c.index].coset;
    }
    // the shift of coset c of the extended domain: s_c = zeta * omega_e^c (rows i = (j << (ek - k)) + c are the points s_c * omega^j)
    Fr coset_shift(uint32_t c) const { return fe_mul(dom.zeta, fe_pow_u64(dom.ext_omega, c)); }

    // ---- 1. set-up: staging buffer, ahead-of-time random polynomial, side events, exchange schedule
    int set_up() {
        // the RNG writes straight into pinned host memory, from where the DMA engine takes it (n scalars for the random polynomial)
        if (!pk->copy_stream) {
            H2_HIPCHK(hipStreamCreateWithFlags(&pk->copy_stream, hipStreamNonBlocking));
            H2_HIPCHK(hipEventCreateWithFlags(&pk->copy_ev, hipEventDisableTiming));
        }
        const size_t stage_cap = (size_t)n + ((size_t)1 << 14);   // the blinding tails of a proof and the n random-polynomial scalars without wrapping
        if (pk->host_stage_elems < stage_cap) {
            if (pk->host_stage) hipHostFree(pk->host_stage);
            pk->host_stage = nullptr;
            pk->host_stage_elems = 0;
            H2_HIPCHK(hipHostMalloc((void **)&pk->host_stage, sizeof(Fr) * stage_cap, 0));
            pk->host_stage_elems = stage_cap;
        }
        // the vanishing argument's random polynomial: with libh2hip's counter-mode generator its n scalars are a function of (seed, position),
        // and the position of that draw follows from the shape — generated NOW, on the copy stream, next to the first rounds
        if (rng == h2hip_chacha_rng_fill && rng_user) {
            const h2hip_chacha_rng *cr = (const h2hip_chacha_rng *)rng_user;
            const uint64_t L = sh.lookups.size(), S = sh.num_perm_sets, A = sh.num_advice_total;
            rng_ahead_pos = cr->pos + A * (uint64_t)(n - u) + A + L * (2 * ((uint64_t)bf + 1) + 2) + S * ((uint64_t)bf + 1) + L * ((uint64_t)bf + 1);
            H2_CHK(sc.take(n, &random_poly));
            H2_CHK(rng_chacha_fill_dev(ctx, random_poly, n, cr->seed, cr->rounds, rng_ahead_pos, pk->copy_stream));
            H2_HIPCHK(hipEventRecord(pk->copy_ev, pk->copy_stream));
            rng_ahead = true;
        }
        // with RCCL and more than one rank the side stream's all-gather and the main stream's host exchanges would use ONE communicator from
        // two streams at once — a pattern no run has exercised (no box shows more than one device: profiles/r06_rccl_cpx_refusal.log); until one does, the
        // side stream carries collectives only over the callback transport (which blocks the host anyway) or when plonk_shard_side = 2 forces it
        int comm_world = 1, comm_rccl = 0;
        if (sharded_any) h2hip_comm_info(pk->comm, &comm_world, nullptr, &comm_rccl);
        side_sharded = sharded_any && (ctx->plonk_shard_side == 2 || (ctx->plonk_shard_side == 1 && !(comm_rccl && comm_world > 1)));
        if ((overlap || side_sharded) && !pk->side_ev) H2_HIPCHK(hipEventCreateWithFlags(&pk->side_ev, hipEventDisableTiming));
        if (overlap && !pk->side_ev1) H2_HIPCHK(hipEventCreateWithFlags(&pk->side_ev1, hipEventDisableTiming));
        link.schedule(sh, qshard);
        return tr.common_scalar(pk->transcript_repr);   // vk.hash_into(transcript)
    }

    // ---- 2. instance columns: values are hashed, not committed (KZG: QUERY_INSTANCE = false)
    int instance_columns() {
        for (uint32_t i = 0; i < sh.p.num_instance; ++i) {
            const size_t len = instance_lens ? instance_lens[i] : 0;
            H2_REQUIRE(len <= u, "InstanceTooLarge");
            H2_REQUIRE(len == 0 || (instances && instances[i]), "NULL instance column");
            std::vector<Fr> vals(len ? len : 1);   // the caller's buffer need not be aligned like Fr
            if (len) memcpy(vals.data(), instances[i], sizeof(Fr) * len);
            for (size_t j = 0; j < len; ++j) H2_CHK(tr.common_scalar(vals[j]));
            H2_CHK(sc.take(n, &inst[i].lagrange));
            H2_HIPCHK(hipMemsetAsync(inst[i].lagrange, 0, sizeof(Fr) * n, st));
            H2_CHK(stage.put(inst[i].lagrange, vals.data(), len));
            H2_HIPCHK(hipStreamSynchronize(st));
        }
        return H2HIP_OK;
    }

    // ---- 3. advice columns: witness rows from the caller, blinding rows from the RNG
    // a phase's blinding rows and blinds (multi-phase keys: phase by phase, each once the phase's witness is in its columns)
    int blind_phase(const std::vector<int> &pcols) {
        TailRun tails;
        stage.reserve(tails, pcols.size(), n - u, n - u);
        for (int c : pcols) H2_CHK(stage.add(tails, adv[c].lagrange + u, stage.draw(n - u)));
        H2_CHK(stage.flush(tails));
        stage.draw(pcols.size());   // Blind(Fr::random) per column
        return H2HIP_OK;
    }
    int advice_columns() {
        const hipMemcpyKind kind = advice_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        if (sh.phased) {   // `advice` holds phase 0's columns; the later phases' are zeroed here and filled by the witness callback
            for (Forms &f : adv) H2_CHK(sc.take(n, &f.lagrange));
            const std::vector<int> &p0 = sh.phase_cols[0];
            for (size_t j = 0; j < p0.size(); ++j) {
                H2_REQUIRE(advice[j], "NULL advice column");
                H2_HIPCHK(hipMemcpyAsync(adv[p0[j]].lagrange, advice[j], sizeof(Fr) * u, kind, st));
            }
            for (size_t ph = 1; ph < sh.phase_cols.size(); ++ph)
                for (int c : sh.phase_cols[ph]) H2_HIPCHK(hipMemsetAsync(adv[c].lagrange, 0, sizeof(Fr) * n, st));
            return blind_phase(p0);
        }
        TailRun tails;
        stage.reserve(tails, sh.num_advice_total, n - u, n - u);
        for (uint32_t c = 0; c < sh.num_advice_total; ++c) {
            H2_REQUIRE(advice[c], "NULL advice column");
            H2_CHK(sc.take(n, &adv[c].lagrange));
            // r06: host-resident columns behind the first are uploaded INSIDE round 1's commitment batch (`col` in round1_base), each right before its
            // MSM is queued: the pageable copy blocks the host, not the GPU, which is working on the columns before it by then
            if (!(lazy_upload && c >= 1)) H2_HIPCHK(hipMemcpyAsync(adv[c].lagrange, advice[c], sizeof(Fr) * u, kind, st));
            const Fr *tail = stage.draw(n - u);
            H2_CHK(stage.add(tails, adv[c].lagrange + u, tail));
        }
        H2_CHK(stage.flush(tails));
        stage.draw(sh.num_advice_total);   // Blind(Fr::random) per column: drawn, unused by KZG
        return H2HIP_OK;
    }

    // ---- 4. sharded: every rank must run the same proof: same shape, same RNG stream (a digest of the first column's blinding rows), and point
    // ranges that tile [0, n) — otherwise the ranks would emit a proof that fails to verify without any of them noticing
    int shard_hello() {
        if (!sharded_any) return H2HIP_OK;
        struct Hello {
            uint64_t offset, len, rank, k, ncols, digest[4];
        } me;
        me.offset = pk->shard_offset;
        me.len = pk->shard_len;
        me.rank = pk->shard_rank;
        me.k = k;
        // + the stages sharded and whether the grand products' rows are routed by an all-to-all (plonk_route_rows, which only acts with
        // shard_ntt): the exchange schedule depends on them, and ranks that disagree would issue different collectives (finding 2).
        // (plonk_shard_side is not folded in: it moves the first-round transforms' all-gather to another stream, but every rank still issues the
        // same collectives in the same host order.)
        const bool route_rows = pk->shard_ntt && ctx->plonk_route_rows != 0;
        me.ncols = (uint64_t)sh.num_advice_total | (uint64_t)(pk->shard_quotient ? 1 : 0) << 32 | (uint64_t)(pk->shard_products ? 1 : 0) << 33 |
                   (uint64_t)(pk->shard_ntt ? 1 : 0) << 34 | (uint64_t)(route_rows ? 1 : 0) << 35;
        {
            Blake2b h(32, "h2hip-shard-rng");
            h.update(pk->host_stage, sizeof(Fr) * (size_t)(n - u));   // the first draw of this proof sits at the start of the staging buffer
            uint8_t d[32];
            h.digest(d);
            memcpy(me.digest, d, 32);
        }
        std::vector<uint8_t> all;
        H2_CHK(link.exchange(&me, sizeof(me), all));
        std::vector<std::pair<uint64_t, uint64_t>> ranges;
        for (uint32_t r = 0; r < pk->shard_world; ++r) {
            Hello o;
            memcpy(&o, all.data() + (size_t)r * (8 + sizeof(Hello)) + 8, sizeof(Hello));
            if (o.k != me.k || o.ncols != me.ncols || memcmp(o.digest, me.digest, 32) != 0 || o.rank != r) {
                set_error("create_proof: rank %u of the sharded proof runs a different proof (shape, sharded stages, row routing, rank order or RNG stream differ)", r);
                return H2HIP_ERR_INVALID;
            }
            ranges.push_back({o.offset, o.len});
        }
        link.rank_ranges = ranges;   // by rank, for the carries of the range divisions
        std::sort(ranges.begin(), ranges.end());
        uint64_t pos = 0;
        for (auto &rg : ranges) {
            if (rg.first != pos) {
                set_error("create_proof: the ranks' point ranges do not tile [0, 2^k)");
                return H2HIP_ERR_INVALID;
            }
            pos += rg.second;
        }
        if (pos != n) {
            set_error("create_proof: the ranks' point ranges do not tile [0, 2^k)");
            return H2HIP_ERR_INVALID;
        }
        return H2HIP_OK;
    }

    // ---- 5. round 1: the advice commitments, theta, the lookups' permuted columns and their commitments, in one of three variants
    int round1() {
        laps.lap(ST_UPLOAD);
        std::vector<const void *> cols;   // this round's commitments: the advice columns, then a' / s' per lookup
        for (Forms &f : adv) cols.push_back(f.lagrange);
        for (size_t li = 0; li < sh.lookups.size(); ++li) {
            const Lookup &l = sh.lookups[li];
            LookupColumns &s = lks[li];
            s.own_inp = l.q_col >= 0 || sh.dyn;
            if (s.own_inp) H2_CHK(sc.take(n, &s.inp));
            else s.inp = adv[l.advice_col].lagrange;
            H2_CHK(sc.take(n, &s.ap.lagrange));
            H2_CHK(sc.take(n, &s.sp.lagrange));
            cols.push_back(s.ap.lagrange);
            cols.push_back(s.sp.lagrange);
        }
        const std::vector<const void *> lookup_cols(cols.begin() + (long)adv.size(), cols.end());
        return sh.phased ? round1_phased(lookup_cols) : sh.dyn ? round1_dynamic(lookup_cols) : round1_base(cols);
    }
    // the permutation itself (a dozen small, latency-bound launches and two host synchronisations: ~0.3 ms at k = 19) and the blinding rows
    int permute_lookups() {
        for (size_t li = 0; li < sh.lookups.size(); ++li) {
            const Lookup &l = sh.lookups[li];
            if (l.q_col >= 0) H2_CHK(h2hip_fr_mul_batch_dev(ctx, lks[li].inp, pk->fixed_values[l.q_col], adv[l.advice_col].lagrange, n));
        }
        {   // all lookups read the one table column: their multiset checks come back in one host synchronisation
            std::vector<const void *> ins(lks.size());
            std::vector<void *> aps(lks.size()), sps(lks.size());
            for (size_t li = 0; li < lks.size(); ++li) {
                ins[li] = lks[li].inp;
                aps[li] = lks[li].ap.lagrange;
                sps[li] = lks[li].sp.lagrange;
            }
            if (!lks.empty()) H2_CHK(h2hip_lookup_permute_presorted_batch_dev(ctx, ins.data(), table_sorted, u, aps.data(), sps.data(), lks.size()));
        }
        TailRun ta, ts;   // per lookup the staging holds [a' rows][s' rows][2 blinds]
        stage.reserve(ta, lks.size(), 2 * ((size_t)bf + 1) + 2, bf + 1);
        ts = ta;
        for (LookupColumns &s : lks) {
            const Fr *t1 = stage.draw(bf + 1);
            H2_CHK(stage.add(ta, s.ap.lagrange + u, t1));
            const Fr *t2 = stage.draw(bf + 1);
            H2_CHK(stage.add(ts, s.sp.lagrange + u, t2));
            stage.draw(2);   // the two commitment blinds
        }
        H2_CHK(stage.flush(ta));
        return stage.flush(ts);
    }
    // BaseConfig, one phase.  Every lookup of halo2-base compresses a single (input, table) expression pair, so theta does not enter the
    // values: the permuted columns are computed before the advice commitments are out, and all of this round's and the next round's
    // commitments go through ONE batched MSM call (the transcript still sees them in upstream's order)
    int round1_base(const std::vector<const void *> &cols) {
        BatchMsmHooks hooks;
        // r04: the ADVICE columns' commitments do not wait for the permutation — the batch MSM queues them on its lanes first, then calls the
        // permutation (on this stream), then queues the permuted columns behind it (`mid`): the first accumulation starts ~0.3 ms earlier
        if (overlap && ctx->plonk_permute_in_commit && !lks.empty() && !adv.empty()) {
            hooks.mid = [this]() -> int { return permute_lookups(); };
            hooks.mid_after = adv.size();
        } else {
            H2_CHK(permute_lookups());
        }
        laps.lap(ST_LOOKUP_PERMUTE);
        std::vector<G1Affine> pts;
        if (overlap) {   // this round's columns -> coefficient and extended form, next to the commitments' reduction and the grand products
            r1.src = lagrange_of(first_round_columns());
            hooks.tail = side.behind_commit([this]() -> int { return side.transforms(r1); }, true);
        }
        if (lazy_upload) {
            hooks.col = [this](size_t j) -> int {
                if (j >= 1 && j < adv.size()) H2_HIPCHK(hipMemcpyAsync(adv[j].lagrange, advice[j], sizeof(Fr) * u, hipMemcpyHostToDevice, st));
                return H2HIP_OK;
            };
        }
        H2_CHK(commit.points(pk->g_lagrange, cols, n, pts, &hooks));
        for (size_t i = 0; i < adv.size(); ++i) H2_CHK(tr.write_point(pts[i]));
        H2_CHK(tr.squeeze_challenge(theta));   // (BaseConfig: every lookup is a single expression, theta does not enter the values)
        for (size_t i = adv.size(); i < pts.size(); ++i) H2_CHK(tr.write_point(pts[i]));
        laps.lap(ST_COMMIT_ROUND1);
        return H2HIP_OK;
    }
    // Dynamic lookups (BasicDynLookupConfig): theta enters the compressed values, so upstream's order is kept literally — the advice
    // commitments, theta, then the compression of every set's input and of the table in ONE launch, the per-proof sort of the table
    // and the batched presorted permutation, then the permuted columns' commitments
    int round1_dynamic(const std::vector<const void *> &lookup_cols) {
        std::vector<const void *> acols;
        for (Forms &f : adv) acols.push_back(f.lagrange);
        H2_CHK(commit.batch(pk->g_lagrange, acols, n));
        H2_CHK(tr.squeeze_challenge(theta));
        H2_CHK(sc.take(n, &dyn_table));
        std::vector<const Fr *> ccols;
        std::vector<Fr *> couts;
        for (size_t li = 0; li < lks.size(); ++li) {
            for (const ColumnRef &c : sh.lookups[li].in) ccols.push_back(column_values(c));
            couts.push_back(lks[li].inp);
        }
        for (const ColumnRef &c : sh.lookups[0].tab) ccols.push_back(column_values(c));
        couts.push_back(dyn_table);
        H2_CHK(lookup_compress_batch_dev(ctx, ccols.data(), couts.data(), (uint32_t)couts.size(), sh.key_cols + 1, n, theta));
        Fr *ts = nullptr;   // sorted keys (Key256, 32 bytes like an Fr) of the compressed table's usable rows
        H2_CHK(sc.take(h2hip_lookup_sorted_table_bytes(u) / sizeof(Fr), &ts));
        H2_CHK(h2hip_lookup_table_sort_dev(ctx, dyn_table, u, ts));
        table_sorted = ts;
        H2_CHK(permute_lookups());
        laps.lap(ST_LOOKUP_PERMUTE);
        H2_CHK(commit.batch(pk->g_lagrange, lookup_cols, n));
        laps.lap(ST_COMMIT_ROUND1);
        return H2HIP_OK;
    }
    // Multi-phase keys [UPSTREAM-RECALL: create_proof's per-phase loop]: per phase its columns' commitments as ONE batched MSM call,
    // the phase's challenges, then the next phase's witness from the caller (at a quiescent point: only the points made the round
    // trip) and its blinding rows.  The range lookups' permuted columns wait for the last phase and go out after theta, as upstream's.
    int round1_phased(const std::vector<const void *> &lookup_cols) {
        for (size_t ph = 0; ph < sh.phase_cols.size(); ++ph) {
            const std::vector<int> &pcols = sh.phase_cols[ph];
            if (ph > 0) {
                H2_HIPCHK(hipStreamSynchronize(st));
                if (witness && witness->fill) {
                    std::vector<void *> dcols;
                    for (int c : pcols) dcols.push_back(adv[c].lagrange);
                    const int wrc = witness->fill(witness->user, (uint32_t)ph, challenges.data(), challenges.size(), dcols.data(), dcols.size());
                    if (wrc != 0) {
                        set_error("create_proof: the witness callback of phase %zu returned %d", ph, wrc);
                        return H2HIP_ERR_INVALID;
                    }
                }
                H2_CHK(blind_phase(pcols));
            }
            std::vector<const void *> pc(pcols.size());
            for (size_t i = 0; i < pcols.size(); ++i) pc[i] = adv[pcols[i]].lagrange;
            H2_CHK(commit.batch(pk->g_lagrange, pc, n));
            for (uint32_t c = 0; c < sh.phase_challenges[ph]; ++c) {
                Fr ch;
                H2_CHK(tr.squeeze_challenge(ch));
                challenges.push_back(ch);
            }
        }
        laps.lap(ST_COMMIT_ROUND1);
        H2_CHK(tr.squeeze_challenge(theta));
        H2_CHK(permute_lookups());
        laps.lap(ST_LOOKUP_PERMUTE);
        H2_CHK(commit.batch(pk->g_lagrange, lookup_cols, n));
        laps.lap(ST_COMMIT_ROUND1);
        return H2HIP_OK;
    }

    // ---- 6./7. grand products: permutation sets (chained through the last usable row), then the lookups.  The factors of all sets (all lookups)
    // are laid out back to back and go through one batched inversion and one prefix product: over the concatenated sets that prefix product
    // IS the chain z_i(0) = z_{i-1}(last usable row), so neither a host round trip nor a rescaling pass is needed.
    int grand_products() {
        H2_CHK(tr.squeeze_challenge(beta));
        H2_CHK(tr.squeeze_challenge(gamma));
        H2_CHK(pshard ? products_by_row_range() : products_local());
        laps.lap(ST_PRODUCTS);
        return H2HIP_OK;
    }
    // the blinding rows of product columns (Lagrange) and one blind per column
    int blind_products(const std::vector<Fr *> &zcols) {
        TailRun tz;
        stage.reserve(tz, zcols.size(), (size_t)bf + 1, bf);
        for (Fr *z : zcols) {
            const Fr *tail = stage.draw(bf);
            H2_CHK(stage.add(tz, z + (n - bf), tail));
            stage.draw(1);   // blind
        }
        return stage.flush(tz);
    }
    int permutation_terms(Fr *num, Fr *den, size_t first_row, size_t rows, bool by_rows) {
        std::vector<const void *> pcols(sh.perm_columns.size()), psig(sh.perm_columns.size());
        for (size_t c = 0; c < sh.perm_columns.size(); ++c) {
            pcols[c] = column_values(sh.perm_columns[c]);
            psig[c] = pk->sigma_values[c];
        }
        if (by_rows)
            return h2hip_permutation_product_terms_rows_dev(ctx, num, den, pcols.data(), psig.data(), (uint32_t)pcols.size(), sh.chunk_len, first_row, rows, &beta,
                                                            &gamma, &dom.delta, &dom.omega);
        return h2hip_permutation_product_terms_sets_dev(ctx, num, den, pcols.data(), psig.data(), (uint32_t)pcols.size(), sh.chunk_len, rows, &beta, &gamma,
                                                        &dom.delta, &dom.omega);
    }
    int products_local() {
        // r05: with ONE permutation set (nothing to chain) the permutation's and the lookups' factors go through ONE batched inversion and ONE
        // prefix product — segments [set | lookup 0 | lookup 1 ...] — instead of two passes of seven launches each (the k = 19 ECDSA shape: the second
        // pass was ~0.25 ms of small launches on the critical path).  Same values: every segment is its own product either way.
        const bool merged = ctx->plonk_merge_products != 0 && sh.num_perm_sets == 1 && !lks.empty();
        const size_t segs = merged ? 1 + lks.size() : std::max<size_t>(sh.num_perm_sets, lks.size());
        Fr *num = nullptr, *den = nullptr;
        if (segs) {
            H2_CHK(sc.take(segs * (size_t)u, &num));
            H2_CHK(sc.take(segs * (size_t)u, &den));
        }
        if (sh.num_perm_sets) H2_CHK(permutation_terms(num, den, 0, u, false));
        std::vector<Fr *> pz(sh.num_perm_sets);
        for (uint32_t si = 0; si < sh.num_perm_sets; ++si) {
            H2_CHK(sc.take(n, &perm_z[si].lagrange));
            pz[si] = perm_z[si].lagrange;
        }
        if (sh.num_perm_sets && !merged) H2_CHK(h2hip_fr_grand_products_dev(ctx, (void *const *)pz.data(), num, den, sh.num_perm_sets, u, 1));
        H2_CHK(blind_products(pz));
        std::vector<Fr *> lk_z(lks.size());
        const size_t lk0 = merged ? 1 : 0;   // the lookups' first segment
        for (size_t li = 0; li < lks.size(); ++li) {
            LookupColumns &s = lks[li];
            H2_CHK(h2hip_lookup_product_terms_dev(ctx, num + (lk0 + li) * (size_t)u, den + (lk0 + li) * (size_t)u, s.inp, table_values(li), s.ap.lagrange,
                                                  s.sp.lagrange, u, &beta, &gamma));
            H2_CHK(sc.take(n, &s.z.lagrange));
            lk_z[li] = s.z.lagrange;
        }
        if (merged) {
            std::vector<void *> all_z(1, pz[0]);
            all_z.insert(all_z.end(), lk_z.begin(), lk_z.end());
            H2_CHK(h2hip_fr_grand_products_dev(ctx, all_z.data(), num, den, all_z.size(), u, 0));
        } else if (!lks.empty()) {
            H2_CHK(h2hip_fr_grand_products_dev(ctx, (void *const *)lk_z.data(), num, den, lks.size(), u, 0));
        }
        H2_CHK(blind_products(lk_z));
        if (num) sc.release(num);
        if (den) sc.release(den);
        return H2HIP_OK;
    }
    int products_by_row_range() {
        // Sharded by ROW RANGE (r04): a product column is a prefix product over the rows, so rank r forms the factors of its rows [a, b) — the
        // rows of its point range below the blinding rows — inverts and multiplies them up locally (1/N of the single-GPU work), the ranks
        // exchange their ranges' total products (32 bytes per product), every rank scales its rows by the product of everything before them (for
        // the permutation argument that includes the earlier sets: z_i(0) = z_{i-1}(last usable row)), and ONE device-to-device all-gather
        // completes the columns on every rank (their coefficient forms are needed everywhere).  This rank's commitment partials only read its
        // own rows.  The blinding rows come from the (replicated) RNG stream.
        const std::vector<std::pair<uint64_t, uint64_t>> &rank_ranges = link.rank_ranges;
        const size_t S = sh.num_perm_sets, nseg = S + lks.size();
        const size_t a = link.lo(u), b = link.hi(u), m = b - a;
        size_t max_m = 0;
        for (auto &rg : rank_ranges) max_m = std::max<size_t>(max_m, std::min<size_t>(rg.first + rg.second, u) - std::min<size_t>(rg.first, u));
        // r06 (built): when lagrange_to_coeff is dealt by column, a product column's rows are only ever needed in full by the rank that
        // transforms it (commitments read a rank's own rows, everything later the coefficient forms) — so the rows go STRAIGHT to the column's owner
        // (column j -> rank j mod N, the order to_coeff deals in) by an all-to-all (grouped ncclSend / ncclRecv: h2hip_comm_alltoall_dev) instead
        // of to everybody by an all-gather: a rank receives 1 / N of the bytes, each block over its own xGMI link.
        const uint32_t NW = pk->shard_world;
        const bool route = pk->shard_ntt && ctx->plonk_route_rows != 0;
        const size_t row_stride = max_m + 1, slot_cols = (nseg + NW - 1) / NW, blk_elems = slot_cols * row_stride;
        const size_t slot_elems = route ? blk_elems * NW : nseg * row_stride;
        Fr *num = nullptr, *den = nullptr, *sendb = nullptr, *recvb = nullptr;
        if (nseg) {
            H2_CHK(sc.take(nseg * std::max<size_t>(m, 1), &num));
            H2_CHK(sc.take(nseg * std::max<size_t>(m, 1), &den));
            H2_CHK(sc.take(slot_elems, &sendb));
            H2_CHK(sc.take(route ? slot_elems : slot_elems * pk->shard_world, &recvb));
            if (route) H2_CHK(comm_reserve_alltoall_dev(pk->comm, sizeof(Fr) * blk_elems));
            else H2_CHK(comm_reserve_allgather_dev(pk->comm, sizeof(Fr) * slot_elems));
        }
        const std::vector<Forms *> zforms = product_columns();
        for (Forms *f : zforms) H2_CHK(sc.take(n, &f->lagrange));
        const std::vector<Fr *> zcol = lagrange_of(zforms);
        if (S && m) H2_CHK(permutation_terms(num, den, a, m, true));
        for (size_t li = 0; li < lks.size() && m; ++li) {
            LookupColumns &s = lks[li];
            H2_CHK(h2hip_lookup_product_terms_dev(ctx, num + (S + li) * m, den + (S + li) * m, s.inp + a, table_values(li) + a, s.ap.lagrange + a,
                                                  s.sp.lagrange + a, m, &beta, &gamma));
        }
        std::vector<Fr> totals(nseg, Fr::one());
        if (nseg) {
            // local prefix products, each starting at 1: column s gets rows [a, b] (m + 1 values; the last one = this range's total)
            std::vector<void *> zloc(nseg);
            for (size_t j = 0; j < nseg; ++j) zloc[j] = zcol[j] + a;
            H2_CHK(h2hip_fr_grand_products_dev(ctx, zloc.data(), num, den, nseg, m, 0));
            for (size_t j = 0; j < nseg; ++j) H2_HIPCHK(hipMemcpyAsync(&totals[j], zcol[j] + b, sizeof(Fr), hipMemcpyDeviceToHost, st));
            H2_HIPCHK(hipStreamSynchronize(st));
        }
        std::vector<uint8_t> all;
        H2_CHK(link.exchange(totals.data(), sizeof(Fr) * nseg, all));   // (also the go-ahead of the all-gather below: nothing after it can fail on one rank alone)
        if (nseg) {
            const size_t slot = 8 + sizeof(Fr) * nseg;
            Fr chain = Fr::one();   // the permutation sets run on from one another
            for (size_t j = 0; j < nseg; ++j) {
                Fr before = Fr::one(), whole = Fr::one();
                for (uint32_t r = 0; r < pk->shard_world; ++r) {
                    Fr t;
                    memcpy(&t, all.data() + (size_t)r * slot + 8 + sizeof(Fr) * j, sizeof(Fr));
                    whole = fe_mul(whole, t);
                    if (rank_ranges[r].first < pk->shard_offset) before = fe_mul(before, t);
                }
                const Fr start = j < S ? fe_mul(chain, before) : before;
                if (j < S) chain = fe_mul(chain, whole);
                H2_CHK(h2hip_fr_scale_dev(ctx, zcol[j] + a, &start, m + 1));
                Fr *slot = route ? sendb + (j % NW) * blk_elems + (j / NW) * row_stride : sendb + j * row_stride;   // routed: block of the column's owner
                H2_HIPCHK(hipMemcpyAsync(slot, zcol[j] + a, sizeof(Fr) * (m + 1), hipMemcpyDeviceToDevice, st));
            }
            if (route) H2_CHK(h2hip_comm_alltoall_dev(pk->comm, ctx, sendb, sizeof(Fr) * blk_elems, recvb));
            else H2_CHK(h2hip_comm_allgather_dev(pk->comm, ctx, sendb, sizeof(Fr) * slot_elems, recvb));
            for (uint32_t r = 0; r < pk->shard_world; ++r) {
                if (r == pk->shard_rank) continue;
                const size_t ar = std::min<size_t>(rank_ranges[r].first, u), br = std::min<size_t>(rank_ranges[r].first + rank_ranges[r].second, u);
                if (rank_ranges[r].second == 0) continue;
                std::vector<Fr *> dst;
                if (route) {   // rank r's rows of the columns THIS rank transforms
                    for (size_t j = pk->shard_rank; j < nseg; j += NW) dst.push_back(zcol[j] + ar);
                    if (!dst.empty()) H2_CHK(fr_scatter_rows(ctx, dst.data(), dst.size(), recvb + (size_t)r * blk_elems, row_stride, br - ar + 1));
                    continue;
                }
                dst.resize(nseg);
                for (size_t j = 0; j < nseg; ++j) dst[j] = zcol[j] + ar;
                H2_CHK(fr_scatter_rows(ctx, dst.data(), nseg, recvb + (size_t)r * slot_elems, row_stride, br - ar + 1));
            }
        }
        H2_CHK(blind_products(zcol));
        if (recvb) sc.release(recvb);
        if (sendb) sc.release(sendb);
        if (den) sc.release(den);
        if (num) sc.release(num);
        return H2HIP_OK;
    }

    // ---- 8. first-round transforms.  Before the host draws the 2^k random scalars, the GPU is given everything that no longer needs the
    // Lagrange values of the first-round columns: their coefficient and extended forms — RNG, upload (own stream) and NTTs overlap.
    // All columns of a round go through the transforms together (32 per launch): a wide shape's 2^14-row columns are far too small to fill the chip alone.
    // `xc`: the context (stream, NTT scratch) the transforms are queued on — the proof's own, or (r05, sharded) the side context, so that the
    // coefficient forms' all-gather and the cosets' transforms of the first-round columns run NEXT TO the round's commitments.
    // lagrange_to_coeff in place: the columns' Lagrange buffers become their coefficient forms
    int to_coeff(const std::vector<Forms *> &forms, h2hip_ctx *xc) {
        const std::vector<Fr *> cols = lagrange_of(forms);
        for (Forms *f : forms) {
            f->coeff = f->lagrange;
            f->lagrange = nullptr;
        }
        if (!(sharded_any && pk->shard_ntt))
            return h2hip_ifft_batch_dev(xc, (void *const *)cols.data(), cols.size(), &dom.omega_inv, k, &dom.ifft_divisor);
        // Sharded by COLUMN (H2HIP_SHARD_NTT_COLUMNS; north_star: "independent NTT columns shard across the GPUs"): column j is transformed by rank
        // j mod N — in the all-gather's send buffer — and ONE device-to-device all-gather hands every rank every coefficient form (each needs
        // them all: its cosets read whole polynomials).  Pays when a transform takes longer than moving one column between GPUs (k = 21: 0.3 ms
        // against 64 MiB over the links a rank receives on: eight fully connected GPUs, not two).  Everything that can fail on this rank alone
        // comes before the go-ahead exchange.
        const uint32_t N = pk->shard_world, me_ = pk->shard_rank;
        const size_t slot_cols = (cols.size() + N - 1) / N, slot_elems = slot_cols * (size_t)n;
        if (cols.empty()) return link.go_ahead();
        Fr *sendb = nullptr, *recvb = nullptr;
        H2_CHK(sc.take(slot_elems, &sendb));
        H2_CHK(sc.take(slot_elems * N, &recvb));
        std::vector<Fr *> mine;
        for (size_t j = me_; j < cols.size(); j += N) {
            Fr *dst = sendb + (j / N) * (size_t)n;
            H2_HIPCHK(hipMemcpyAsync(dst, cols[j], sizeof(Fr) * n, hipMemcpyDeviceToDevice, xc->stream));
            mine.push_back(dst);
        }
        if (!mine.empty()) H2_CHK(h2hip_ifft_batch_dev(xc, (void *const *)mine.data(), mine.size(), &dom.omega_inv, k, &dom.ifft_divisor));
        H2_CHK(comm_reserve_allgather_dev(pk->comm, sizeof(Fr) * slot_elems));
        H2_CHK(link.go_ahead());
        H2_CHK(h2hip_comm_allgather_dev(pk->comm, xc, sendb, sizeof(Fr) * slot_elems, recvb));
        for (size_t j = 0; j < cols.size(); ++j)
            H2_HIPCHK(hipMemcpyAsync(cols[j], recvb + (j % N) * slot_elems + (j / N) * (size_t)n, sizeof(Fr) * n, hipMemcpyDeviceToDevice, xc->stream));
        for (Fr *p : {recvb, sendb}) {   // queued on the side context: back to the pool only once the side stream has been joined
            if (xc != ctx) side.deferred.push_back(p);
            else sc.release(p);
        }
        return H2HIP_OK;
    }
    // coeff_to_extended on context `xc`: takes the columns' extended forms (sharded quotient: this rank's cosets only)
    int to_ext(const std::vector<Forms *> &forms, h2hip_ctx *xc) {
        std::vector<void *> o(forms.size());
        std::vector<const void *> polys_(forms.size());
        for (size_t i = 0; i < forms.size(); ++i) {
            H2_CHK(sc.take(ne_loc, &forms[i]->coset));
            o[i] = forms[i]->coset;
            polys_[i] = forms[i]->coeff;
        }
        if (!qshard) return h2hip_coeff_to_extended_batch_dev(xc, polys_.data(), k, o.data(), ek, polys_.size(), &dom.ext_omega, &dom.zeta);
        // sharded: only this rank's cosets, each a 2^k-point transform of f(s_c X) — [coset][n] per column
        for (size_t m = 0; m < ncm; ++m) {
            std::vector<void *> om(o.size());
            for (size_t i = 0; i < o.size(); ++i) om[i] = (Fr *)o[i] + m * (size_t)n;
            const Fr s_c = coset_shift(pk->my_cosets[m]);
            H2_CHK(h2hip_fr_coset_scale_batch_dev(xc, om.data(), polys_.data(), polys_.size(), n, &s_c));
            H2_CHK(ntt_run_batch(xc, (Fr *const *)om.data(), nullptr, om.size(), k, dom.omega, 0, nullptr, nullptr));
        }
        return H2HIP_OK;
    }
    // the lookups' compressed inputs on the extended domain, from the extended forms h(X) reads anyway
    int lookup_input_cosets() {
        if (sh.dyn) {
            // compressed from the advice cosets and the key's fixed cosets: one launch, no transform
            std::vector<const Fr *> ccols;
            std::vector<Fr *> couts;
            for (size_t li = 0; li < lks.size(); ++li) {
                H2_CHK(sc.take(ne_loc, &lks[li].inp_coset));
                for (const ColumnRef &c : sh.lookups[li].in) ccols.push_back(column_coset(c));
                couts.push_back(lks[li].inp_coset);
            }
            H2_CHK(sc.take(ne_loc, &dyn_table_cos));
            for (const ColumnRef &c : sh.lookups[0].tab) ccols.push_back(column_coset(c));
            couts.push_back(dyn_table_cos);
            return lookup_compress_batch_dev(ctx, ccols.data(), couts.data(), (uint32_t)couts.size(), sh.key_cols + 1, ne_loc, theta);
        }
        for (size_t li = 0; li < lks.size(); ++li) {
            const Lookup &l = sh.lookups[li];
            if (l.q_col >= 0) {   // the product of the cosets is the coset of the product polynomial q_lookup(X) * a(X)
                H2_CHK(sc.take(ne_loc, &lks[li].inp_coset));
                H2_CHK(h2hip_fr_mul_batch_dev(ctx, lks[li].inp_coset, fixed_cos(l.q_col), adv[l.advice_col].coset, qshard ? ncm * (size_t)n : ne));
            }
        }
        return H2HIP_OK;
    }
    int first_round_transforms() {
        if (!random_poly) H2_CHK(sc.take(n, &random_poly));
        const std::vector<Forms *> round1 = first_round_columns();
        for (LookupColumns &s : lks)
            if (s.own_inp) {
                sc.release(s.inp);   // (a product of this stream, never read by the side stream)
                s.inp = nullptr;
            }
        if (overlap) {
            // the side stream holds (or is still producing) the coefficient and extended forms of the first-round columns; the grand products
            // above were the last readers of their Lagrange values on THIS stream
            for (size_t i = 0; i < round1.size(); ++i) {
                side.lagrange_done.push_back(round1[i]->lagrange);
                *round1[i] = Forms{nullptr, r1.coef[i], r1.cos[i]};
            }
            return H2HIP_OK;   // (the lookup inputs' cosets: after the side stream's extended forms have been joined)
        }
        if (!side_sharded) {
            H2_CHK(to_coeff(round1, ctx));
            H2_CHK(to_ext(round1, ctx));
            return lookup_input_cosets();
        }
        // everything the main stream holds so far (the grand products: the last readers of these columns' Lagrange values) precedes the side
        // work; the main stream goes on with this round's commitments and joins the side stream before the first reader of the cosets
        H2_CHK(side.pick(nullptr));
        H2_CHK(side.wait_for_main());
        H2_CHK(to_coeff(round1, side.c));
        H2_CHK(to_ext(round1, side.c));
        return side.queued();
    }

    // ---- 9. this round's commitments are the grand products AND the vanishing argument's random polynomial (nothing is squeezed between
    // them): one batched call over two base sets
    int commit_products_and_random() {
        if (rng == h2hip_chacha_rng_fill) {
            // libh2hip's own seeded ChaCha generator: counter mode, so the n elements are generated where they are needed — on the
            // device, straight into the polynomial — and the host only advances the stream position (same values as the host callback).
            // Normally they were generated at the start of the proof already (position known from the shape), next to everything else.
            h2hip_chacha_rng *cr = (h2hip_chacha_rng *)rng_user;
            if (rng_ahead && cr->pos == rng_ahead_pos) {
                H2_HIPCHK(hipStreamWaitEvent(st, pk->copy_ev, 0));
            } else {
                if (rng_ahead) H2_HIPCHK(hipStreamWaitEvent(st, pk->copy_ev, 0));   // (the buffer is overwritten in stream order)
                H2_CHK(rng_chacha_fill_dev(ctx, random_poly, n, cr->seed, cr->rounds, cr->pos, st));
            }
            cr->pos += n;
        } else {
            const Fr *vals = stage.draw(n);
            H2_HIPCHK(hipMemcpyAsync(random_poly, vals, sizeof(Fr) * n, hipMemcpyHostToDevice, pk->copy_stream));
            H2_HIPCHK(hipEventRecord(pk->copy_ev, pk->copy_stream));
            H2_HIPCHK(hipStreamWaitEvent(st, pk->copy_ev, 0));
        }
        stage.draw(1);   // random_blind
        const std::vector<Fr *> zs = lagrange_of(product_columns());
        std::vector<const void *> cols(zs.begin(), zs.end());
        std::vector<const h2hip_bases *> bases(cols.size(), pk->g_lagrange);
        cols.push_back(random_poly);
        bases.push_back(pk->g);
        std::vector<G1Affine> pts;
        BatchMsmHooks hooks;
        if (overlap) {   // the grand products' coefficient and extended forms do not depend on y: next to this round's reduction
            r3.src = zs;
            if (ctx->plonk_early_intt) {
                // the products are complete on this stream: their lagrange_to_coeff goes to the side context NOW — it runs next to the round's sorts
                // (and, on the last lane's context, in front of that lane's column: the third accumulation of the round, a millisecond away)
                H2_CHK(side.pick(ctx->lane[2]));
                H2_CHK(side.wait_for_main());
                H2_CHK(side.to_coeff(r3));
                H2_CHK(side.queued());
                hooks.tail = side.behind_commit([this]() -> int { return side.to_ext(r3); });
            } else
                hooks.tail = side.behind_commit([this]() -> int { return side.transforms(r3); });
        }
        H2_CHK(commit.points_multi(nullptr, bases, cols, n, pts, &hooks));
        for (size_t i = 0; i + 1 < pts.size(); ++i) H2_CHK(tr.write_point(pts[i]));
        laps.lap(ST_COMMIT_PRODUCTS);
        H2_CHK(tr.write_point(pts.back()));   // the random polynomial's commitment
        return tr.squeeze_challenge(y);
    }

    // ---- 10. join of the side stream, the grand products' coefficient and extended forms, h(X)'s accumulator
    int join_products() {   // overlap: both rounds' transforms are complete before anything behind this reads their results or reuses their inputs
        H2_CHK(side.join());
        const std::vector<Forms *> zs = product_columns();
        for (size_t i = 0; i < zs.size(); ++i) {
            sc.release(zs[i]->lagrange);
            *zs[i] = Forms{nullptr, r3.coef[i], r3.cos[i]};
        }
        return H2HIP_OK;
    }
    int join_and_extend_products() {
        if (overlap) {
            if (ctx->plonk_gate_before_join && side.r1_recorded && !stage_ms) {
                // the gate identities (and q_lookup * a's cosets) read first-round columns only: they start when THOSE transforms are done — the grand
                // products' coset transforms, queued behind this round's accumulations, are usually still running when y arrives
                H2_HIPCHK(hipStreamWaitEvent(st, pk->side_ev1, 0));
                products_join_late = true;
            } else
                H2_CHK(join_products());
            for (Fr *p : side.lagrange_done) sc.release(p);
            H2_CHK(lookup_input_cosets());
            laps.lap(ST_TO_COEFF);
        } else {
            if (side_sharded) {   // the first-round columns' coefficient forms and cosets are complete; their helpers go back to the pool
                H2_CHK(side.join());
                for (Fr *p : side.deferred) sc.release(p);
                side.deferred.clear();
                H2_CHK(lookup_input_cosets());
            }
            const std::vector<Forms *> zs = product_columns();
            H2_CHK(to_coeff(zs, ctx));
            laps.lap(ST_TO_COEFF);
            H2_CHK(to_ext(zs, ctx));
        }
        H2_CHK(sc.take(ne, &acc));
        acc_loc = acc;
        if (qshard) H2_CHK(sc.take((size_t)pk->max_cosets * n, &acc_loc));
        H2_HIPCHK(hipMemsetAsync(acc_loc, 0, sizeof(Fr) * (qshard ? (size_t)pk->max_cosets * n : ne), st));
        laps.lap(ST_TO_EXT);
        return H2HIP_OK;
    }

    // ---- 11. h(X) numerator on the extended domain: the pointwise identities, folded by y in evaluate_h's order.  All gate columns, the whole
    // permutation argument and all lookups go through batched launches (every launch reads and writes the accumulator once).
    // One pass covers the whole extended domain (single GPU) or one coset of it (sharded: the same kernels on a 2^k-point domain with
    // shift s_c and generator omega; `off` = the coset's offset in the [coset][n] arrays), followed by the division by X^n - 1.
    int quotient_pass(size_t off, uint32_t ek_, const Fr &zeta_, const Fr &w_) {
        {
            std::vector<const void *> gq(sh.p.num_advice), ga(sh.p.num_advice);
            for (uint32_t a = 0; a < sh.p.num_advice; ++a) {
                gq[a] = fixed_cos(sh.first_q_enable_col + (int)a) + off;
                ga[a] = adv[sh.first_gate_advice + a].coset + off;
            }
            H2_CHK(h2hip_quotient_flex_gate_batch_dev(ctx, acc_loc + off, gq.data(), ga.data(), gq.size(), ek_, k, &y));
        }
        if (sh.num_rlc) {   // the RLC gates follow the flex gates in the constraint system's gate list
            H2_REQUIRE(!challenges.empty(), "internal: an RLC key without a challenge");
            std::vector<const void *> gq(sh.num_rlc), ga(sh.num_rlc);
            for (uint32_t j = 0; j < sh.num_rlc; ++j) {
                gq[j] = fixed_cos(sh.first_q_rlc_col + (int)j) + off;
                ga[j] = adv[sh.first_rlc_advice + j].coset + off;
            }
            H2_CHK(h2hip_quotient_rlc_gate_batch_dev(ctx, acc_loc + off, gq.data(), ga.data(), gq.size(), ek_, k, &challenges[0], &y));
        }
        if (products_join_late) {
            products_join_late = false;
            H2_CHK(join_products());
        }
        const Fr *l0 = (qshard ? pk->l0_sh : pk->l0) + off, *l_last = (qshard ? pk->l_last_sh : pk->l_last) + off,
                 *l_blind = (qshard ? pk->l_blind_sh : pk->l_blind) + off;
        if (sh.num_perm_sets) {
            std::vector<const void *> pcols(sh.perm_columns.size()), psig(sh.perm_columns.size()), pz(perm_z.size());
            for (size_t i = 0; i < perm_z.size(); ++i) pz[i] = perm_z[i].coset + off;
            for (size_t c = 0; c < sh.perm_columns.size(); ++c) {
                pcols[c] = column_coset(sh.perm_columns[c]) + off;
                psig[c] = sigma_cos(c) + off;
            }
            H2_CHK(h2hip_quotient_permutation_sets_dev(ctx, acc_loc + off, pz.data(), sh.num_perm_sets, pcols.data(), psig.data(), (uint32_t)pcols.size(),
                                                       sh.chunk_len, l0, l_last, l_blind, ek_, k, -(int32_t)(bf + 1), &beta, &gamma, &dom.delta, &zeta_, &w_, &y));
        }
        if (!lks.empty()) {
            std::vector<const void *> lz(lks.size()), la(lks.size()), ls(lks.size()), lap(lks.size()), lsp(lks.size());
            for (size_t li = 0; li < lks.size(); ++li) {
                const Lookup &l = sh.lookups[li];
                const LookupColumns &c = lks[li];
                lz[li] = c.z.coset + off;
                la[li] = (c.inp_coset ? c.inp_coset : adv[l.advice_col].coset) + off;
                ls[li] = (sh.dyn ? dyn_table_cos : fixed_cos(l.table_col)) + off;
                lap[li] = c.ap.coset + off;
                lsp[li] = c.sp.coset + off;
            }
            H2_CHK(h2hip_quotient_lookups_dev(ctx, acc_loc + off, lz.data(), la.data(), ls.data(), lap.data(), lsp.data(), lks.size(), l0, l_last, l_blind, ek_,
                                              k, &beta, &gamma, &y));
        }
        return h2hip_divide_by_vanishing_poly_dev(ctx, acc_loc + off, ek_, k, &w_, &zeta_);   // vanishing.construct: numerator / (X^n - 1)
    }
    // sharded quotient: every rank needs all of h's coefficients (its slices of the pieces are committed next, its evaluations opened later): one
    // go-ahead exchange (status only), then ONE all-gather of the cosets, device to device, and the interleave into extended-domain order
    int gather_quotient_cosets() {
        // Everything that can fail on this rank alone — the gathered buffer (256 MiB at k = 21), the transport's staging area — is done BEFORE
        // the go-ahead: a rank that fails here reports it through that exchange; after it only the collective itself is left
        Fr *gathered = nullptr;
        const size_t slot_elems = (size_t)pk->max_cosets * n;
        H2_CHK(sc.take(slot_elems * pk->shard_world, &gathered));
        H2_CHK(comm_reserve_allgather_dev(pk->comm, sizeof(Fr) * slot_elems));
        H2_CHK(link.go_ahead());
        // r04: extended_to_coeff by cosets as well.  The inverse transform of the whole extended domain factors into the size-n inverse coset
        // transform of every coset (iNTT, then s_c^-t: done HERE, where the coset's values are — 1 / 2^(ek-k) of the whole transform's work per
        // coset) and a 2^(ek-k)-point inverse DFT across the cosets for every t, which is pointwise: it runs on every rank after the all-gather
        // (h2hip_fr_coset_combine_dev) and leaves h(X)'s coefficients where extended_to_coeff would
        for (size_t m = 0; m < ncm; ++m) {
            const Fr s_c_inv = fe_inv(coset_shift(pk->my_cosets[m]));
            Fr *col = acc_loc + m * (size_t)n;
            H2_CHK(h2hip_ifft_dev(ctx, col, &dom.omega_inv, k, &dom.ifft_divisor));
            H2_CHK(h2hip_fr_coset_scale_batch_dev(ctx, (void *const *)&col, (const void *const *)&col, 1, n, &s_c_inv));
        }
        H2_CHK(h2hip_comm_allgather_dev(pk->comm, ctx, acc_loc, sizeof(Fr) * slot_elems, gathered));
        const uint32_t log_c = ek - k;
        uint32_t slots[16] = {0};
        for (uint32_t c = 0; c < (1u << log_c); ++c) slots[c] = (c % pk->shard_world) * pk->max_cosets + c / pk->shard_world;
        const Fr rho_inv = fe_inv(fe_pow_u64(dom.ext_omega, (uint64_t)n)), zeta_n_inv = fe_inv(fe_pow_u64(dom.zeta, (uint64_t)n));
        H2_CHK(h2hip_fr_coset_combine_dev(ctx, acc, gathered, slots, log_c, n, &rho_inv, &zeta_n_inv));
        sc.release(gathered);
        sc.release(acc_loc);
        return H2HIP_OK;
    }
    int quotient() {
        if (!qshard) {
            H2_CHK(quotient_pass(0, ek, dom.zeta, dom.ext_omega));
        } else {
            for (size_t m = 0; m < ncm; ++m) {
                const Fr s_c = coset_shift(pk->my_cosets[m]);
                H2_CHK(quotient_pass(m * (size_t)n, k, s_c, dom.omega));
            }
            H2_CHK(gather_quotient_cosets());
        }
        laps.lap(ST_QUOTIENT);
        for (Forms &f : perm_z) sc.release(f.coset);
        for (LookupColumns &c : lks) {
            sc.release(c.z.coset);
            sc.release(c.ap.coset);
            sc.release(c.sp.coset);
            if (c.inp_coset) sc.release(c.inp_coset);
        }
        if (dyn_table_cos) sc.release(dyn_table_cos);
        for (Forms &f : adv) sc.release(f.coset);
        for (Forms &f : inst) sc.release(f.coset);
        return H2HIP_OK;
    }

    // ---- 12. h(X) back to coefficients, split into pieces, committed
    int h_pieces() {
        if (!qshard) H2_CHK(h2hip_extended_to_coeff_dev(ctx, acc, ek, &dom.ext_omega_inv, &dom.ext_ifft_divisor, &dom.zeta_inv));   // (sharded: done by cosets above)
        laps.lap(ST_H_COEFF);
        stage.draw(sh.quotient_pieces);   // h_blinds
        std::vector<const void *> cols;
        for (uint32_t i = 0; i < sh.quotient_pieces; ++i) cols.push_back(acc + (size_t)i * n);
        H2_CHK(commit.batch(pk->g, cols, n));
        laps.lap(ST_COMMIT_H);
        return tr.squeeze_challenge(x);
    }

    // ---- 13. evaluations: every (polynomial, point) pair of the round goes through ONE batched launch; the transcript then takes the
    // values in upstream's order
    Fr rotate(int rot) const {
        int64_t r = ((int64_t)rot % (int64_t)n + (int64_t)n) % (int64_t)n;
        return fe_mul(x, fe_pow_u64(dom.omega, (uint64_t)r));
    }
    int evaluations() {
        const Fr xn = fe_pow_u64(x, n);
        std::map<const Fr *, int> poly_index;
        auto poly_id = [&](const Fr *p) -> int {
            auto it = poly_index.find(p);
            if (it != poly_index.end()) return it->second;
            polys.push_back(p);
            poly_index[p] = (int)polys.size() - 1;
            return (int)polys.size() - 1;
        };
        // vanishing.evaluate: h(X) = sum_i x^(n i) h_i(X) (its evaluation is not written to the proof; the multiopen needs it)
        Fr *h_poly = nullptr;
        H2_CHK(sc.take(n, &h_poly));
        {
            std::vector<const void *> pieces(sh.quotient_pieces);
            std::vector<Fr> xn_pows(sh.quotient_pieces);
            Fr xp = Fr::one();
            for (uint32_t i = 0; i < sh.quotient_pieces; ++i) {
                pieces[i] = acc + (size_t)i * n;
                xn_pows[i] = xp;
                xp = fe_mul(xp, xn);
            }
            H2_CHK(h2hip_fr_linear_combination_dev(ctx, h_poly, pieces.data(), xn_pows.data(), pieces.size(), n));
        }
        const Fr x_next = rotate(1), x_last = rotate(-(int)(bf + 1)), x_inv = rotate(-1);
        std::vector<Query> evq;            // in the order the values are written: advice, fixed, random, sigma, permutation sets, lookups; then h
        std::vector<const void *> ev_polys;
        auto want = [&](const Fr *poly, const Fr &point) -> size_t {
            evq.push_back(Query{-1, point, Fr::zero()});
            ev_polys.push_back(poly);
            return evq.size() - 1;
        };
        const size_t i_adv = evq.size();
        for (auto &aq : sh.advice_queries) want(adv[aq.first].coeff, rotate(aq.second));
        const size_t i_fixed = evq.size();
        for (auto &fq : sh.fixed_queries) want(pk->fixed_polys[fq.first], rotate(fq.second));
        const size_t i_random = want(random_poly, x);
        const size_t i_sigma = evq.size();
        for (Fr *sp_ : pk->sigma_polys) want(sp_, x);
        const size_t i_perm = evq.size();
        for (uint32_t si = 0; si < sh.num_perm_sets; ++si) {
            want(perm_z[si].coeff, x);
            want(perm_z[si].coeff, x_next);
            if (si + 1 != sh.num_perm_sets) want(perm_z[si].coeff, x_last);
        }
        const size_t i_lookup = evq.size();
        for (LookupColumns &s : lks) {   // product_eval, product_next_eval, permuted_input_eval, permuted_input_inv_eval, permuted_table_eval
            want(s.z.coeff, x);
            want(s.z.coeff, x_next);
            want(s.ap.coeff, x);
            want(s.ap.coeff, x_inv);
            want(s.sp.coeff, x);
        }
        const size_t n_written = evq.size();
        const size_t i_h = want(h_poly, x);
        {
            std::vector<Fr> points(evq.size()), vals(evq.size());
            for (size_t i = 0; i < evq.size(); ++i) points[i] = evq[i].point;
            if (!sharded_any) {
                std::vector<size_t> lens(evq.size(), n);
                H2_CHK(h2hip_fr_eval_polynomial_batch_dev(ctx, ev_polys.data(), lens.data(), points.data(), evq.size(), vals.data()));
            } else {
                // sharded (r04): every polynomial is evaluated over this rank's COEFFICIENT range [lo, hi) — the range of its SRS slice —
                // p(x) = sum_ranks x^lo * sum_j c[lo + j] x^j: the same batched launch on 1/N of the coefficients, one exchange of 32 bytes per
                // query, N-term sums on the host.  Every rank ends up with every evaluation (the transcripts stay in lock step).
                H2_REQUIRE(evq.size() == (size_t)sh.num_evals() + 1, "internal: evaluation count differs from the exchange schedule");
                const size_t lo = link.lo(n), hi = link.hi(n);
                std::vector<const void *> part(evq.size());
                std::vector<size_t> lens(evq.size(), hi - lo);
                for (size_t i = 0; i < evq.size(); ++i) part[i] = (const Fr *)ev_polys[i] + lo;
                if (hi > lo) H2_CHK(h2hip_fr_eval_polynomial_batch_dev(ctx, part.data(), lens.data(), points.data(), evq.size(), vals.data()));
                for (size_t i = 0; i < evq.size(); ++i) vals[i] = hi > lo ? fe_mul(vals[i], fe_pow_u64(points[i], lo)) : Fr::zero();
                std::vector<uint8_t> all;
                H2_CHK(link.exchange(vals.data(), sizeof(Fr) * vals.size(), all));
                const size_t slot = 8 + sizeof(Fr) * vals.size();
                for (size_t i = 0; i < vals.size(); ++i) {
                    Fr sum = Fr::zero();
                    for (uint32_t r = 0; r < pk->shard_world; ++r) {
                        Fr v;
                        memcpy(&v, all.data() + (size_t)r * slot + 8 + sizeof(Fr) * i, sizeof(Fr));
                        sum = fe_add(sum, v);
                    }
                    vals[i] = sum;
                }
            }
            for (size_t i = 0; i < evq.size(); ++i) evq[i].eval = vals[i];
        }
        for (size_t i = 0; i < n_written; ++i) H2_CHK(tr.write_scalar(evq[i].eval));
        // the multiopen's query list in upstream's order: advice, permutation (sets at x / x_next, then sets.rev().skip(1) at x_last), lookups
        // (product, permuted input, permuted table at x; permuted input at x_inv; product at x_next), fixed, permutation polynomials, h, random
        auto ask = [&](size_t i) {
            Query q = evq[i];
            q.poly = poly_id((const Fr *)ev_polys[i]);
            queries.push_back(q);
        };
        for (size_t i = i_adv; i < i_fixed; ++i) ask(i);
        {
            std::vector<size_t> tail;
            size_t i = i_perm;
            for (uint32_t si = 0; si < sh.num_perm_sets; ++si) {
                ask(i);
                ask(i + 1);
                i += 2;
                if (si + 1 != sh.num_perm_sets) tail.push_back(i++);
            }
            for (size_t t = tail.size(); t-- > 0;) ask(tail[t]);
        }
        for (size_t li = 0; li < lks.size(); ++li) {
            const size_t i = i_lookup + 5 * li;
            ask(i);       // product at x
            ask(i + 2);   // permuted input at x
            ask(i + 4);   // permuted table at x
            ask(i + 3);   // permuted input at x_inv
            ask(i + 1);   // product at x_next
        }
        for (size_t i = i_fixed; i < i_random; ++i) ask(i);
        for (size_t i = i_sigma; i < i_perm; ++i) ask(i);
        ask(i_h);
        ask(i_random);
        laps.lap(ST_EVALS);
        return H2HIP_OK;
    }

    // ---- 14. ProverSHPLONK::create_proof [UPSTREAM-RECALL poly/kzg/multiopen/shplonk/prover.rs]
    // Sharded (r04): every step between the evaluations and the two commitments is pointwise in the coefficient index — S_i = sum_j y^j P_ij,
    // the v-weighted sum of the sets' quotients, the linearisation — except the divisions by (X - root), whose suffix Horner needs ONE value per
    // (range boundary, root): what the coefficients above the range evaluate to.  With the commitments sharded by point range = coefficient
    // range a rank only ever needs ITS range [lo, hi) of these polynomials: it forms S_i on its range, the ranks exchange the ranges' partial
    // evaluations at the roots (32 bytes per (set, root) pair), and each divides its range with the carry assembled from the ranges above
    // (h2hip_fr_kate_division_range_dev).  The same for the final division of the linearisation by (X - u).
    int shplonk() {
        Fr yq, v, uq;
        H2_CHK(tr.squeeze_challenge(yq));
        std::vector<RotationSet> sets;
        std::vector<Fr> super_points;
        construct_intermediate_sets(queries, sets, super_points);
        H2_REQUIRE(!sets.empty(), "more than 64 distinct opening points");
        H2_CHK(tr.squeeze_challenge(v));
        const size_t lo = link.lo(n), hi = link.hi(n);
        const size_t L = hi - lo;   // coefficients held here (everything on one GPU)
        // S_i(X) = sum_j y^j P_ij(X) (kept for the linearisation), r_i(X) = sum_j y^j * interpolant of P_ij on the set's points
        std::vector<Fr *> S(sets.size());
        std::vector<std::vector<Fr>> low(sets.size()), pf_weights(sets.size());
        Fr *buf_a = nullptr, *buf_b = nullptr, *h_x = nullptr;
        H2_CHK(sc.take(n, &buf_a));
        H2_CHK(sc.take(n, &buf_b));
        H2_CHK(sc.take(n, &h_x));
        H2_HIPCHK(hipMemsetAsync(h_x, 0, sizeof(Fr) * n, st));
        size_t n_open = 0;
        for (size_t i = 0; i < sets.size(); ++i) {
            const RotationSet &rs = sets[i];
            H2_REQUIRE(rs.points.size() <= 8, "more than 8 rotations in one opening set");
            n_open += rs.points.size();
            H2_CHK(sc.take(n, &S[i]));
            low[i].assign(rs.points.size(), Fr::zero());
            Fr ypow = Fr::one();
            const std::vector<std::vector<Fr>> basis = lagrange_basis(rs.points, pf_weights[i]);
            std::vector<const void *> terms(rs.polys.size());
            std::vector<Fr> ypows(rs.polys.size());
            for (size_t j = 0; j < rs.polys.size(); ++j) {
                terms[j] = polys[rs.polys[j]] + lo;
                ypows[j] = ypow;
                std::vector<Fr> r = lagrange_interpolate(basis, rs.evals[j]);
                for (size_t t = 0; t < r.size(); ++t) low[i][t] = fe_add(low[i][t], fe_mul(ypow, r[t]));
                ypow = fe_mul(ypow, yq);
            }
            if (L) H2_CHK(h2hip_fr_linear_combination_dev(ctx, S[i] + lo, terms.data(), ypows.data(), terms.size(), L));   // every P_j read once
        }
        std::vector<std::vector<Fr>> carries(sets.size());
        if (sharded_any) {
            H2_REQUIRE(n_open <= SHPLONK_MAX_OPENINGS, "sharded create_proof: more (rotation set, point) pairs than the exchange holds");
            std::vector<const void *> part;
            std::vector<size_t> lens;
            std::vector<Fr> at, vals(SHPLONK_MAX_OPENINGS, Fr::zero());
            for (size_t i = 0; i < sets.size(); ++i)
                for (const Fr &pt : sets[i].points) {
                    part.push_back(S[i] + lo);
                    lens.push_back(L);
                    at.push_back(pt);
                }
            if (L) H2_CHK(h2hip_fr_eval_polynomial_batch_dev(ctx, part.data(), lens.data(), at.data(), part.size(), vals.data()));
            std::vector<uint8_t> all;
            H2_CHK(link.exchange(vals.data(), sizeof(Fr) * SHPLONK_MAX_OPENINGS, all));
            size_t idx = 0;
            for (size_t i = 0; i < sets.size(); ++i)
                for (const Fr &pt : sets[i].points) carries[i].push_back(link.carry_from(all, 8 + sizeof(Fr) * SHPLONK_MAX_OPENINGS, idx++, pt, hi));
        }
        Fr vpow = Fr::one();
        // (S_i - r_i) / prod_j (X - point_j) = sum_j w_j (S_i(X) - S_i(point_j)) / (X - point_j) (partial fractions; r_i interpolates S_i
        // on the points by construction): all roots in ONE pass over S_i, no copy and no explicit subtraction of r_i; v^i folded into the
        // weights, the sets' quotients add up in h_x — single GPU: ALL sets in one call (one job table, one carry launch)
        if (!sharded_any) {
            std::vector<const void *> polys_s(sets.size());
            std::vector<Fr> pts, wts;
            std::vector<uint32_t> sizes(sets.size());
            for (size_t i = 0; i < sets.size(); ++i) {
                polys_s[i] = S[i];
                sizes[i] = (uint32_t)sets[i].points.size();
                for (size_t j = 0; j < sets[i].points.size(); ++j) {
                    pts.push_back(sets[i].points[j]);
                    wts.push_back(fe_mul(pf_weights[i][j], vpow));
                }
                vpow = fe_mul(vpow, v);
            }
            H2_CHK(h2hip_fr_kate_division_sets_dev(ctx, h_x, polys_s.data(), n, pts.data(), wts.data(), sizes.data(), sets.size(), 1));   // (h_x starts as zeros)
        } else {
            for (size_t i = 0; i < sets.size(); ++i) {
                const RotationSet &rs = sets[i];
                if (L) {
                    H2_CHK(h2hip_fr_kate_division_range_dev(ctx, buf_b + lo, S[i] + lo, L, rs.points.data(), pf_weights[i].data(), carries[i].data(),
                                                            (uint32_t)rs.points.size()));
                    H2_CHK(h2hip_fr_axpy_dev(ctx, h_x + lo, &vpow, buf_b + lo, L));
                }
                vpow = fe_mul(vpow, v);
            }
        }
        H2_CHK(commit.batch(pk->g, std::vector<const void *>(1, h_x), n));
        H2_CHK(tr.squeeze_challenge(uq));
        // linearisation L(X) = sum_i v^i Z_{T\S_i}(u) (S_i(X) - r_i(u)) - Z_T(u) h(X), which vanishes at u
        Fr *l_x = buf_a;
        Fr const0 = Fr::zero(), z_diff_0 = Fr::one();
        vpow = Fr::one();
        std::vector<const void *> lin_terms;
        std::vector<Fr> lin_coeffs;
        for (size_t i = 0; i < sets.size(); ++i) {
            Fr z_i = Fr::one();
            for (const Fr &p : super_points) {
                bool in_set = false;
                for (const Fr &sp : sets[i].points) in_set |= fr_cmp(sp, p) == 0;
                if (!in_set) z_i = fe_mul(z_i, fe_sub(uq, p));
            }
            if (i == 0) z_diff_0 = z_i;
            const Fr c_i = fe_mul(vpow, z_i);
            lin_terms.push_back(S[i] + lo);
            lin_coeffs.push_back(c_i);
            const0 = fe_add(const0, fe_mul(c_i, eval_small(low[i], uq)));
            vpow = fe_mul(vpow, v);
        }
        Fr zt = Fr::one();
        for (const Fr &p : super_points) zt = fe_mul(zt, fe_sub(uq, p));
        lin_terms.push_back(h_x + lo);
        lin_coeffs.push_back(fe_neg(zt));
        if (L) H2_CHK(h2hip_fr_linear_combination_dev(ctx, l_x + lo, lin_terms.data(), lin_coeffs.data(), lin_terms.size(), L));
        if (L && lo == 0) H2_CHK(h2hip_fr_sub_low_dev(ctx, l_x, &const0, 1));
        const Fr inv0 = fe_inv(z_diff_0);
        if (!sharded_any) {
            H2_CHK(h2hip_fr_kate_division_dev(ctx, buf_b, l_x, n, &uq));
            H2_CHK(h2hip_fr_scale_dev(ctx, buf_b, &inv0, (size_t)n - 1));
        } else {
            Fr e = Fr::zero();
            const void *part = l_x + lo;
            if (L) H2_CHK(h2hip_fr_eval_polynomial_batch_dev(ctx, &part, &L, &uq, 1, &e));
            std::vector<uint8_t> all;
            H2_CHK(link.exchange(&e, sizeof(Fr), all));
            const Fr carry = link.carry_from(all, 8 + sizeof(Fr), 0, uq, hi), one = Fr::one();
            if (L) {
                H2_CHK(h2hip_fr_kate_division_range_dev(ctx, buf_b + lo, l_x + lo, L, &uq, &one, &carry, 1));
                H2_CHK(h2hip_fr_scale_dev(ctx, buf_b + lo, &inv0, L));
            }
        }
        H2_CHK(commit.batch(pk->g, std::vector<const void *>(1, buf_b), (size_t)n - 1));
        laps.lap(ST_MULTIOPEN);
        return H2HIP_OK;
    }
};

int create_proof_impl(h2hip_ctx *ctx, h2hip_plonk_pk *pk, const void *const *advice, bool advice_on_device, const void *const *instances,
                      const size_t *instance_lens, h2hip_rng_fill_fn rng, void *rng_user, ProverTranscript &tr, double *stage_ms,
                      const h2hip_phase_witness *witness) {
    ProofRun run(ctx, pk, advice, advice_on_device, instances, instance_lens, rng, rng_user, tr, stage_ms, witness);
    H2_CHK(run.set_up());
    H2_CHK(run.instance_columns());
    H2_CHK(run.advice_columns());
    H2_CHK(run.shard_hello());
    H2_CHK(run.round1());
    H2_CHK(run.grand_products());
    H2_CHK(run.first_round_transforms());
    H2_CHK(run.commit_products_and_random());
    H2_CHK(run.join_and_extend_products());
    H2_CHK(run.quotient());
    H2_CHK(run.h_pieces());
    H2_CHK(run.evaluations());
    return run.shplonk();
}

}  // namespace plonk
}  // namespace h2

extern "C" const char *h2hip_plonk_stage_name(int stage) { return stage >= 0 && stage < H2HIP_PLONK_STAGES ? h2::plonk::STAGE_NAMES[stage] : ""; }
