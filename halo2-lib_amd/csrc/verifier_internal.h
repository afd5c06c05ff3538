// The verifier's two halves (verifier.hip), shared with the batch verifier (verify_batch.hip):
//   derive  replays ONE proof's transcript and returns what the final check needs — W' = h2, the (commitment, scalar) pairs whose sum is the
//           right-hand point `outer`, and the scalar on g[0] — or rejects the proof;
//   finish  turns that into a verdict: the scalar multiplications (on the host for one proof, one device MSM for a batch) and ONE pairing
//           e(W', s_g2) * e(-outer, g2) == 1.
// Both read the constraint system from the prover's plonk::Shape (plonk_shape.h); every h2hip_plonk_verify_proof* entry, the transcript
// entry and the batch entry build it with plonk::shape_of_kind from their params.
#pragma once
#include <utility>
#include <vector>

#include "host_field.h"
#include "internal.h"
#include "plonk_shape.h"
#include "transcript.h"

namespace h2 {
namespace verifier {

// the verifying key and the SRS elements, as the entry points receive them
struct VKey {
    const void *fixed_commitments, *permutation_commitments, *transcript_repr, *g1, *g2, *s_g2;
};
// A proof is a table of 32-byte words; which of them are points follows from the shape: every commitment up to the h pieces, then the
// evaluations, then h1 and h2 (which Shape::num_commitments counts as its last two).  Returns the number of words of a well-formed proof;
// point_words (optional): the point words in reading order.
size_t proof_words(const plonk::Shape &sh, std::vector<uint32_t> *point_words);
// a proof's points already decompressed, in reading order, each with its verdict (h2hip_g1_decompress_checked_dev: 0 ok)
struct DecodedPoints {
    const G1Affine *pts;
    const uint32_t *status;
    size_t n;
};
struct Term {
    int vk_slot;   // -1: a point of this proof; c: fixed commitment c; num_fixed_total + j: sigma commitment j
    G1Affine p;
    Fr s;
};
struct Derived {
    G1Affine w;                // W' = h2
    std::vector<Term> terms;   // outer = sum s * p + g0_scalar * g[0]
    Fr g0_scalar;
};
// argument checks common to every entry (H2HIP_ERR_INVALID): NULL key parts the shape needs, g2 / s_g2 on the twist
int check_key(const plonk::Shape &sh, const VKey &vk, const void *const *instances_host, const size_t *instance_lens);
// pre == nullptr: every point is decompressed on the host (a square root each).  *well_formed = 0 is a rejection: malformed bytes, a
// non-canonical scalar, a bad point, an instance column longer than usable_rows, x on the domain, a zero z_diff.
int derive(const plonk::Shape &sh, const VKey &vk, const void *const *instances_host, const size_t *instance_lens, const uint8_t *proof, size_t proof_len,
           const DecodedPoints *pre, Derived *out, int *well_formed);
// the same over any reader (transcript.h): the built-in Blake2b reader above, or the adapter over the caller's callbacks.  A reader whose
// err is set makes derive return it.
int derive(const plonk::Shape &sh, const VKey &vk, const void *const *instances_host, const size_t *instance_lens, TranscriptReader &tr, Derived *out,
           int *well_formed);
G1Affine outer_on_host(const VKey &vk, const Derived &d);                                 // the terms' sum by host double-and-add
int pairing_verdict(const VKey &vk, const G1Affine &left, const G1Affine &outer, int *accepted);   // e(left, s_g2) * e(-outer, g2) == 1
// derive + finish for one proof: the argument checks that need the shape, then what h2hip_plonk_verify_proof* compute
int verify_one(const plonk::Shape &sh, const VKey &vk, const void *const *instances_host, const size_t *instance_lens, const uint8_t *proof, size_t proof_len,
               int *accepted);
template <class P>
inline bool canonical(const Fe<P> &a) {
    unsigned br = 0;
    for (int j = 0; j < 8; ++j) subb32(a.l[j], P::m(j), br);
    return br != 0;
}

}  // namespace verifier
}  // namespace h2
