// The transcript as the prover and the verifier see it: two small interfaces, each with the built-in Blake2b implementation
// (Blake2bWrite / Blake2bRead + Challenge255, what the byte-returning entries serve) and a thin adapter over the caller's h2hip_transcript
// callbacks (include/h2hip.h).  The prover's side is here; the reader's interface and its adapter too, the Blake2b reader (which also takes
// points the batch verifier decompressed on the device) stays in verifier.hip.
#pragma once
#include <vector>

#include "blake2b.h"
#include "host_field.h"
#include "internal.h"

namespace h2 {

static const unsigned SIGN_BIT = 6, INF_BIT = 7;   // compressed G1: sign(y) and identity flags in the top byte (halo2curves new_curve_impl!; the
                                                   // positions are UNVERIFIED for halo2curves-axiom 0.7.3, see oracle/transcript.py)

template <class P>
inline bool fe_canonical(const Fe<P> &a) {   // limbs < the modulus
    unsigned br = 0;
    for (int j = 0; j < 8; ++j) subb32(a.l[j], P::m(j), br);
    return br != 0;
}

// ---------------------------------------------------------------------------------------------- prover
// what create_proof asks of a transcript; every call returns H2HIP_OK or ends the proof
struct ProverTranscript {
    virtual ~ProverTranscript() {}
    virtual int common_scalar(const Fr &s) = 0;
    virtual int write_scalar(const Fr &s) = 0;
    virtual int write_point(const G1Affine &p) = 0;
    virtual int squeeze_challenge(Fr &out) = 0;
    // upstream: io::Error "cannot write points at infinity to the transcript" — checked by the library for every implementation
    static int refuse_identity(const G1Affine &p) {
        if (p.x.is_zero() && p.y.is_zero()) {
            set_error("create_proof: a commitment is the point at infinity and cannot be written to the transcript");
            return H2HIP_ERR_INVALID;
        }
        return H2HIP_OK;
    }
};

struct Transcript final : ProverTranscript {   // Blake2bWrite<Vec<u8>, G1Affine, Challenge255<_>>  
    Blake2b st;
    std::vector<uint8_t> proof;
    Transcript() : st(64, "Halo2-Transcript") {}
    int common_scalar(const Fr &s) override {
        uint8_t b[33];
        b[0] = 0x02;
        fr_repr(s, b + 1);
        st.update(b, 33);
        return H2HIP_OK;
    }
    int write_scalar(const Fr &s) override {
        common_scalar(s);
        uint8_t b[32];
        fr_repr(s, b);
        proof.insert(proof.end(), b, b + 32);
        return H2HIP_OK;
    }
    int write_point(const G1Affine &p) override {
        H2_CHK(refuse_identity(p));
        uint8_t b[65];
        b[0] = 0x01;
        fq_repr(p.x, b + 1);
        fq_repr(p.y, b + 33);
        st.update(b, 65);
        uint8_t c[32];
        memcpy(c, b + 1, 32);
        c[31] |= (uint8_t)((b[33] & 1) << SIGN_BIT);
        proof.insert(proof.end(), c, c + 32);
        return H2HIP_OK;
    }
    int squeeze_challenge(Fr &out) override {
        uint8_t z = 0x00, d[64];
        st.update(&z, 1);
        st.digest(d);
        out = fr_from_uniform_bytes(d);
        return H2HIP_OK;
    }
};

// the caller's transcript behind the prover's interface: counts the calls of every operation, so that a failure can be named
struct CallbackTranscript final : ProverTranscript {
    const h2hip_transcript *t;
    unsigned n_common = 0, n_scalar = 0, n_point = 0, n_squeeze = 0;
    explicit CallbackTranscript(const h2hip_transcript *t_) : t(t_) {}
    static int failed(const char *op, unsigned ordinal, int rc) {
        set_error("create_proof: the transcript's %s #%u returned %d", op, ordinal, rc);
        return H2HIP_ERR_INVALID;
    }
    int common_scalar(const Fr &s) override {
        const int rc = t->common_scalar(t->user, &s);
        return ++n_common, rc ? failed("common_scalar", n_common, rc) : H2HIP_OK;
    }
    int write_scalar(const Fr &s) override {
        const int rc = t->write_scalar(t->user, &s);
        return ++n_scalar, rc ? failed("write_scalar", n_scalar, rc) : H2HIP_OK;
    }
    int write_point(const G1Affine &p) override {
        H2_CHK(refuse_identity(p));
        const int rc = t->write_point(t->user, &p);
        return ++n_point, rc ? failed("write_point", n_point, rc) : H2HIP_OK;
    }
    int squeeze_challenge(Fr &out) override {
        out = Fr::zero();
        const int rc = t->squeeze_challenge(t->user, &out);
        ++n_squeeze;
        if (rc) return failed("squeeze_challenge", n_squeeze, rc);
        if (!fe_canonical(out)) {
            set_error("create_proof: the transcript's squeeze_challenge #%u returned a value that is not a canonical Fr", n_squeeze);
            return H2HIP_ERR_INVALID;
        }
        return H2HIP_OK;
    }
};

// ---------------------------------------------------------------------------------------------- verifier
// What verify_proof asks of a transcript.  A value that cannot be read makes the proof malformed (ok = false: a rejection); a transcript that
// fails where no proof byte is involved is an error (err != H2HIP_OK).  After either, every call returns zeros without touching the source.
struct TranscriptReader {
    bool ok = true;
    int err = H2HIP_OK;
    virtual ~TranscriptReader() {}
    virtual void common_scalar(const Fr &s) = 0;
    virtual Fr read_scalar() = 0;
    virtual G1Affine read_point() = 0;
    virtual Fr squeeze_challenge() = 0;
    virtual bool exhausted() const = 0;   // no input is left over (a reader that cannot tell says true)
};

struct CallbackReader final : TranscriptReader {
    const h2hip_transcript *t;
    explicit CallbackReader(const h2hip_transcript *t_) : t(t_) {}
    bool live() const { return ok && err == H2HIP_OK; }
    void broken(const char *op, int rc) {
        set_error("verify_proof: the transcript's %s returned %d", op, rc);
        err = H2HIP_ERR_INVALID;
    }
    void common_scalar(const Fr &s) override {
        if (!live()) return;
        const int rc = t->common_scalar(t->user, &s);
        if (rc) broken("common_scalar", rc);
    }
    Fr read_scalar() override {
        Fr s = Fr::zero();
        if (!live()) return s;
        if (t->read_scalar(t->user, &s) != 0 || !fe_canonical(s)) {
            ok = false;
            return Fr::zero();
        }
        return s;
    }
    G1Affine read_point() override {
        G1Affine z, p;
        z.x = z.y = p.x = p.y = Fq::zero();
        if (!live()) return z;
        if (t->read_point(t->user, &p) != 0 || !fe_canonical(p.x) || !fe_canonical(p.y) || (p.x.is_zero() && p.y.is_zero())) {
            ok = false;
            return z;
        }
        Fq three = Fq::zero();
        three.l[0] = 3;
        if (!(fe_sqr(p.y) == fe_add(fe_mul(fe_sqr(p.x), p.x), fe_to_mont(three)))) {   // y^2 == x^3 + 3
            ok = false;
            return z;
        }
        return p;
    }
    Fr squeeze_challenge() override {
        Fr c = Fr::zero();
        if (!live()) return c;
        const int rc = t->squeeze_challenge(t->user, &c);
        if (rc) {
            broken("squeeze_challenge", rc);
            return Fr::zero();
        }
        if (!fe_canonical(c)) {
            set_error("verify_proof: the transcript's squeeze_challenge returned a value that is not a canonical Fr");
            err = H2HIP_ERR_INVALID;
            return Fr::zero();
        }
        return c;
    }
    bool exhausted() const override { return true; }
};

}  // namespace h2
