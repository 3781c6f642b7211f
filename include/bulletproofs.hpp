// bulletproofs.hpp -- host-side mirror (C++17, header-only) of the reference crate's public
// verification surface, implemented over the C ABI of libbpgpu.so (include/bpgpu.h).
//
// Mirrors, with the same names, argument meaning and error behaviour:
//   ProofError ............ src/errors.rs:12-54
//   PedersenGens .......... src/generators.rs:30-53        (default() = basepoint + hashed blinding base)
//   BulletproofGens ....... src/generators.rs:157-204      (new(gens_capacity, party_capacity))
//   Transcript ............ merlin::Transcript: new / append_message / append_u64 / challenge_bytes, held as its
//                           208-byte STROBE state; verifiers take it by reference and leave it advanced
//   RangeProof ............ src/range_proof/mod.rs:59-76, from_bytes 504-538, to_bytes 487-500,
//                           verify_single[_with_rng] 316-342, verify_multiple[_with_rng] 345-470,
//                           prove_single/multiple_with_rng 115-288 (variable time on the GPU)
//   LinearProof ........... src/linear_proof.rs: create 40-173 (variable time on the GPU), from_bytes 350-394,
//                           to_bytes 322-331, verify 175-236
// plus verify_batch, the batched entry point this engine exists for.  No arithmetic happens on the
// host: parsing checks lengths and scalar canonicity (so from_bytes fails where the reference's does)
// and everything else is one call into the GPU library.  There is no CPU fallback.
#ifndef BULLETPROOFS_HPP
#define BULLETPROOFS_HPP
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <variant>
#include <vector>

#include "bpgpu.h"

namespace bulletproofs {

enum class ProofError {
    VerificationError = BPGPU_VERDICT_VERIFICATION_ERROR,
    FormatError = BPGPU_VERDICT_FORMAT_ERROR,
    InvalidBitsize = BPGPU_VERDICT_INVALID_BITSIZE,
    InvalidGeneratorsLength = BPGPU_VERDICT_INVALID_GENERATORS_LENGTH,
};

// Result<(), ProofError>
struct Status {
    bool ok_;
    ProofError err_;
    static Status Ok() { return {true, ProofError::VerificationError}; }
    static Status Err(ProofError e) { return {false, e}; }
    bool is_ok() const { return ok_; }
    ProofError unwrap_err() const {
        if (ok_) throw std::logic_error("unwrap_err on Ok");
        return err_;
    }
    bool operator==(const Status &o) const { return ok_ == o.ok_ && (ok_ || err_ == o.err_); }
};

using CompressedRistretto = std::array<uint8_t, 32>;
using ScalarBytes = std::array<uint8_t, 32>;

class GpuError : public std::runtime_error {
  public:
    using std::runtime_error::runtime_error;
};

class PedersenGens {
  public:
    CompressedRistretto B{}, B_blinding{};
    bool operator==(const PedersenGens &o) const { return B == o.B && B_blinding == o.B_blinding; }
};

class Transcript;
class OpeningProof;

class BulletproofGens {
  public:
    size_t gens_capacity, party_capacity;
    // BulletproofGens::new(gens_capacity, party_capacity): generators are derived on `device`
    BulletproofGens(size_t gens_capacity_, size_t party_capacity_, int device = 0)
        : gens_capacity(gens_capacity_), party_capacity(party_capacity_) {
        bpgpu_ctx *c = nullptr;
        if (bpgpu_ctx_create(device, &c) != BPGPU_OK) throw GpuError("bpgpu_ctx_create failed: no usable GPU (there is no CPU fallback)");
        ctx_.reset(c, bpgpu_ctx_destroy);
        if (bpgpu_gens_create(c, gens_capacity, party_capacity) != BPGPU_OK) throw GpuError(bpgpu_last_error(c));
    }
    bpgpu_ctx *ctx() const { return ctx_.get(); }
    // PedersenGens::default() as held by this verifier
    PedersenGens pedersen() const {
        PedersenGens pc;
        if (bpgpu_gens_export(ctx_.get(), nullptr, nullptr, pc.B.data(), pc.B_blinding.data()) != BPGPU_OK) throw GpuError(bpgpu_last_error(ctx_.get()));
        return pc;
    }
    // PedersenGens::commit(value, blinding) (generators.rs:38-42) with this context's bases, compressed (variable time on the GPU)
    CompressedRistretto commit(const ScalarBytes &value, const ScalarBytes &blinding) const {
        const PedersenGens pc = pedersen();
        uint8_t sc[64], pt[64], status = 0;
        std::memcpy(sc, value.data(), 32);
        std::memcpy(sc + 32, blinding.data(), 32);
        std::memcpy(pt, pc.B.data(), 32);
        std::memcpy(pt + 32, pc.B_blinding.data(), 32);
        const uint32_t nt = 2;
        CompressedRistretto out{};
        if (bpgpu_msm_batch(ctx_.get(), 1, &nt, sc, pt, out.data(), &status) != BPGPU_OK) throw GpuError(bpgpu_last_error(ctx_.get()));
        if (status != 0) throw std::invalid_argument("commit: scalars must be canonical");
        return out;
    }
    // values.size() calls of commit in ONE GPU launch (bpgpu_pedersen_commit_batch; no counterpart in the crate) -> (commitments, blindings).
    // blindings == nullptr: blinding i is the (first_draw + i)-th Scalar::random of ChaChaRng::from_seed(rng_seed32), drawn on the
    // device (rng_seed32 == nullptr: the library draws the seed).  Row i equals commit(values[i], blindings[i]).
    std::pair<std::vector<CompressedRistretto>, std::vector<ScalarBytes>> commit_batch(const std::vector<uint64_t> &values, const std::vector<ScalarBytes> *blindings,
                                                                                      const uint8_t *rng_seed32 = nullptr, uint64_t first_draw = 0) const {
        return commit_rows(values.data(), 8, values.size(), blindings, rng_seed32, first_draw);
    }
    std::pair<std::vector<CompressedRistretto>, std::vector<ScalarBytes>> commit_batch(const std::vector<ScalarBytes> &values, const std::vector<ScalarBytes> *blindings,
                                                                                      const uint8_t *rng_seed32 = nullptr, uint64_t first_draw = 0) const {
        return commit_rows(values.data(), 32, values.size(), blindings, rng_seed32, first_draw);
    }
    // does (values[i], blindings[i]) open commitments[i]? (bpgpu_pedersen_open_batch)  VerificationError: it does not, or the
    // commitment is no valid encoding; FormatError: a non-canonical scalar
    std::vector<Status> verify_openings(const std::vector<CompressedRistretto> &commitments, const std::vector<uint64_t> &values,
                                        const std::vector<ScalarBytes> &blindings) const {
        return open_rows(commitments, values.data(), 8, values.size(), blindings);
    }
    std::vector<Status> verify_openings(const std::vector<CompressedRistretto> &commitments, const std::vector<ScalarBytes> &values,
                                        const std::vector<ScalarBytes> &blindings) const {
        return open_rows(commitments, values.data(), 32, values.size(), blindings);
    }
    // Row r: sum(plus[r]) - sum(minus[r]) + values[r] B + blindings[r] B_blinding, compressed (bpgpu_pedersen_sum_batch; no counterpart
    // in the crate).  minus, values, blindings may be nullptr (no subtracted terms / zero).  An entry is empty where a term of the row
    // did not decode; a non-canonical scalar throws std::invalid_argument.
    using Rows = std::vector<std::vector<CompressedRistretto>>;
    std::vector<std::optional<CompressedRistretto>> sum_commitments(const Rows &plus, const Rows *minus = nullptr, const std::vector<uint64_t> *values = nullptr,
                                                                    const std::vector<ScalarBytes> *blindings = nullptr) const {
        return sum_rows(plus, minus, values ? values->data() : nullptr, 8, values ? values->size() : plus.size(), blindings);
    }
    std::vector<std::optional<CompressedRistretto>> sum_commitments(const Rows &plus, const Rows *minus, const std::vector<ScalarBytes> &values,
                                                                    const std::vector<ScalarBytes> *blindings = nullptr) const {
        return sum_rows(plus, minus, values.data(), 32, values.size(), blindings);
    }
    // does sum(inputs[r]) - sum(outputs[r]) open to (values[r], blindings[r])? (bpgpu_pedersen_balance_batch)  VerificationError: it
    // does not, or a commitment is no valid encoding; FormatError: a non-canonical scalar.  A missing value or blinding is zero.
    std::vector<Status> verify_balance(const Rows &inputs, const Rows &outputs, const std::vector<uint64_t> *values = nullptr,
                                       const std::vector<ScalarBytes> *blindings = nullptr) const {
        return balance_rows(inputs, outputs, values ? values->data() : nullptr, 8, values ? values->size() : inputs.size(), blindings);
    }
    std::vector<Status> verify_balance(const Rows &inputs, const Rows &outputs, const std::vector<ScalarBytes> &values,
                                       const std::vector<ScalarBytes> *blindings = nullptr) const {
        return balance_rows(inputs, outputs, values.data(), 32, values.size(), blindings);
    }
    // The excess proofs of a block of confidential transactions (defined behind OpeningProof below): row r proves knowledge of the
    // blinding of E_r = sum(inputs[r]) - sum(outputs[r]) - fees[r] B -- an OpeningProof with the public value 0 under the key E_r -- and
    // verify_balance_proved checks rows of them without any secret: E_r through sum_commitments (value l - fee), then ONE combined
    // check.  (The Python twin keeps E_r on the device between the two calls; this header has no device allocator and uses the host forms.)
    inline std::vector<OpeningProof> prove_balance(const std::vector<uint64_t> &fees, const std::vector<ScalarBytes> &excess_blindings,
                                                   std::vector<Transcript> &transcripts, const Rows &inputs, const Rows &outputs,
                                                   const uint8_t *rng_seed32 = nullptr) const;
    inline std::vector<Status> verify_balance_proved(const Rows &inputs, const Rows &outputs, const std::vector<uint64_t> &fees,
                                                     const std::vector<OpeningProof> &proofs, std::vector<Transcript> &transcripts) const;
    // BulletproofGens::increase_capacity (generators.rs:177-204): no-op unless larger; the device tables are rebuilt
    void increase_capacity(size_t new_capacity) {
        if (gens_capacity >= new_capacity) return;
        if (bpgpu_gens_create(ctx_.get(), new_capacity, party_capacity) != BPGPU_OK) throw GpuError(bpgpu_last_error(ctx_.get()));
        gens_capacity = new_capacity;
    }
    // the aggregated iterators G(n, m) / H(n, m) (generators.rs:207-259): the first n generators of each of the first m parties
    std::vector<CompressedRistretto> G(size_t n, size_t m) const { return slice(true, n, m, 0); }
    std::vector<CompressedRistretto> H(size_t n, size_t m) const { return slice(false, n, m, 0); }
    // share(j).G(n) / share(j).H(n) (generators.rs:168-175, 262-292)
    std::vector<CompressedRistretto> share_G(size_t j, size_t n) const { return slice(true, n, 1, j); }
    std::vector<CompressedRistretto> share_H(size_t j, size_t n) const { return slice(false, n, 1, j); }

    // The verifier multiplies by pc_gens.B / B_blinding (mod.rs:439-440); the device tables hold the bases of this
    // BulletproofGens.  Any other PedersenGens would silently verify a different statement: refuse it.
    void check_pedersen(const PedersenGens &pc) const {
        if (!(pc == pedersen())) throw std::invalid_argument("pc_gens differs from the Pedersen bases in the device tables (load custom bases with bpgpu_gens_load)");
    }

  private:
    std::pair<std::vector<CompressedRistretto>, std::vector<ScalarBytes>> commit_rows(const void *values, size_t value_bytes, size_t nb,
                                                                                     const std::vector<ScalarBytes> *blindings, const uint8_t *rng_seed32,
                                                                                     uint64_t first_draw) const {
        if (blindings && blindings->size() != nb) throw std::invalid_argument("commit_batch: one blinding per value");
        std::vector<CompressedRistretto> out(nb);
        std::vector<ScalarBytes> bl(nb);
        std::vector<uint8_t> st(nb);
        const uint8_t *bl_in = blindings && nb ? (*blindings)[0].data() : nullptr;
        if (blindings && (rng_seed32 || first_draw)) throw std::invalid_argument("commit_batch: blindings given, rng_seed32 and first_draw do not apply");
        if (nb == 0) return {out, bl};
        if (bpgpu_pedersen_commit_batch(ctx_.get(), nb, values, value_bytes, bl_in, rng_seed32, first_draw, out[0].data(), bl[0].data(), st.data()) != BPGPU_OK)
            throw GpuError(bpgpu_last_error(ctx_.get()));
        for (size_t i = 0; i < nb; i++)
            if (st[i] != BPGPU_MSM_OK) throw std::invalid_argument("commit_batch: scalars must be canonical");
        return {out, bl};
    }
    std::vector<Status> open_rows(const std::vector<CompressedRistretto> &commitments, const void *values, size_t value_bytes, size_t nb,
                                  const std::vector<ScalarBytes> &blindings) const {
        if (commitments.size() != nb || blindings.size() != nb) throw std::invalid_argument("verify_openings: one commitment and one blinding per value");
        std::vector<uint8_t> vd(nb);
        std::vector<Status> res;
        if (nb == 0) return res;
        if (bpgpu_pedersen_open_batch(ctx_.get(), nb, commitments[0].data(), values, value_bytes, blindings[0].data(), vd.data()) != BPGPU_OK)
            throw GpuError(bpgpu_last_error(ctx_.get()));
        for (size_t i = 0; i < nb; i++) res.push_back(vd[i] == 0 ? Status::Ok() : Status::Err((ProofError)vd[i]));
        return res;
    }
    // the flat form of bpgpu_pedersen_sum_batch: offsets, the rows' added terms followed by their subtracted ones, one sign byte per term
    struct SignedRows {
        std::vector<uint32_t> off;
        std::vector<uint8_t> pts, signs;
    };
    static SignedRows flatten(const Rows &plus, const Rows *minus, size_t n_scalars, const std::vector<ScalarBytes> *blindings, const char *who) {
        if ((minus && minus->size() != plus.size()) || n_scalars != plus.size() || (blindings && blindings->size() != plus.size()))
            throw std::invalid_argument(std::string(who) + ": one list of subtracted commitments, one value and one blinding per row");
        SignedRows f;
        f.off.push_back(0);
        for (size_t r = 0; r < plus.size(); r++) {
            for (int side = 0; side < 2; side++) {
                if (side && !minus) break;
                for (const CompressedRistretto &c : side ? (*minus)[r] : plus[r]) {
                    f.pts.insert(f.pts.end(), c.begin(), c.end());
                    f.signs.push_back(static_cast<uint8_t>(side));
                }
            }
            f.off.push_back(static_cast<uint32_t>(f.signs.size()));
        }
        return f;
    }
    std::vector<std::optional<CompressedRistretto>> sum_rows(const Rows &plus, const Rows *minus, const void *values, size_t value_bytes, size_t n_values,
                                                             const std::vector<ScalarBytes> *blindings) const {
        const SignedRows f = flatten(plus, minus, n_values, blindings, "sum_commitments");
        const size_t nb = plus.size();
        std::vector<std::optional<CompressedRistretto>> res(nb);
        if (nb == 0) return res;
        std::vector<CompressedRistretto> out(nb);
        std::vector<uint8_t> st(nb);
        if (bpgpu_pedersen_sum_batch(ctx_.get(), nb, f.off.data(), f.pts.data(), f.signs.data(), values, value_bytes, blindings ? (*blindings)[0].data() : nullptr,
                                     out[0].data(), st.data()) != BPGPU_OK)
            throw GpuError(bpgpu_last_error(ctx_.get()));
        for (size_t i = 0; i < nb; i++) {
            if (st[i] == BPGPU_MSM_BAD_SCALAR) throw std::invalid_argument("sum_commitments: scalars must be canonical");
            if (st[i] == BPGPU_MSM_OK) res[i] = out[i];
        }
        return res;
    }
    std::vector<Status> balance_rows(const Rows &inputs, const Rows &outputs, const void *values, size_t value_bytes, size_t n_values,
                                     const std::vector<ScalarBytes> *blindings) const {
        const SignedRows f = flatten(inputs, &outputs, n_values, blindings, "verify_balance");
        const size_t nb = inputs.size();
        std::vector<uint8_t> vd(nb);
        std::vector<Status> res;
        if (nb == 0) return res;
        if (bpgpu_pedersen_balance_batch(ctx_.get(), nb, f.off.data(), f.pts.data(), f.signs.data(), values, value_bytes, blindings ? (*blindings)[0].data() : nullptr,
                                         vd.data()) != BPGPU_OK)
            throw GpuError(bpgpu_last_error(ctx_.get()));
        for (size_t i = 0; i < nb; i++) res.push_back(vd[i] == 0 ? Status::Ok() : Status::Err((ProofError)vd[i]));
        return res;
    }
    std::vector<CompressedRistretto> slice(bool g, size_t n, size_t m, size_t first_party) const {
        if (n > gens_capacity || first_party + m > party_capacity) throw std::out_of_range("generators: n or party index beyond capacity");
        const size_t tot = gens_capacity * party_capacity;
        std::vector<uint8_t> flat(tot * 32);
        if (bpgpu_gens_export(ctx_.get(), g ? flat.data() : nullptr, g ? nullptr : flat.data(), nullptr, nullptr) != BPGPU_OK)
            throw GpuError(bpgpu_last_error(ctx_.get()));
        std::vector<CompressedRistretto> out(n * m);
        for (size_t j = 0; j < m; j++)
            for (size_t i = 0; i < n; i++) std::memcpy(out[j * n + i].data(), &flat[((first_party + j) * gens_capacity + i) * 32], 32);
        return out;
    }
    std::shared_ptr<bpgpu_ctx> ctx_;
};

// merlin::Transcript, held as its 208-byte STROBE-128 state (bpgpu.h BPGPU_TRANSCRIPT_BYTES).  It may absorb
// application messages before it is handed to a verifier, and a verifier leaves it advanced, as
// verify_multiple_with_rng(&mut transcript, ...) does (mod.rs:345-353).
class Transcript {
  public:
    explicit Transcript(const std::string &label) : Transcript(reinterpret_cast<const uint8_t *>(label.data()), label.size()) {}
    Transcript(const uint8_t *label, size_t n) : fresh_label_(label, label + n), fresh_(true) {
        if (bpgpu_transcript_new(label, n, state_.data()) != BPGPU_OK) throw std::invalid_argument("bpgpu_transcript_new");
    }
    void append_message(const std::string &label, const uint8_t *msg, size_t n) {
        if (bpgpu_transcript_append_message(state_.data(), reinterpret_cast<const uint8_t *>(label.data()), label.size(), msg, n) != BPGPU_OK)
            throw std::invalid_argument("bpgpu_transcript_append_message");
        fresh_ = false;
    }
    void append_u64(const std::string &label, uint64_t x) {
        uint8_t b[8];
        for (int i = 0; i < 8; i++) b[i] = static_cast<uint8_t>(x >> (8 * i));
        append_message(label, b, 8);
    }
    void challenge_bytes(const std::string &label, uint8_t *out, size_t n) {
        if (bpgpu_transcript_challenge_bytes(state_.data(), reinterpret_cast<const uint8_t *>(label.data()), label.size(), out, n) != BPGPU_OK)
            throw std::invalid_argument("bpgpu_transcript_challenge_bytes");
        fresh_ = false;
    }
    const std::array<uint8_t, BPGPU_TRANSCRIPT_BYTES> &state() const { return state_; }
    std::array<uint8_t, BPGPU_TRANSCRIPT_BYTES> &state_mut() {
        fresh_ = false;
        return state_;
    }
    // the label while the transcript is still exactly Transcript::new(label) (what the batch-combined entry point needs)
    bool is_fresh() const { return fresh_; }
    const std::vector<uint8_t> &label() const { return fresh_label_; }

  private:
    std::array<uint8_t, BPGPU_TRANSCRIPT_BYTES> state_{};
    std::vector<uint8_t> fresh_label_;
    bool fresh_;
};

// n transcripts built and bound on the GPU (bpgpu_transcript_batch): the rows share their labels, the messages are per row.  Appends are
// recorded and sent as ONE script -- by the next challenge, by states(), or when the batch is consumed: the std::vector<Transcript>&
// overloads of RangeProof::prove_batch / verify_batch_combined and LinearProof::create_batch / verify_batch / verify_batch_combined have a
// TranscriptBatch& twin that leaves the batch advanced where the vector would be.
class TranscriptBatch {
  public:
    TranscriptBatch(bpgpu_ctx *ctx, const std::string &label, size_t n) : ctx_(ctx), n_(n), label_(label.begin(), label.end()), fresh_(true) {}
    // n rows that all start from one bound transcript (which is not advanced)
    static TranscriptBatch from_transcript(bpgpu_ctx *ctx, const Transcript &t, size_t n) {
        TranscriptBatch b(ctx, "", n);
        b.fresh_ = false;
        b.states_.assign(t.state().begin(), t.state().end());
        b.shared_ = true;
        return b;
    }
    // rows from per-row states
    static TranscriptBatch from_states(bpgpu_ctx *ctx, const std::vector<Transcript> &ts) {
        TranscriptBatch b(ctx, "", ts.size());
        b.assign(ts);
        return b;
    }
    size_t size() const { return n_; }
    TranscriptBatch clone() const { return *this; }

    // one message per row, of any lengths
    void append_message(const std::string &label, const std::vector<std::vector<uint8_t>> &messages) {
        if (messages.size() != n_) throw std::invalid_argument("append_message: one message per row");
        op o{BPGPU_TS_APPEND, label, {}, 0, 0, {}};
        for (const auto &m : messages) o.len = std::max(o.len, m.size());
        o.stride = o.len;
        o.data.resize(n_ * o.len);
        bool ragged = false;
        for (size_t r = 0; r < n_; r++) {
            if (!messages[r].empty()) std::memcpy(&o.data[r * o.len], messages[r].data(), messages[r].size());
            o.lens.push_back(static_cast<uint32_t>(messages[r].size()));
            ragged = ragged || messages[r].size() != o.len;
        }
        if (!ragged) o.lens.clear();
        pending_.push_back(std::move(o));
    }
    // one message for all rows
    void append_message(const std::string &label, const uint8_t *msg, size_t n) {
        pending_.push_back(op{BPGPU_TS_APPEND, label, std::vector<uint8_t>(msg, msg + n), 0, n, {}});
    }
    void append_u64(const std::string &label, const std::vector<uint64_t> &xs) {
        if (xs.size() != n_) throw std::invalid_argument("append_u64: one value per row");
        op o{BPGPU_TS_APPEND_U64, label, std::vector<uint8_t>(8 * n_), 8, 8, {}};
        if (n_) std::memcpy(o.data.data(), xs.data(), 8 * n_);
        pending_.push_back(std::move(o));
    }
    void append_u64(const std::string &label, uint64_t x) {
        op o{BPGPU_TS_APPEND_U64, label, std::vector<uint8_t>(8), 0, 8, {}};
        std::memcpy(o.data.data(), &x, 8);
        pending_.push_back(std::move(o));
    }
    // n challenge bytes per row
    std::vector<std::vector<uint8_t>> challenge_bytes(const std::string &label, size_t n) {
        pending_.push_back(op{BPGPU_TS_CHALLENGE, label, std::vector<uint8_t>(n_ * n + 1), n ? n : 1, n, {}});
        const std::vector<uint8_t> flat = flush();
        std::vector<std::vector<uint8_t>> out(n_);
        for (size_t r = 0; r < n_; r++) out[r].assign(flat.begin() + r * n, flat.begin() + (r + 1) * n);
        return out;
    }
    // the crate's challenge_scalar per row (transcript.rs:89-95)
    std::vector<ScalarBytes> challenge_scalars(const std::string &label) {
        pending_.push_back(op{BPGPU_TS_CHALLENGE_SCALAR, label, std::vector<uint8_t>(n_ * 32 + 1), 32, 0, {}});
        const std::vector<uint8_t> flat = flush();
        std::vector<ScalarBytes> out(n_);
        for (size_t r = 0; r < n_; r++) std::memcpy(out[r].data(), &flat[r * 32], 32);
        return out;
    }
    // the rows' states, n x BPGPU_TRANSCRIPT_BYTES (what the `_ts` entry points take as `transcripts`)
    const std::vector<uint8_t> &states() {
        if (!pending_.empty() || fresh_ || shared_) flush();
        return states_;
    }
    Transcript operator[](size_t i) {
        Transcript t("");
        std::memcpy(t.state_mut().data(), &states().at(i * BPGPU_TRANSCRIPT_BYTES), BPGPU_TRANSCRIPT_BYTES);
        return t;
    }
    std::vector<Transcript> to_transcripts() {
        std::vector<Transcript> out;
        for (size_t i = 0; i < n_; i++) out.push_back((*this)[i]);
        return out;
    }
    // the rows as some call left them
    void assign(const std::vector<Transcript> &ts) {
        n_ = ts.size();
        states_.resize(n_ * BPGPU_TRANSCRIPT_BYTES);
        for (size_t i = 0; i < n_; i++) std::memcpy(&states_[i * BPGPU_TRANSCRIPT_BYTES], ts[i].state().data(), BPGPU_TRANSCRIPT_BYTES);
        fresh_ = shared_ = false;
        pending_.clear();
    }

  private:
    struct op {
        uint32_t kind;
        std::string label;
        std::vector<uint8_t> data;
        size_t stride, len;
        std::vector<uint32_t> lens;
    };
    // the recorded operations as scripts of at most BPGPU_TS_MAX_OPS; returns the last operation's output rows
    std::vector<uint8_t> flush() {
        std::vector<op> script;
        script.swap(pending_);
        size_t lo = 0;
        do {
            const size_t hi = std::min(script.size(), lo + BPGPU_TS_MAX_OPS);
            std::vector<bpgpu_ts_op> ops;
            for (size_t o = lo; o < hi; o++)
                ops.push_back(bpgpu_ts_op{script[o].kind, reinterpret_cast<const uint8_t *>(script[o].label.data()), script[o].label.size(), script[o].data.data(),
                                          script[o].stride, script[o].len, script[o].lens.empty() ? nullptr : script[o].lens.data()});
            std::vector<uint8_t> out(n_ * BPGPU_TRANSCRIPT_BYTES + 1);
            const int rc = bpgpu_transcript_batch(ctx_, n_, !fresh_ ? nullptr : label_.empty() ? reinterpret_cast<const uint8_t *>("") : label_.data(), fresh_ ? label_.size() : 0, fresh_ ? nullptr : states_.data(),
                                                  fresh_ || shared_ ? 0 : BPGPU_TRANSCRIPT_BYTES, ops.data(), ops.size(), out.data());
            if (rc != BPGPU_OK) throw GpuError(bpgpu_last_error(ctx_));
            out.resize(n_ * BPGPU_TRANSCRIPT_BYTES);
            states_.swap(out);
            fresh_ = shared_ = false;
            lo = hi;
        } while (lo < script.size());
        return script.empty() ? std::vector<uint8_t>() : std::move(script.back().data);
    }
    bpgpu_ctx *ctx_;
    size_t n_;
    std::vector<uint8_t> label_, states_;
    bool fresh_, shared_ = false;
    std::vector<op> pending_;
};

namespace detail {
inline bool scalar_is_canonical(const uint8_t *s) {   // Scalar::from_canonical_bytes
    static const uint8_t L[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                                  0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0x10};
    for (int i = 31; i >= 0; i--) {
        if (s[i] < L[i]) return true;
        if (s[i] > L[i]) return false;
    }
    return false;
}
}  // namespace detail

class RangeProof {
  public:
    // Result<RangeProof, ProofError> of RangeProof::from_bytes (mod.rs:504-538 + ipp.rs:373-407)
    static std::variant<RangeProof, ProofError> from_bytes(const uint8_t *slice, size_t len) {
        if (len % 32 != 0 || len < 7 * 32) return ProofError::FormatError;
        for (int i = 4; i < 7; i++)
            if (!detail::scalar_is_canonical(slice + 32 * i)) return ProofError::FormatError;
        const size_t ne = (len - 7 * 32) / 32;
        if (ne < 2 || (ne - 2) % 2 != 0) return ProofError::FormatError;
        const size_t lg_n = (ne - 2) / 2;
        if (lg_n >= 32) return ProofError::FormatError;
        if (!detail::scalar_is_canonical(slice + len - 64) || !detail::scalar_is_canonical(slice + len - 32)) return ProofError::FormatError;
        RangeProof p;
        p.bytes_.assign(slice, slice + len);
        return p;
    }
    static std::variant<RangeProof, ProofError> from_bytes(const std::vector<uint8_t> &v) { return from_bytes(v.data(), v.size()); }

    // RangeProof::prove_multiple_with_rng (mod.rs:234-288) on the GPU: (proof, value commitments).  `transcript` is &mut
    // (left advanced).  rng_bytes: the bytes the rng would hand Scalar::random, in the reference's draw order --
    // 64 * (m (2n + 2) + 2m) of them -- or nullptr for the OS CSPRNG.  VARIABLE TIME in the secrets (see bpgpu.h).
    static std::pair<RangeProof, std::vector<CompressedRistretto>> prove_multiple_with_rng(const BulletproofGens &bp_gens, const PedersenGens &pc_gens,
                                                                                           Transcript &transcript, const std::vector<uint64_t> &values,
                                                                                           const std::vector<ScalarBytes> &blindings, size_t n,
                                                                                           const uint8_t *rng_bytes = nullptr) {
        bp_gens.check_pedersen(pc_gens);
        const size_t m = values.size();
        if (blindings.size() != m) throw std::invalid_argument("prove_multiple: WrongNumBlindingFactors");
        size_t k = 0;
        while ((size_t(1) << k) < n * m) k++;
        RangeProof p;
        p.bytes_.resize(32 * (9 + 2 * k));
        std::vector<CompressedRistretto> vc(m);
        std::vector<uint8_t> bl(32 * m);
        for (size_t j = 0; j < m; j++) std::memcpy(&bl[32 * j], blindings[j].data(), 32);
        std::array<uint8_t, BPGPU_TRANSCRIPT_BYTES> in = transcript.state();
        const int rc = bpgpu_rangeproof_prove_batch(bp_gens.ctx(), n, m, 1, values.data(), bl.data(), nullptr, 0, in.data(), rng_bytes, p.bytes_.data(),
                                                    m ? vc[0].data() : nullptr, transcript.state_mut().data());
        if (rc != BPGPU_OK) throw GpuError(bpgpu_last_error(bp_gens.ctx()));
        return {p, vc};
    }
    static std::pair<RangeProof, CompressedRistretto> prove_single_with_rng(const BulletproofGens &bp_gens, const PedersenGens &pc_gens, Transcript &transcript,
                                                                            uint64_t v, const ScalarBytes &v_blinding, size_t n,
                                                                            const uint8_t *rng_bytes = nullptr) {
        auto r = prove_multiple_with_rng(bp_gens, pc_gens, transcript, {v}, {v_blinding}, n, rng_bytes);
        return {r.first, r.second[0]};
    }
    // prove_multiple / prove_single (mod.rs:290-311, 141-158): thread_rng() -> the OS CSPRNG
    static std::pair<RangeProof, std::vector<CompressedRistretto>> prove_multiple(const BulletproofGens &bp_gens, const PedersenGens &pc_gens,
                                                                                  Transcript &transcript, const std::vector<uint64_t> &values,
                                                                                  const std::vector<ScalarBytes> &blindings, size_t n) {
        return prove_multiple_with_rng(bp_gens, pc_gens, transcript, values, blindings, n, nullptr);
    }
    static std::pair<RangeProof, CompressedRistretto> prove_single(const BulletproofGens &bp_gens, const PedersenGens &pc_gens, Transcript &transcript,
                                                                   uint64_t v, const ScalarBytes &v_blinding, size_t n) {
        return prove_single_with_rng(bp_gens, pc_gens, transcript, v, v_blinding, n, nullptr);
    }
    // values.size() proofs in ONE GPU pass (bpgpu_rangeproof_prove_batch_ts; no counterpart in the crate): values[i] / blindings[i] are
    // the m values / blindings of proof i; transcripts: ONE bound transcript, the start state of every proof (not advanced), or one
    // per proof, each left advanced as prove_multiple_with_rng leaves it.  rng32: 32 bytes per proof, proof i's rng being
    // ChaChaRng::from_seed(rng32 + 32 i), its scalars drawn on the device; nullptr: the library draws the seeds.
    static std::vector<std::pair<RangeProof, std::vector<CompressedRistretto>>> prove_batch(const BulletproofGens &bp_gens, const PedersenGens &pc_gens,
                                                                                            std::vector<Transcript> &transcripts,
                                                                                            const std::vector<std::vector<uint64_t>> &values,
                                                                                            const std::vector<std::vector<ScalarBytes>> &blindings, size_t n,
                                                                                            const uint8_t *rng32 = nullptr) {
        bp_gens.check_pedersen(pc_gens);
        const size_t nb = values.size(), m = nb ? values[0].size() : 0;
        std::vector<std::pair<RangeProof, std::vector<CompressedRistretto>>> out(nb);
        if (!nb) return out;
        if (blindings.size() != nb || (transcripts.size() != nb && transcripts.size() != 1)) throw std::invalid_argument("prove_batch: one row per proof");
        const bool per_proof = transcripts.size() == nb && nb != 1;
        size_t k = 0;
        while ((size_t(1) << k) < n * m) k++;
        const size_t pl = 32 * (9 + 2 * k), TS = BPGPU_TRANSCRIPT_BYTES;
        std::vector<uint64_t> va(nb * m);
        std::vector<uint8_t> bl(32 * nb * m), ts(per_proof ? nb * TS : TS), tso(nb * TS), pr(nb * pl), vc(32 * nb * m);
        for (size_t i = 0; i < nb; i++) {
            if (values[i].size() != m || blindings[i].size() != m) throw std::invalid_argument("prove_batch: WrongNumBlindingFactors");
            for (size_t j = 0; j < m; j++) {
                va[i * m + j] = values[i][j];
                std::memcpy(&bl[32 * (i * m + j)], blindings[i][j].data(), 32);
            }
            if (per_proof || i == 0) std::memcpy(&ts[i * TS], transcripts[i].state().data(), TS);
        }
        const int rc = bpgpu_rangeproof_prove_batch_ts(bp_gens.ctx(), n, m, nb, va.data(), bl.data(), ts.data(), per_proof ? TS : 0, rng32, pr.data(),
                                                       vc.data(), tso.data());
        if (rc != BPGPU_OK) throw GpuError(bpgpu_last_error(bp_gens.ctx()));
        for (size_t i = 0; i < nb; i++) {
            out[i].first.bytes_.assign(pr.begin() + i * pl, pr.begin() + (i + 1) * pl);
            out[i].second.resize(m);
            for (size_t j = 0; j < m; j++) std::memcpy(out[i].second[j].data(), &vc[32 * (i * m + j)], 32);
            if (transcripts.size() == nb) std::memcpy(transcripts[i].state_mut().data(), &tso[i * TS], TS);
        }
        return out;
    }
    // ... on a TranscriptBatch, one row per proof, left advanced as the vector would be
    static std::vector<std::pair<RangeProof, std::vector<CompressedRistretto>>> prove_batch(const BulletproofGens &bp_gens, const PedersenGens &pc_gens,
                                                                                            TranscriptBatch &transcripts,
                                                                                            const std::vector<std::vector<uint64_t>> &values,
                                                                                            const std::vector<std::vector<ScalarBytes>> &blindings, size_t n,
                                                                                            const uint8_t *rng32 = nullptr) {
        if (transcripts.size() != values.size()) throw std::invalid_argument("prove_batch: one row per proof");
        std::vector<Transcript> ts = transcripts.to_transcripts();
        auto out = prove_batch(bp_gens, pc_gens, ts, values, blindings, n, rng32);
        transcripts.assign(ts);
        return out;
    }

    // ---- rewindable proofs (bpgpu_rangeproof_prove_batch_rw / bpgpu_rangeproof_rewind_batch; no counterpart in the crate; m = 1) ----
    // What a rewound row gives back: the value, its blinding and the 16-byte message the prover put in.
    struct Rewound {
        uint64_t value;
        ScalarBytes blinding;
        std::array<uint8_t, 16> message;
    };
    // values.size() rewindable proofs in ONE GPU pass: prove_batch with one value per proof and a_blinding = draw 0 - (value + 2^64
    // message), so that whoever holds proof i's seed (rng32 + 32 i, REQUIRED) gets (value, blinding, message) back with rewind_batch.
    // messages: empty (every message zero) or one per proof.  transcripts: as prove_batch.  A seed must never serve two
    // (commitment, transcript) pairs: derive it with rewind_seeds.
    static std::vector<std::pair<RangeProof, CompressedRistretto>> prove_batch_rewindable(const BulletproofGens &bp_gens, const PedersenGens &pc_gens,
                                                                                          std::vector<Transcript> &transcripts, const std::vector<uint64_t> &values,
                                                                                          const std::vector<ScalarBytes> &blindings, size_t n, const uint8_t *rng32,
                                                                                          const std::vector<std::array<uint8_t, 16>> &messages = {}) {
        bp_gens.check_pedersen(pc_gens);
        const size_t nb = values.size();
        std::vector<std::pair<RangeProof, CompressedRistretto>> out(nb);
        if (!nb) return out;
        if (blindings.size() != nb || (transcripts.size() != nb && transcripts.size() != 1) || (!messages.empty() && messages.size() != nb))
            throw std::invalid_argument("prove_batch_rewindable: one row per proof");
        if (!rng32) throw std::invalid_argument("prove_batch_rewindable: the seeds are required");
        const bool per_proof = transcripts.size() == nb && nb != 1;
        size_t k = 0;
        while ((size_t(1) << k) < n) k++;
        const size_t pl = 32 * (9 + 2 * k), TS = BPGPU_TRANSCRIPT_BYTES;
        std::vector<uint8_t> bl(32 * nb), ts(per_proof ? nb * TS : TS), tso(nb * TS), pr(nb * pl), vc(32 * nb), msg(messages.empty() ? 0 : 16 * nb);
        for (size_t i = 0; i < nb; i++) {
            std::memcpy(&bl[32 * i], blindings[i].data(), 32);
            if (!messages.empty()) std::memcpy(&msg[16 * i], messages[i].data(), 16);
            if (per_proof || i == 0) std::memcpy(&ts[i * TS], transcripts[i].state().data(), TS);
        }
        const int rc = bpgpu_rangeproof_prove_batch_rw(bp_gens.ctx(), n, 1, nb, values.data(), bl.data(), ts.data(), per_proof ? TS : 0, rng32,
                                                       messages.empty() ? nullptr : msg.data(), pr.data(), vc.data(), tso.data());
        if (rc != BPGPU_OK) throw GpuError(bpgpu_last_error(bp_gens.ctx()));
        for (size_t i = 0; i < nb; i++) {
            out[i].first.bytes_.assign(pr.begin() + i * pl, pr.begin() + (i + 1) * pl);
            std::memcpy(out[i].second.data(), &vc[32 * i], 32);
            if (transcripts.size() == nb) std::memcpy(transcripts[i].state_mut().data(), &tso[i * TS], TS);
        }
        return out;
    }
    // Rewind every (proofs[i], commitments[i]) under seeds + 32 i in ONE GPU launch.  transcripts: ONE bound transcript, the start state
    // of every row, or one per row; none is advanced.  A row that is the seed holder's own gives its Rewound, any other std::nullopt;
    // a proof that from_bytes rejects (or a length that is not that of an (n, 1) proof) makes the call return FormatError.
    // This does NOT verify the proofs: a recovered message is only as good as the proof's verification.
    static std::variant<std::vector<std::optional<Rewound>>, ProofError> rewind_batch(const BulletproofGens &bp_gens, const PedersenGens &pc_gens,
                                                                                      const std::vector<Transcript> &transcripts,
                                                                                      const std::vector<std::vector<uint8_t>> &proofs,
                                                                                      const std::vector<CompressedRistretto> &commitments, size_t n,
                                                                                      const uint8_t *seeds) {
        bp_gens.check_pedersen(pc_gens);
        const size_t nb = proofs.size();
        std::vector<std::optional<Rewound>> out(nb);
        if (!nb) return out;
        if (commitments.size() != nb || (transcripts.size() != nb && transcripts.size() != 1) || !seeds) throw std::invalid_argument("rewind_batch: one row per proof");
        const bool per_proof = transcripts.size() == nb && nb != 1;
        size_t k = 0;
        while ((size_t(1) << k) < n) k++;
        const size_t pl = 32 * (9 + 2 * k), TS = BPGPU_TRANSCRIPT_BYTES;
        std::vector<uint8_t> pr(nb * pl), vc(32 * nb), ts(per_proof ? nb * TS : TS), st(nb), msg(16 * nb), bl(32 * nb);
        std::vector<uint64_t> va(nb);
        for (size_t i = 0; i < nb; i++) {
            if (proofs[i].size() != pl) return ProofError::FormatError;
            std::memcpy(&pr[i * pl], proofs[i].data(), pl);
            std::memcpy(&vc[32 * i], commitments[i].data(), 32);
            if (per_proof || i == 0) std::memcpy(&ts[i * TS], transcripts[i].state().data(), TS);
        }
        const int rc = bpgpu_rangeproof_rewind_batch(bp_gens.ctx(), n, nb, pr.data(), pl, vc.data(), ts.data(), per_proof ? TS : 0, seeds, st.data(), va.data(),
                                                     msg.data(), bl.data());
        if (rc != BPGPU_OK) throw GpuError(bpgpu_last_error(bp_gens.ctx()));
        for (size_t i = 0; i < nb; i++) {
            if (st[i] == BPGPU_REWIND_FORMAT) return ProofError::FormatError;
            if (st[i] != BPGPU_REWIND_OK) continue;
            Rewound r;
            r.value = va[i];
            std::memcpy(r.blinding.data(), &bl[32 * i], 32);
            std::memcpy(r.message.data(), &msg[16 * i], 16);
            out[i] = r;
        }
        return out;
    }
    // Scan every (proofs[i], commitments[i]) under nkeys wallet keys (keys32: nkeys x 32 bytes, shared by every row) with ONE transcript
    // replay per row (bpgpu_rangeproof_scan_batch): the seed of (key j, commitment i) is rewind_seeds' derivation.  A row that one of
    // the keys opens gives (index of that key, its Rewound), any other std::nullopt; FormatError as rewind_batch.  The lowest key that
    // passes the 2^192 test decides a row (bpgpu.h).  This does NOT verify the proofs.
    static std::variant<std::vector<std::optional<std::pair<uint32_t, Rewound>>>, ProofError> scan_batch(const BulletproofGens &bp_gens, const PedersenGens &pc_gens,
                                                                                                        const std::vector<Transcript> &transcripts,
                                                                                                        const std::vector<std::vector<uint8_t>> &proofs,
                                                                                                        const std::vector<CompressedRistretto> &commitments,
                                                                                                        size_t n, const uint8_t *keys32, size_t nkeys) {
        bp_gens.check_pedersen(pc_gens);
        const size_t nb = proofs.size();
        std::vector<std::optional<std::pair<uint32_t, Rewound>>> out(nb);
        if (!nb) return out;
        if (commitments.size() != nb || (transcripts.size() != nb && transcripts.size() != 1) || !keys32) throw std::invalid_argument("scan_batch: one row per proof, and the keys");
        const bool per_proof = transcripts.size() == nb && nb != 1;
        size_t k = 0;
        while ((size_t(1) << k) < n) k++;
        const size_t pl = 32 * (9 + 2 * k), TS = BPGPU_TRANSCRIPT_BYTES;
        std::vector<uint8_t> pr(nb * pl), vc(32 * nb), ts(per_proof ? nb * TS : TS), st(nb), msg(16 * nb), bl(32 * nb);
        std::vector<uint64_t> va(nb);
        std::vector<uint32_t> ki(nb);
        for (size_t i = 0; i < nb; i++) {
            if (proofs[i].size() != pl) return ProofError::FormatError;
            std::memcpy(&pr[i * pl], proofs[i].data(), pl);
            std::memcpy(&vc[32 * i], commitments[i].data(), 32);
            if (per_proof || i == 0) std::memcpy(&ts[i * TS], transcripts[i].state().data(), TS);
        }
        const int rc = bpgpu_rangeproof_scan_batch(bp_gens.ctx(), n, nb, pr.data(), pl, vc.data(), ts.data(), per_proof ? TS : 0, keys32, nkeys, st.data(), ki.data(),
                                                   va.data(), msg.data(), bl.data());
        if (rc != BPGPU_OK) throw GpuError(bpgpu_last_error(bp_gens.ctx()));
        for (size_t i = 0; i < nb; i++) {
            if (st[i] == BPGPU_REWIND_FORMAT) return ProofError::FormatError;
            if (st[i] != BPGPU_REWIND_OK) continue;
            Rewound r;
            r.value = va[i];
            std::memcpy(r.blinding.data(), &bl[32 * i], 32);
            std::memcpy(r.message.data(), &msg[16 * i], 16);
            out[i] = std::make_pair(ki[i], r);
        }
        return out;
    }
    // one proof: the Rewound of V if this proof was made rewindable under seed32 on `transcript` (not advanced), std::nullopt if not
    std::variant<std::optional<Rewound>, ProofError> rewind_single(const BulletproofGens &bp_gens, const PedersenGens &pc_gens, const Transcript &transcript,
                                                                   const CompressedRistretto &V, size_t n, const uint8_t *seed32) const {
        auto r = rewind_batch(bp_gens, pc_gens, std::vector<Transcript>{transcript}, {bytes_}, {V}, n, seed32);
        if (std::holds_alternative<ProofError>(r)) return std::get<ProofError>(r);
        return std::get<0>(r)[0];
    }
    // One seed per commitment from a 32-byte wallet key, derived on the GPU (the derivation fixed in bpgpu.h): Transcript::new(b"bpgpu
    // rewind seed v1"), append_message(b"key", key32), append_message(b"C", commitment_i), challenge_bytes(b"seed", 32).  Returns the
    // seeds concatenated: the rng32 of prove_batch_rewindable and the seeds of rewind_batch.
    static std::vector<uint8_t> rewind_seeds(bpgpu_ctx *ctx, const uint8_t *key32, const std::vector<CompressedRistretto> &commitments) {
        std::vector<uint8_t> out;
        if (commitments.empty()) return out;
        TranscriptBatch t(ctx, "bpgpu rewind seed v1", commitments.size());
        t.append_message("key", key32, 32);
        std::vector<std::vector<uint8_t>> cs;
        for (const auto &c : commitments) cs.emplace_back(c.begin(), c.end());
        t.append_message("C", cs);
        for (const auto &s : t.challenge_bytes("seed", 32)) out.insert(out.end(), s.begin(), s.end());
        return out;
    }
    const std::vector<uint8_t> &to_bytes() const { return bytes_; }

    // verify_multiple_with_rng: rng64 = the 64 bytes the rng would hand Scalar::random (mod.rs:396)
    // (`transcript` is `&mut Transcript`: it may hold earlier messages and is left advanced)
    Status verify_multiple_with_rng(const BulletproofGens &bp_gens, const PedersenGens &pc_gens, Transcript &transcript,
                                    const std::vector<CompressedRistretto> &value_commitments, size_t n, const uint8_t *rng64) const {
        bp_gens.check_pedersen(pc_gens);
        uint8_t verdict = 0;
        std::array<uint8_t, BPGPU_TRANSCRIPT_BYTES> in = transcript.state();
        const int rc = bpgpu_rangeproof_verify_batch_ts(bp_gens.ctx(), n, value_commitments.size(), 1, bytes_.data(), bytes_.size(),
                                                        value_commitments.empty() ? nullptr : value_commitments[0].data(), in.data(),
                                                        BPGPU_TRANSCRIPT_BYTES, rng64, &verdict, nullptr, transcript.state_mut().data());
        if (rc != BPGPU_OK) throw GpuError(bpgpu_last_error(bp_gens.ctx()));
        return verdict == 0 ? Status::Ok() : Status::Err(static_cast<ProofError>(verdict));
    }
    Status verify_multiple_with_rng(const BulletproofGens &bp_gens, const PedersenGens &pc_gens, Transcript &&transcript,
                                    const std::vector<CompressedRistretto> &value_commitments, size_t n, const uint8_t *rng64) const {
        return verify_multiple_with_rng(bp_gens, pc_gens, transcript, value_commitments, n, rng64);
    }
    // verify_multiple: thread_rng() -> the library draws from the OS CSPRNG
    Status verify_multiple(const BulletproofGens &bp_gens, const PedersenGens &pc_gens, Transcript &transcript,
                           const std::vector<CompressedRistretto> &value_commitments, size_t n) const {
        return verify_multiple_with_rng(bp_gens, pc_gens, transcript, value_commitments, n, nullptr);
    }
    Status verify_multiple(const BulletproofGens &bp_gens, const PedersenGens &pc_gens, Transcript &&transcript,
                           const std::vector<CompressedRistretto> &value_commitments, size_t n) const {
        return verify_multiple_with_rng(bp_gens, pc_gens, transcript, value_commitments, n, nullptr);
    }
    Status verify_single_with_rng(const BulletproofGens &bp_gens, const PedersenGens &pc_gens, Transcript &transcript,
                                  const CompressedRistretto &V, size_t n, const uint8_t *rng64) const {
        return verify_multiple_with_rng(bp_gens, pc_gens, transcript, {V}, n, rng64);
    }
    Status verify_single_with_rng(const BulletproofGens &bp_gens, const PedersenGens &pc_gens, Transcript &&transcript,
                                  const CompressedRistretto &V, size_t n, const uint8_t *rng64) const {
        return verify_multiple_with_rng(bp_gens, pc_gens, transcript, {V}, n, rng64);
    }
    Status verify_single(const BulletproofGens &bp_gens, const PedersenGens &pc_gens, Transcript &transcript,
                         const CompressedRistretto &V, size_t n) const {
        return verify_multiple_with_rng(bp_gens, pc_gens, transcript, {V}, n, nullptr);
    }
    Status verify_single(const BulletproofGens &bp_gens, const PedersenGens &pc_gens, Transcript &&transcript,
                         const CompressedRistretto &V, size_t n) const {
        return verify_multiple_with_rng(bp_gens, pc_gens, transcript, {V}, n, nullptr);
    }

    // Batched form: proofs[i].verify_multiple(bp_gens, pc_gens, &mut transcript.clone(), &commitments[i], n)
    // for all i in one GPU pass (`transcript` itself is not advanced).  All proofs must share the aggregation size m
    // and the byte length.
    static std::vector<Status> verify_batch(const BulletproofGens &bp_gens, const PedersenGens &pc_gens, const Transcript &transcript,
                                            const std::vector<std::vector<uint8_t>> &proofs,
                                            const std::vector<std::vector<CompressedRistretto>> &commitments, size_t n,
                                            const uint8_t *rng64 = nullptr) {
        const size_t nb = proofs.size();
        std::vector<Status> out;
        if (nb == 0) return out;
        bp_gens.check_pedersen(pc_gens);
        const size_t m = commitments.at(0).size(), len = proofs[0].size();
        std::vector<uint8_t> flat(nb * len), vs(nb * m * 32), verdict(nb);
        for (size_t i = 0; i < nb; i++) {
            if (proofs[i].size() != len || commitments.at(i).size() != m) throw std::invalid_argument("verify_batch: proofs of one call share (m, length)");
            std::memcpy(&flat[i * len], proofs[i].data(), len);
            for (size_t j = 0; j < m; j++) std::memcpy(&vs[(i * m + j) * 32], commitments[i][j].data(), 32);
        }
        const int rc = bpgpu_rangeproof_verify_batch_ts(bp_gens.ctx(), n, m, nb, flat.data(), len, vs.data(), transcript.state().data(), 0, rng64,
                                                        verdict.data(), nullptr, nullptr);
        if (rc != BPGPU_OK) throw GpuError(bpgpu_last_error(bp_gens.ctx()));
        for (size_t i = 0; i < nb; i++) out.push_back(verdict[i] == 0 ? Status::Ok() : Status::Err(static_cast<ProofError>(verdict[i])));
        return out;
    }

    // Same verdicts through the batch-combined check (bpgpu_rangeproof_verify_rlc / _rlc_ts, no counterpart in the crate): one
    // identity test for the whole batch when every proof verifies, per-proof re-verification inside the call when
    // not.  weights64 = nullptr draws the combination weights from the OS CSPRNG.
    // A fresh Transcript(label) is replayed from its label; a transcript the caller has already bound to its transaction or session
    // (the `&mut Transcript` of mod.rs:345-353) goes to bpgpu_rangeproof_verify_rlc_ts as the batch's one start state.  `transcript`
    // itself is not advanced, as in verify_batch.
    static std::vector<Status> verify_batch_combined(const BulletproofGens &bp_gens, const PedersenGens &pc_gens, const Transcript &transcript,
                                                     const std::vector<std::vector<uint8_t>> &proofs,
                                                     const std::vector<std::vector<CompressedRistretto>> &commitments, size_t n,
                                                     const uint8_t *rng64 = nullptr, const uint8_t *weights64 = nullptr) {
        const size_t nb = proofs.size();
        std::vector<Status> out;
        if (nb == 0) return out;
        bp_gens.check_pedersen(pc_gens);
        size_t m = 0, len = 0;
        std::vector<uint8_t> flat, vs, verdict(nb);
        flatten(proofs, commitments, flat, vs, m, len);
        const int rc = transcript.is_fresh()
                           ? bpgpu_rangeproof_verify_rlc(bp_gens.ctx(), n, m, nb, flat.data(), len, vs.data(), transcript.label().data(), transcript.label().size(),
                                                         rng64, weights64, verdict.data(), nullptr)
                           : bpgpu_rangeproof_verify_rlc_ts(bp_gens.ctx(), n, m, nb, flat.data(), len, vs.data(), transcript.state().data(), 0, rng64, weights64,
                                                            verdict.data(), nullptr, nullptr);
        if (rc != BPGPU_OK) throw GpuError(bpgpu_last_error(bp_gens.ctx()));
        for (size_t i = 0; i < nb; i++) out.push_back(verdict[i] == 0 ? Status::Ok() : Status::Err(static_cast<ProofError>(verdict[i])));
        return out;
    }
    // ... with ONE transcript per proof, each at whatever position its history left it (bpgpu_rangeproof_verify_rlc_ts, one state per
    // proof).  The transcripts are not advanced.
    static std::vector<Status> verify_batch_combined(const BulletproofGens &bp_gens, const PedersenGens &pc_gens, const std::vector<Transcript> &transcripts,
                                                     const std::vector<std::vector<uint8_t>> &proofs,
                                                     const std::vector<std::vector<CompressedRistretto>> &commitments, size_t n,
                                                     const uint8_t *rng64 = nullptr, const uint8_t *weights64 = nullptr) {
        const size_t nb = proofs.size();
        std::vector<Status> out;
        if (transcripts.size() != nb) throw std::invalid_argument("verify_batch_combined: one transcript per proof");
        if (nb == 0) return out;
        bp_gens.check_pedersen(pc_gens);
        size_t m = 0, len = 0;
        std::vector<uint8_t> flat, vs, verdict(nb), states(nb * BPGPU_TRANSCRIPT_BYTES);
        flatten(proofs, commitments, flat, vs, m, len);
        for (size_t i = 0; i < nb; i++) std::memcpy(&states[i * BPGPU_TRANSCRIPT_BYTES], transcripts[i].state().data(), BPGPU_TRANSCRIPT_BYTES);
        const int rc = bpgpu_rangeproof_verify_rlc_ts(bp_gens.ctx(), n, m, nb, flat.data(), len, vs.data(), states.data(), BPGPU_TRANSCRIPT_BYTES, rng64,
                                                      weights64, verdict.data(), nullptr, nullptr);
        if (rc != BPGPU_OK) throw GpuError(bpgpu_last_error(bp_gens.ctx()));
        for (size_t i = 0; i < nb; i++) out.push_back(verdict[i] == 0 ? Status::Ok() : Status::Err(static_cast<ProofError>(verdict[i])));
        return out;
    }
    static std::vector<Status> verify_batch_combined(const BulletproofGens &bp_gens, const PedersenGens &pc_gens, TranscriptBatch &transcripts,
                                                     const std::vector<std::vector<uint8_t>> &proofs,
                                                     const std::vector<std::vector<CompressedRistretto>> &commitments, size_t n,
                                                     const uint8_t *rng64 = nullptr, const uint8_t *weights64 = nullptr) {
        return verify_batch_combined(bp_gens, pc_gens, transcripts.to_transcripts(), proofs, commitments, n, rng64, weights64);
    }

  private:
    // the proofs and commitments of one combined call as flat buffers; they share (m, length)
    static void flatten(const std::vector<std::vector<uint8_t>> &proofs, const std::vector<std::vector<CompressedRistretto>> &commitments,
                        std::vector<uint8_t> &flat, std::vector<uint8_t> &vs, size_t &m, size_t &len) {
        const size_t nb = proofs.size();
        m = commitments.at(0).size(), len = proofs[0].size();
        flat.resize(nb * len), vs.resize(nb * m * 32);
        for (size_t i = 0; i < nb; i++) {
            if (proofs[i].size() != len || commitments.at(i).size() != m) throw std::invalid_argument("verify_batch_combined: proofs of one call share (m, length)");
            std::memcpy(&flat[i * len], proofs[i].data(), len);
            for (size_t j = 0; j < m; j++) std::memcpy(&vs[(i * m + j) * 32], commitments[i][j].data(), 32);
        }
    }
    std::vector<uint8_t> bytes_;
};

// LinearProof (src/linear_proof.rs, `pub use` lib.rs:36): <a, b> = c for a committed secret a and a public b.
// from_bytes :350-394, to_bytes :322-331, serialized_size :318-320, verify :175-236.  The reference's verify takes no
// generator object; here the device context that runs the check is passed explicitly (any BulletproofGens holds one).
class LinearProof {
  public:
    static std::variant<LinearProof, ProofError> from_bytes(const uint8_t *slice, size_t len) {
        if (len % 32 != 0) return ProofError::FormatError;
        const size_t ne = len / 32;
        if (ne < 3 || (ne - 3) % 2 != 0 || (ne - 3) / 2 >= 32) return ProofError::FormatError;
        if (!detail::scalar_is_canonical(slice + len - 64) || !detail::scalar_is_canonical(slice + len - 32)) return ProofError::FormatError;
        LinearProof p;
        p.bytes_.assign(slice, slice + len);
        return p;
    }
    static std::variant<LinearProof, ProofError> from_bytes(const std::vector<uint8_t> &v) { return from_bytes(v.data(), v.size()); }
    const std::vector<uint8_t> &to_bytes() const { return bytes_; }
    size_t serialized_size() const { return bytes_.size(); }

    // LinearProof::create(transcript, rng, &C, r, a_vec, b_vec, G_vec, &F, &B) (:40-173) on the GPU, variable time like the
    // reference's.  rng_bytes: the 64 * (2 lg n + 2) bytes the rng would yield to Scalar::random (nullptr = OS CSPRNG).
    static std::variant<LinearProof, ProofError> create(bpgpu_ctx *ctx, Transcript &transcript, const uint8_t *rng_bytes, const CompressedRistretto &C,
                                                        const ScalarBytes &r, const std::vector<ScalarBytes> &a_vec, const std::vector<ScalarBytes> &b_vec,
                                                        const std::vector<CompressedRistretto> &G_vec, const CompressedRistretto &F,
                                                        const CompressedRistretto &B) {
        const size_t n = b_vec.size();
        if (G_vec.size() != n) return ProofError::InvalidGeneratorsLength;                                        // :61-63
        if (a_vec.size() != n || n == 0 || (n & (n - 1))) throw std::invalid_argument("InvalidInputLength");       // :64-70
        size_t lg = 0;
        while ((size_t(1) << lg) < n) lg++;
        LinearProof p;
        p.bytes_.resize(32 * (2 * lg + 3));
        uint8_t status = 0;
        std::array<uint8_t, BPGPU_TRANSCRIPT_BYTES> in = transcript.state();
        const int rc = bpgpu_linear_create_batch(ctx, n, 1, nullptr, 0, in.data(), rng_bytes, C.data(), r.data(), a_vec[0].data(), b_vec[0].data(), 0,
                                                 G_vec[0].data(), F.data(), B.data(), p.bytes_.data(), &status, transcript.state_mut().data());
        if (rc != BPGPU_OK) throw GpuError(bpgpu_last_error(ctx));
        if (status != 0) throw std::invalid_argument("an input point does not decode or a scalar is not canonical");
        return p;
    }

    // LinearProof::verify(&self, transcript, C, G, F, B, b_vec); the transcript is left advanced
    Status verify(bpgpu_ctx *ctx, Transcript &transcript, const CompressedRistretto &C, const std::vector<CompressedRistretto> &G,
                  const CompressedRistretto &F, const CompressedRistretto &B, const std::vector<ScalarBytes> &b_vec) const {
        if (G.size() != b_vec.size()) return Status::Err(ProofError::InvalidGeneratorsLength);   // :189-191
        uint8_t verdict = 0;
        std::array<uint8_t, BPGPU_TRANSCRIPT_BYTES> in = transcript.state();
        const int rc = bpgpu_linear_verify_batch(ctx, b_vec.size(), 1, bytes_.data(), bytes_.size(), nullptr, 0, in.data(), C.data(),
                                                 G.empty() ? nullptr : G[0].data(), F.data(), B.data(), b_vec.empty() ? nullptr : b_vec[0].data(), 0,
                                                 &verdict, nullptr, transcript.state_mut().data());
        if (rc != BPGPU_OK) throw GpuError(bpgpu_last_error(ctx));
        return verdict == 0 ? Status::Ok() : Status::Err(static_cast<ProofError>(verdict));
    }
    // many proofs of one size over the same G, F, B in one GPU pass; b_vecs holds one public vector per proof.
    // `transcript` is cloned per proof and not advanced.
    static std::vector<Status> verify_batch(bpgpu_ctx *ctx, const Transcript &transcript, const std::vector<LinearProof> &proofs,
                                            const std::vector<CompressedRistretto> &Cs, const std::vector<CompressedRistretto> &G,
                                            const CompressedRistretto &F, const CompressedRistretto &B,
                                            const std::vector<std::vector<ScalarBytes>> &b_vecs) {
        const size_t nb = proofs.size(), n = G.size();
        std::vector<Status> out;
        if (nb == 0) return out;
        if (Cs.size() != nb || b_vecs.size() != nb) throw std::invalid_argument("one commitment and one public vector per proof");
        const size_t pl = proofs[0].bytes_.size();
        std::vector<uint8_t> pb, cb, bb, verdict(nb);
        for (size_t i = 0; i < nb; i++) {
            if (proofs[i].bytes_.size() != pl || b_vecs[i].size() != n) throw std::invalid_argument("proofs of a batch must have one size");
            pb.insert(pb.end(), proofs[i].bytes_.begin(), proofs[i].bytes_.end());
            cb.insert(cb.end(), Cs[i].begin(), Cs[i].end());
            for (const auto &x : b_vecs[i]) bb.insert(bb.end(), x.begin(), x.end());
        }
        const int rc = bpgpu_linear_verify_batch(ctx, n, nb, pb.data(), pl, nullptr, 0, transcript.state().data(), cb.data(),
                                                 n ? G[0].data() : nullptr, F.data(), B.data(), n ? bb.data() : nullptr, 0, verdict.data(), nullptr,
                                                 nullptr);
        if (rc != BPGPU_OK) throw GpuError(bpgpu_last_error(ctx));
        for (uint8_t v : verdict) out.push_back(v == 0 ? Status::Ok() : Status::Err(static_cast<ProofError>(v)));
        return out;
    }
    // verify_batch's arguments and verdicts through the batch-combined check (bpgpu_linear_verify_rlc; no counterpart in the crate):
    // one identity test per batch when every proof verifies, per-proof re-verification inside the call when not.  weights64: 64 bytes
    // per proof, unpredictable to the provers, or nullptr (drawn by the library).
    static std::vector<Status> verify_batch_combined(bpgpu_ctx *ctx, const Transcript &transcript, const std::vector<LinearProof> &proofs,
                                                     const std::vector<CompressedRistretto> &Cs, const std::vector<CompressedRistretto> &G,
                                                     const CompressedRistretto &F, const CompressedRistretto &B,
                                                     const std::vector<std::vector<ScalarBytes>> &b_vecs, const uint8_t *weights64 = nullptr) {
        const size_t nb = proofs.size(), n = G.size();
        std::vector<Status> out;
        if (nb == 0) return out;
        if (Cs.size() != nb || b_vecs.size() != nb) throw std::invalid_argument("one commitment and one public vector per proof");
        const size_t pl = proofs[0].bytes_.size();
        std::vector<uint8_t> pb, cb, bb, verdict(nb);
        for (size_t i = 0; i < nb; i++) {
            if (proofs[i].bytes_.size() != pl || b_vecs[i].size() != n) throw std::invalid_argument("proofs of a batch must have one size");
            pb.insert(pb.end(), proofs[i].bytes_.begin(), proofs[i].bytes_.end());
            cb.insert(cb.end(), Cs[i].begin(), Cs[i].end());
            for (const auto &x : b_vecs[i]) bb.insert(bb.end(), x.begin(), x.end());
        }
        const int rc = bpgpu_linear_verify_rlc(ctx, n, nb, pb.data(), pl, nullptr, 0, transcript.state().data(), cb.data(),
                                               n ? G[0].data() : nullptr, F.data(), B.data(), n ? bb.data() : nullptr, 0, weights64, verdict.data(),
                                               nullptr, nullptr);
        if (rc != BPGPU_OK) throw GpuError(bpgpu_last_error(ctx));
        for (uint8_t v : verdict) out.push_back(v == 0 ? Status::Ok() : Status::Err(static_cast<ProofError>(v)));
        return out;
    }

    // ---- one Transcript per proof (bpgpu_linear_*_ts): each proof runs on its caller's own transcript, bound to whatever session it
    // belongs to, and every transcript is left as create() / verify() leaves it (after an Err: right after innerproduct_domain_sep(n))
    static std::vector<Status> verify_batch(bpgpu_ctx *ctx, std::vector<Transcript> &transcripts, const std::vector<LinearProof> &proofs,
                                            const std::vector<CompressedRistretto> &Cs, const std::vector<CompressedRistretto> &G,
                                            const CompressedRistretto &F, const CompressedRistretto &B,
                                            const std::vector<std::vector<ScalarBytes>> &b_vecs) {
        return verify_ts(ctx, transcripts, proofs, Cs, G, F, B, b_vecs, false, nullptr);
    }
    static std::vector<Status> verify_batch_combined(bpgpu_ctx *ctx, std::vector<Transcript> &transcripts, const std::vector<LinearProof> &proofs,
                                                     const std::vector<CompressedRistretto> &Cs, const std::vector<CompressedRistretto> &G,
                                                     const CompressedRistretto &F, const CompressedRistretto &B,
                                                     const std::vector<std::vector<ScalarBytes>> &b_vecs, const uint8_t *weights64 = nullptr) {
        return verify_ts(ctx, transcripts, proofs, Cs, G, F, B, b_vecs, true, weights64);
    }
    // transcripts.size() proofs in one GPU pass (no counterpart in the crate).  rng_seed32: 32 bytes per proof, proof i's rng being
    // ChaChaRng::from_seed(rng_seed32 + 32 i), its scalars drawn on the device (nullptr: the library draws the seeds).
    static std::vector<LinearProof> create_batch(bpgpu_ctx *ctx, std::vector<Transcript> &transcripts, const std::vector<CompressedRistretto> &Cs,
                                                 const std::vector<ScalarBytes> &rs, const std::vector<std::vector<ScalarBytes>> &a_vecs,
                                                 const std::vector<std::vector<ScalarBytes>> &b_vecs, const std::vector<CompressedRistretto> &G,
                                                 const CompressedRistretto &F, const CompressedRistretto &B, const uint8_t *rng_seed32 = nullptr) {
        const size_t nb = transcripts.size(), n = G.size();
        std::vector<LinearProof> out;
        if (nb == 0) return out;
        if (Cs.size() != nb || rs.size() != nb || a_vecs.size() != nb || b_vecs.size() != nb)
            throw std::invalid_argument("one commitment, blinding, secret and public vector per proof");
        if (n == 0 || (n & (n - 1))) throw std::invalid_argument("InvalidInputLength");
        size_t lg = 0;
        while ((size_t(1) << lg) < n) lg++;
        const size_t pl = 32 * (2 * lg + 3);
        std::vector<uint8_t> ts, cb, rb, ab, bb, pb(nb * pl), status(nb), tso(nb * BPGPU_TRANSCRIPT_BYTES);
        for (size_t i = 0; i < nb; i++) {
            if (a_vecs[i].size() != n || b_vecs[i].size() != n) throw std::invalid_argument("InvalidInputLength");
            ts.insert(ts.end(), transcripts[i].state().begin(), transcripts[i].state().end());
            cb.insert(cb.end(), Cs[i].begin(), Cs[i].end());
            rb.insert(rb.end(), rs[i].begin(), rs[i].end());
            for (const auto &x : a_vecs[i]) ab.insert(ab.end(), x.begin(), x.end());
            for (const auto &x : b_vecs[i]) bb.insert(bb.end(), x.begin(), x.end());
        }
        const int rc = bpgpu_linear_create_batch_ts(ctx, n, nb, ts.data(), BPGPU_TRANSCRIPT_BYTES, rng_seed32, cb.data(), rb.data(), ab.data(), bb.data(), 0,
                                                    G[0].data(), F.data(), B.data(), pb.data(), status.data(), tso.data());
        if (rc != BPGPU_OK) throw GpuError(bpgpu_last_error(ctx));
        for (uint8_t s : status)
            if (s != 0) throw std::invalid_argument("an input point does not decode or a scalar is not canonical");
        for (size_t i = 0; i < nb; i++) {
            std::memcpy(transcripts[i].state_mut().data(), &tso[i * BPGPU_TRANSCRIPT_BYTES], BPGPU_TRANSCRIPT_BYTES);
            LinearProof p;
            p.bytes_.assign(pb.begin() + i * pl, pb.begin() + (i + 1) * pl);
            out.push_back(std::move(p));
        }
        return out;
    }
    // ... and the same three on a TranscriptBatch, left advanced as the vector would be
    static std::vector<Status> verify_batch(bpgpu_ctx *ctx, TranscriptBatch &transcripts, const std::vector<LinearProof> &proofs,
                                            const std::vector<CompressedRistretto> &Cs, const std::vector<CompressedRistretto> &G,
                                            const CompressedRistretto &F, const CompressedRistretto &B,
                                            const std::vector<std::vector<ScalarBytes>> &b_vecs) {
        std::vector<Transcript> ts = transcripts.to_transcripts();
        std::vector<Status> out = verify_ts(ctx, ts, proofs, Cs, G, F, B, b_vecs, false, nullptr);
        transcripts.assign(ts);
        return out;
    }
    static std::vector<Status> verify_batch_combined(bpgpu_ctx *ctx, TranscriptBatch &transcripts, const std::vector<LinearProof> &proofs,
                                                     const std::vector<CompressedRistretto> &Cs, const std::vector<CompressedRistretto> &G,
                                                     const CompressedRistretto &F, const CompressedRistretto &B,
                                                     const std::vector<std::vector<ScalarBytes>> &b_vecs, const uint8_t *weights64 = nullptr) {
        std::vector<Transcript> ts = transcripts.to_transcripts();
        std::vector<Status> out = verify_ts(ctx, ts, proofs, Cs, G, F, B, b_vecs, true, weights64);
        transcripts.assign(ts);
        return out;
    }
    static std::vector<LinearProof> create_batch(bpgpu_ctx *ctx, TranscriptBatch &transcripts, const std::vector<CompressedRistretto> &Cs,
                                                 const std::vector<ScalarBytes> &rs, const std::vector<std::vector<ScalarBytes>> &a_vecs,
                                                 const std::vector<std::vector<ScalarBytes>> &b_vecs, const std::vector<CompressedRistretto> &G,
                                                 const CompressedRistretto &F, const CompressedRistretto &B, const uint8_t *rng_seed32 = nullptr) {
        std::vector<Transcript> ts = transcripts.to_transcripts();
        std::vector<LinearProof> out = create_batch(ctx, ts, Cs, rs, a_vecs, b_vecs, G, F, B, rng_seed32);
        transcripts.assign(ts);
        return out;
    }

  private:
    static std::vector<Status> verify_ts(bpgpu_ctx *ctx, std::vector<Transcript> &transcripts, const std::vector<LinearProof> &proofs,
                                         const std::vector<CompressedRistretto> &Cs, const std::vector<CompressedRistretto> &G,
                                         const CompressedRistretto &F, const CompressedRistretto &B,
                                         const std::vector<std::vector<ScalarBytes>> &b_vecs, bool combined, const uint8_t *weights64) {
        const size_t nb = proofs.size(), n = G.size();
        std::vector<Status> out;
        if (nb == 0) return out;
        if (transcripts.size() != nb || Cs.size() != nb || b_vecs.size() != nb)
            throw std::invalid_argument("one transcript, one commitment and one public vector per proof");
        const size_t pl = proofs[0].bytes_.size();
        std::vector<uint8_t> ts, pb, cb, bb, verdict(nb), tso(nb * BPGPU_TRANSCRIPT_BYTES);
        for (size_t i = 0; i < nb; i++) {
            if (proofs[i].bytes_.size() != pl || b_vecs[i].size() != n) throw std::invalid_argument("proofs of a batch must have one size");
            ts.insert(ts.end(), transcripts[i].state().begin(), transcripts[i].state().end());
            pb.insert(pb.end(), proofs[i].bytes_.begin(), proofs[i].bytes_.end());
            cb.insert(cb.end(), Cs[i].begin(), Cs[i].end());
            for (const auto &x : b_vecs[i]) bb.insert(bb.end(), x.begin(), x.end());
        }
        const uint8_t *g = n ? G[0].data() : nullptr, *b = n ? bb.data() : nullptr;
        const int rc = combined ? bpgpu_linear_verify_rlc_ts(ctx, n, nb, pb.data(), pl, ts.data(), BPGPU_TRANSCRIPT_BYTES, cb.data(), g, F.data(), B.data(), b, 0,
                                                             weights64, verdict.data(), nullptr, tso.data())
                                : bpgpu_linear_verify_batch_ts(ctx, n, nb, pb.data(), pl, ts.data(), BPGPU_TRANSCRIPT_BYTES, cb.data(), g, F.data(), B.data(), b, 0,
                                                               verdict.data(), nullptr, tso.data());
        if (rc != BPGPU_OK) throw GpuError(bpgpu_last_error(ctx));
        for (size_t i = 0; i < nb; i++) {
            std::memcpy(transcripts[i].state_mut().data(), &tso[i * BPGPU_TRANSCRIPT_BYTES], BPGPU_TRANSCRIPT_BYTES);
            out.push_back(verdict[i] == 0 ? Status::Ok() : Status::Err(static_cast<ProofError>(verdict[i])));
        }
        return out;
    }
    std::vector<uint8_t> bytes_;
};

// A proof of knowledge of the opening of a Pedersen commitment C = v B + r B_blinding under the context's bases (no counterpart in the
// crate; the protocol is fixed in bpgpu.h, bpgpu_opening_*).  Two forms: v and r both secret (96 bytes: R | s_v | s_r), or `public_values`
// -- v is known to the verifier, only r is secret (64 bytes: R | s_r); with v = 0 that is a Schnorr signature under the key C, the excess
// proof of a confidential transaction.  Transcripts are one per proof and are left advanced; the TranscriptBatch twins leave the batch so.
class OpeningProof {
  public:
    // raises FormatError for a length other than 64 or 96 or a scalar that is not canonical
    static std::optional<OpeningProof> from_bytes(const uint8_t *b, size_t n, ProofError *err = nullptr) {
        bool ok = n == 64 || n == 96;
        for (size_t off = 32; ok && off < n; off += 32) ok = detail::scalar_is_canonical(b + off);
        if (!ok) {
            if (err) *err = ProofError::FormatError;
            return std::nullopt;
        }
        OpeningProof p;
        p.bytes_.assign(b, b + n);
        return p;
    }
    const std::vector<uint8_t> &to_bytes() const { return bytes_; }
    size_t serialized_size() const { return bytes_.size(); }

    // values.size() proofs in ONE GPU launch (bpgpu_opening_create_batch_ts).  rng_seed32: 32 bytes per proof, proof i's rng being
    // ChaChaRng::from_seed(rng_seed32 + 32 i) (nullptr: the library draws the seeds) -- never one seed for two statements or transcripts.
    // Throws std::invalid_argument for a scalar that is not canonical.
    static std::vector<OpeningProof> create_batch(const BulletproofGens &bp_gens, std::vector<Transcript> &transcripts, const std::vector<uint64_t> &values,
                                                  const std::vector<ScalarBytes> &blindings, const std::vector<CompressedRistretto> &commitments,
                                                  bool public_values = false, const uint8_t *rng_seed32 = nullptr) {
        return create_rows(bp_gens, transcripts, values.data(), 8, values.size(), blindings, commitments, public_values, rng_seed32);
    }
    static std::vector<OpeningProof> create_batch(const BulletproofGens &bp_gens, std::vector<Transcript> &transcripts, const std::vector<ScalarBytes> &values,
                                                  const std::vector<ScalarBytes> &blindings, const std::vector<CompressedRistretto> &commitments,
                                                  bool public_values = false, const uint8_t *rng_seed32 = nullptr) {
        return create_rows(bp_gens, transcripts, values.data(), 32, values.size(), blindings, commitments, public_values, rng_seed32);
    }
    // ... with the commitments made here by bp_gens.commit_batch(values, blindings) -> (proofs, commitments)
    static std::pair<std::vector<OpeningProof>, std::vector<CompressedRistretto>> create_batch(const BulletproofGens &bp_gens, std::vector<Transcript> &transcripts,
                                                                                             const std::vector<uint64_t> &values,
                                                                                             const std::vector<ScalarBytes> &blindings, bool public_values = false,
                                                                                             const uint8_t *rng_seed32 = nullptr) {
        std::vector<CompressedRistretto> coms = bp_gens.commit_batch(values, &blindings).first;
        return {create_batch(bp_gens, transcripts, values, blindings, coms, public_values, rng_seed32), coms};
    }
    // every proof on its own (bpgpu_opening_verify_batch_ts).  public_values == nullptr: proofs with a secret value (96 bytes); else the
    // public values of 64-byte proofs
    static std::vector<Status> verify_batch(const BulletproofGens &bp_gens, std::vector<Transcript> &transcripts, const std::vector<OpeningProof> &proofs,
                                            const std::vector<CompressedRistretto> &commitments, const std::vector<uint64_t> *public_values = nullptr) {
        return verify_rows(bp_gens, transcripts, proofs, commitments, public_values, false, nullptr);
    }
    // the same verdicts through ONE combined check (bpgpu_opening_verify_rlc_ts): one multiscalar multiplication over two points per proof
    // when every proof verifies, per-proof re-verification inside the call when not.  weights64: 64 bytes per proof, unpredictable to the
    // provers, or nullptr (drawn by the library)
    static std::vector<Status> verify_batch_combined(const BulletproofGens &bp_gens, std::vector<Transcript> &transcripts, const std::vector<OpeningProof> &proofs,
                                                     const std::vector<CompressedRistretto> &commitments, const std::vector<uint64_t> *public_values = nullptr,
                                                     const uint8_t *weights64 = nullptr) {
        return verify_rows(bp_gens, transcripts, proofs, commitments, public_values, true, weights64);
    }
    // ... and on a TranscriptBatch, left advanced as the vector would be
    static std::vector<OpeningProof> create_batch(const BulletproofGens &bp_gens, TranscriptBatch &transcripts, const std::vector<uint64_t> &values,
                                                  const std::vector<ScalarBytes> &blindings, const std::vector<CompressedRistretto> &commitments,
                                                  bool public_values = false, const uint8_t *rng_seed32 = nullptr) {
        std::vector<Transcript> ts = transcripts.to_transcripts();
        std::vector<OpeningProof> out = create_batch(bp_gens, ts, values, blindings, commitments, public_values, rng_seed32);
        transcripts.assign(ts);
        return out;
    }
    static std::vector<Status> verify_batch(const BulletproofGens &bp_gens, TranscriptBatch &transcripts, const std::vector<OpeningProof> &proofs,
                                            const std::vector<CompressedRistretto> &commitments, const std::vector<uint64_t> *public_values = nullptr) {
        std::vector<Transcript> ts = transcripts.to_transcripts();
        std::vector<Status> out = verify_rows(bp_gens, ts, proofs, commitments, public_values, false, nullptr);
        transcripts.assign(ts);
        return out;
    }
    static std::vector<Status> verify_batch_combined(const BulletproofGens &bp_gens, TranscriptBatch &transcripts, const std::vector<OpeningProof> &proofs,
                                                     const std::vector<CompressedRistretto> &commitments, const std::vector<uint64_t> *public_values = nullptr,
                                                     const uint8_t *weights64 = nullptr) {
        std::vector<Transcript> ts = transcripts.to_transcripts();
        std::vector<Status> out = verify_rows(bp_gens, ts, proofs, commitments, public_values, true, weights64);
        transcripts.assign(ts);
        return out;
    }
    // one proof; the transcript is left advanced
    static OpeningProof create(const BulletproofGens &bp_gens, Transcript &transcript, uint64_t value, const ScalarBytes &blinding,
                               const CompressedRistretto &commitment, bool public_value = false, const uint8_t *rng_seed32 = nullptr) {
        std::vector<Transcript> ts{transcript};
        OpeningProof p = create_batch(bp_gens, ts, std::vector<uint64_t>{value}, {blinding}, {commitment}, public_value, rng_seed32)[0];
        transcript = ts[0];
        return p;
    }
    Status verify(const BulletproofGens &bp_gens, Transcript &transcript, const CompressedRistretto &commitment, const uint64_t *public_value = nullptr) const {
        std::vector<Transcript> ts{transcript};
        const std::vector<uint64_t> pv{public_value ? *public_value : 0};
        const Status st = verify_rows(bp_gens, ts, {*this}, {commitment}, public_value ? &pv : nullptr, false, nullptr)[0];
        transcript = ts[0];
        return st;
    }

  private:
    static std::vector<uint8_t> states_of(const std::vector<Transcript> &transcripts) {
        std::vector<uint8_t> ts;
        for (const Transcript &t : transcripts) ts.insert(ts.end(), t.state().begin(), t.state().end());
        return ts;
    }
    static std::vector<OpeningProof> create_rows(const BulletproofGens &bp_gens, std::vector<Transcript> &transcripts, const void *values, size_t value_bytes,
                                                 size_t nb, const std::vector<ScalarBytes> &blindings, const std::vector<CompressedRistretto> &commitments,
                                                 bool public_values, const uint8_t *rng_seed32) {
        std::vector<OpeningProof> out;
        if (transcripts.size() != nb || blindings.size() != nb || commitments.size() != nb)
            throw std::invalid_argument("create_batch: one transcript, one blinding and one commitment per value");
        if (nb == 0) return out;
        const size_t pl = public_values ? 64 : 96;
        const std::vector<uint8_t> ts = states_of(transcripts);
        std::vector<uint8_t> pb(nb * pl), status(nb), tso(nb * BPGPU_TRANSCRIPT_BYTES);
        const int rc = bpgpu_opening_create_batch_ts(bp_gens.ctx(), public_values ? BPGPU_OPENING_BLINDING : BPGPU_OPENING_FULL, nb, ts.data(), BPGPU_TRANSCRIPT_BYTES,
                                                     rng_seed32, commitments[0].data(), values, value_bytes, blindings[0].data(), pb.data(), status.data(), tso.data());
        if (rc != BPGPU_OK) throw GpuError(bpgpu_last_error(bp_gens.ctx()));
        for (uint8_t s : status)
            if (s != 0) throw std::invalid_argument("create_batch: scalars must be canonical");
        for (size_t i = 0; i < nb; i++) {
            std::memcpy(transcripts[i].state_mut().data(), &tso[i * BPGPU_TRANSCRIPT_BYTES], BPGPU_TRANSCRIPT_BYTES);
            OpeningProof p;
            p.bytes_.assign(pb.begin() + i * pl, pb.begin() + (i + 1) * pl);
            out.push_back(std::move(p));
        }
        return out;
    }
    static std::vector<Status> verify_rows(const BulletproofGens &bp_gens, std::vector<Transcript> &transcripts, const std::vector<OpeningProof> &proofs,
                                           const std::vector<CompressedRistretto> &commitments, const std::vector<uint64_t> *public_values, bool combined,
                                           const uint8_t *weights64) {
        const size_t nb = proofs.size(), pl = public_values ? 64 : 96;
        std::vector<Status> out;
        if (transcripts.size() != nb || commitments.size() != nb || (public_values && public_values->size() != nb))
            throw std::invalid_argument("one transcript, one commitment and one public value per proof");
        if (nb == 0) return out;
        const std::vector<uint8_t> ts = states_of(transcripts);
        std::vector<uint8_t> pb, verdict(nb), tso(nb * BPGPU_TRANSCRIPT_BYTES);
        for (const OpeningProof &p : proofs) {
            if (p.bytes_.size() != pl) throw std::invalid_argument("every proof of a call has one form");
            pb.insert(pb.end(), p.bytes_.begin(), p.bytes_.end());
        }
        const int form = public_values ? BPGPU_OPENING_BLINDING : BPGPU_OPENING_FULL;
        const void *pv = public_values ? public_values->data() : nullptr;
        bpgpu_ctx *ctx = bp_gens.ctx();
        const int rc = combined ? bpgpu_opening_verify_rlc_ts(ctx, form, nb, pb.data(), pl, ts.data(), BPGPU_TRANSCRIPT_BYTES, commitments[0].data(), pv, 8, weights64,
                                                              verdict.data(), nullptr, tso.data())
                                : bpgpu_opening_verify_batch_ts(ctx, form, nb, pb.data(), pl, ts.data(), BPGPU_TRANSCRIPT_BYTES, commitments[0].data(), pv, 8,
                                                                verdict.data(), nullptr, tso.data());
        if (rc != BPGPU_OK) throw GpuError(bpgpu_last_error(ctx));
        for (size_t i = 0; i < nb; i++) {
            std::memcpy(transcripts[i].state_mut().data(), &tso[i * BPGPU_TRANSCRIPT_BYTES], BPGPU_TRANSCRIPT_BYTES);
            out.push_back(verdict[i] == 0 ? Status::Ok() : Status::Err(static_cast<ProofError>(verdict[i])));
        }
        return out;
    }
    std::vector<uint8_t> bytes_;
};

namespace detail {
// l - fee as a canonical 32-byte scalar
inline ScalarBytes neg_fee(uint64_t fee) {
    static const uint8_t L[32] = {0xed, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                                  0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0,    0x10};
    ScalarBytes out{};
    if (fee == 0) return out;
    int borrow = 0;
    for (int i = 0; i < 32; i++) {
        const int f = i < 8 ? static_cast<int>((fee >> (8 * i)) & 0xff) : 0, d = L[i] - f - borrow;
        out[i] = static_cast<uint8_t>(d & 0xff);
        borrow = d < 0;
    }
    return out;
}
}  // namespace detail

inline std::vector<OpeningProof> BulletproofGens::prove_balance(const std::vector<uint64_t> &fees, const std::vector<ScalarBytes> &excess_blindings,
                                                                std::vector<Transcript> &transcripts, const Rows &inputs, const Rows &outputs,
                                                                const uint8_t *rng_seed32) const {
    std::vector<ScalarBytes> neg;
    for (uint64_t f : fees) neg.push_back(detail::neg_fee(f));
    std::vector<CompressedRistretto> E;
    for (const auto &e : sum_commitments(inputs, &outputs, neg)) {
        if (!e) throw std::invalid_argument("prove_balance: a commitment does not decode");
        E.push_back(*e);
    }
    return OpeningProof::create_batch(*this, transcripts, std::vector<uint64_t>(fees.size(), 0), excess_blindings, E, true, rng_seed32);
}
inline std::vector<Status> BulletproofGens::verify_balance_proved(const Rows &inputs, const Rows &outputs, const std::vector<uint64_t> &fees,
                                                                  const std::vector<OpeningProof> &proofs, std::vector<Transcript> &transcripts) const {
    std::vector<ScalarBytes> neg;
    for (uint64_t f : fees) neg.push_back(detail::neg_fee(f));
    const auto sums = sum_commitments(inputs, &outputs, neg);
    std::vector<CompressedRistretto> E;
    for (const auto &e : sums) E.push_back(e ? *e : CompressedRistretto{});
    const std::vector<uint64_t> zeros(fees.size(), 0);
    std::vector<Status> out = OpeningProof::verify_batch_combined(*this, transcripts, proofs, E, &zeros);
    // a row whose sum did not decode has no key: never verified, whatever its proof says about the placeholder
    for (size_t i = 0; i < out.size(); i++)
        if (!sums[i]) out[i] = Status::Err(ProofError::VerificationError);
    return out;
}

// A linear relation between points, written once (no counterpart in the crate; the `zkp` crate's pattern next to it; the protocol is fixed
// in include/bpgpu.h, bpgpu_sigma_*): secrets, instance points and equations  point = sum secret * base , where a base is B, B_blinding or
// G(i) of bp_gens or another instance point.  compile() records it on the GPU context and returns the SigmaRelation that proves and
// verifies batches.
//     SigmaStatement st(gens); auto x = st.secret(); auto A = st.point(), H = st.point(), Bp = st.point();
//     st.equation(A, {{x, st.B}}); st.equation(H, {{x, Bp}}); SigmaRelation dleq = st.compile();
// At most 8 secrets, 8 points, 8 equations of 8 terms, 32 terms in all.  Public scalar coefficients are not part of a relation: fold them
// into an instance point first (BulletproofGens::sum_commitments).
// Canonical descriptor bytes: u8 S, u8 P, u8 E, then per equation u8 lhs, u8 nterms, then nterms x (u8 secret, u8 base); base ids
// 0 = B_blinding, 1 = B, 2 + i = G_i, 16 + p = instance point p.
// Transcript, on the caller's own state: append_message(b"dom-sep", b"sigmaproof v1"); append_message(b"stmt", digest);
// append_point(b"P", P_i) in slot order; validate_and_append_point(b"T", T_k), k = 1 .. E; c = challenge_scalar(b"c").
// A proof is T_1 | .. | T_E | s_1 | .. | s_S, 32 (E + S) bytes, s_j = k_j + c x_j.
class SigmaRelation;
class SigmaStatement {
  public:
    struct Secret {
        uint8_t index;
    };
    struct Base {
        uint8_t id;
    };
    const Base B_blinding{0}, B{1};
    explicit SigmaStatement(const BulletproofGens &bp_gens) : gens_(bp_gens) {}
    Secret secret() { return Secret{static_cast<uint8_t>(S_++)}; }
    Base point() { return Base{static_cast<uint8_t>(16 + P_++)}; }
    Base G(size_t i) const {
        if (i >= 8) throw std::invalid_argument("G(i): i in 0 .. 7");
        return Base{static_cast<uint8_t>(2 + i)};
    }
    void equation(Base lhs, const std::vector<std::pair<Secret, Base>> &terms) {
        if (lhs.id < 16) throw std::invalid_argument("the left-hand side is an instance point (from point())");
        eqs_.push_back({lhs.id, terms});
    }
    // the canonical bytes of include/bpgpu.h
    std::vector<uint8_t> descriptor() const {
        if (S_ > 255 || P_ > 239 || eqs_.size() > 255) throw std::invalid_argument("a relation has at most 8 secrets, 8 points and 8 equations of 8 terms");
        std::vector<uint8_t> d{static_cast<uint8_t>(S_), static_cast<uint8_t>(P_), static_cast<uint8_t>(eqs_.size())};
        for (const auto &e : eqs_) {
            if (e.second.size() > 255) throw std::invalid_argument("a relation has at most 8 terms per equation");
            d.push_back(e.first);
            d.push_back(static_cast<uint8_t>(e.second.size()));
            for (const auto &t : e.second) {
                d.push_back(t.first.index);
                d.push_back(t.second.id);
            }
        }
        return d;
    }
    // throws std::invalid_argument for what bpgpu_sigma_relation_create refuses (a count out of range, an unused secret or point, a G(i)
    // beyond the generators)
    inline SigmaRelation compile() const;

  private:
    BulletproofGens gens_;
    size_t S_ = 0, P_ = 0;
    std::vector<std::pair<uint8_t, std::vector<std::pair<Secret, Base>>>> eqs_;
};

// A recorded relation (SigmaStatement::compile, or canonical descriptor bytes).  secrets: per row S scalars; points: per row P encodings,
// slot order.  Transcripts: one per proof, each left advanced; a TranscriptBatch is left advanced as the vector would be.
class SigmaRelation {
  public:
    using Proof = std::vector<uint8_t>;
    using SecretRows = std::vector<std::vector<ScalarBytes>>;
    using PointRows = std::vector<std::vector<CompressedRistretto>>;
    SigmaRelation(const BulletproofGens &bp_gens, const std::vector<uint8_t> &descriptor) : gens_(bp_gens), descriptor_(descriptor) {
        bpgpu_sigma_relation *r = nullptr;
        const int rc = bpgpu_sigma_relation_create(gens_.ctx(), descriptor_.data(), descriptor_.size(), &r);
        if (rc == BPGPU_ERR_INVALID_ARG) throw std::invalid_argument(bpgpu_last_error(gens_.ctx()));
        if (rc != BPGPU_OK) throw GpuError(bpgpu_last_error(gens_.ctx()));
        rel_.reset(r, bpgpu_sigma_relation_destroy);
        bpgpu_sigma_relation_shape(r, &S_, &P_, &E_, digest_.data());
    }
    size_t secrets() const { return S_; }
    size_t points() const { return P_; }
    size_t equations() const { return E_; }
    size_t proof_len() const { return 32 * (E_ + S_); }
    const std::array<uint8_t, 32> &digest() const { return digest_; }
    const std::vector<uint8_t> &descriptor() const { return descriptor_; }

    // points.size() proofs (bpgpu_sigma_create_batch_ts).  rng_seed32: 32 bytes per row, row i's rng being ChaChaRng::from_seed(rng_seed32 + 32 i)
    // (nullptr: the library draws the seeds) -- never one seed for two statements or transcripts.  Throws std::invalid_argument for a
    // secret that is not canonical or an instance base that does not decode.
    std::vector<Proof> create_batch(std::vector<Transcript> &transcripts, const SecretRows &secrets, const PointRows &points, const uint8_t *rng_seed32 = nullptr) const {
        const size_t nb = points.size();
        if (transcripts.size() != nb || secrets.size() != nb) throw std::invalid_argument("create_batch: one transcript and one row of secrets per row of points");
        std::vector<Proof> out;
        if (nb == 0) return out;
        const std::vector<uint8_t> ts = states_of(transcripts), pts = pack(points, P_, "points"), xs = pack(secrets, S_, "secrets");
        const size_t pl = proof_len();
        std::vector<uint8_t> pb(nb * pl), status(nb), tso(nb * BPGPU_TRANSCRIPT_BYTES);
        const int rc = bpgpu_sigma_create_batch_ts(gens_.ctx(), rel_.get(), nb, ts.data(), BPGPU_TRANSCRIPT_BYTES, rng_seed32, pts.data(), xs.data(), pb.data(),
                                                   status.data(), tso.data());
        if (rc != BPGPU_OK) throw GpuError(bpgpu_last_error(gens_.ctx()));
        for (uint8_t s : status)
            if (s != 0) throw std::invalid_argument(s == 2 ? "create_batch: secrets must be canonical" : "create_batch: an instance base does not decode");
        for (size_t i = 0; i < nb; i++) {
            std::memcpy(transcripts[i].state_mut().data(), &tso[i * BPGPU_TRANSCRIPT_BYTES], BPGPU_TRANSCRIPT_BYTES);
            out.emplace_back(pb.begin() + i * pl, pb.begin() + (i + 1) * pl);
        }
        return out;
    }
    // every proof on its own (bpgpu_sigma_verify_batch_ts)
    std::vector<Status> verify_batch(std::vector<Transcript> &transcripts, const std::vector<Proof> &proofs, const PointRows &points) const {
        return verify_rows(transcripts, proofs, points, false, nullptr);
    }
    // the same verdicts through ONE combined check (bpgpu_sigma_verify_rlc_ts): one multiscalar multiplication over P + E points per proof
    // when every proof verifies, per-proof re-verification inside the call when not.  weights64: 64 bytes per (proof, equation),
    // unpredictable to the provers, or nullptr (drawn by the library)
    std::vector<Status> verify_batch_combined(std::vector<Transcript> &transcripts, const std::vector<Proof> &proofs, const PointRows &points,
                                              const uint8_t *weights64 = nullptr) const {
        return verify_rows(transcripts, proofs, points, true, weights64);
    }
    std::vector<Proof> create_batch(TranscriptBatch &transcripts, const SecretRows &secrets, const PointRows &points, const uint8_t *rng_seed32 = nullptr) const {
        std::vector<Transcript> ts = transcripts.to_transcripts();
        std::vector<Proof> out = create_batch(ts, secrets, points, rng_seed32);
        transcripts.assign(ts);
        return out;
    }
    std::vector<Status> verify_batch(TranscriptBatch &transcripts, const std::vector<Proof> &proofs, const PointRows &points) const {
        std::vector<Transcript> ts = transcripts.to_transcripts();
        std::vector<Status> out = verify_rows(ts, proofs, points, false, nullptr);
        transcripts.assign(ts);
        return out;
    }
    std::vector<Status> verify_batch_combined(TranscriptBatch &transcripts, const std::vector<Proof> &proofs, const PointRows &points,
                                              const uint8_t *weights64 = nullptr) const {
        std::vector<Transcript> ts = transcripts.to_transcripts();
        std::vector<Status> out = verify_rows(ts, proofs, points, true, weights64);
        transcripts.assign(ts);
        return out;
    }
    // one proof; the transcript is left advanced
    Proof create(Transcript &transcript, const std::vector<ScalarBytes> &secrets, const std::vector<CompressedRistretto> &points, const uint8_t *rng_seed32 = nullptr) const {
        std::vector<Transcript> ts{transcript};
        Proof p = create_batch(ts, SecretRows{secrets}, PointRows{points}, rng_seed32)[0];
        transcript = ts[0];
        return p;
    }
    Status verify(Transcript &transcript, const Proof &proof, const std::vector<CompressedRistretto> &points) const {
        std::vector<Transcript> ts{transcript};
        const Status st = verify_rows(ts, {proof}, PointRows{points}, false, nullptr)[0];
        transcript = ts[0];
        return st;
    }

  private:
    static std::vector<uint8_t> states_of(const std::vector<Transcript> &transcripts) {
        std::vector<uint8_t> ts;
        for (const Transcript &t : transcripts) ts.insert(ts.end(), t.state().begin(), t.state().end());
        return ts;
    }
    template <class T>
    static std::vector<uint8_t> pack(const std::vector<std::vector<T>> &rows, size_t per_row, const char *what) {
        std::vector<uint8_t> out;
        for (const auto &row : rows) {
            if (row.size() != per_row) throw std::invalid_argument(std::string("wrong number of ") + what + " in a row");
            for (const T &x : row) out.insert(out.end(), x.begin(), x.end());
        }
        return out;
    }
    std::vector<Status> verify_rows(std::vector<Transcript> &transcripts, const std::vector<Proof> &proofs, const PointRows &points, bool combined,
                                    const uint8_t *weights64) const {
        const size_t nb = proofs.size(), pl = proof_len();
        std::vector<Status> out;
        if (transcripts.size() != nb || points.size() != nb) throw std::invalid_argument("one transcript and one row of points per proof");
        if (nb == 0) return out;
        const std::vector<uint8_t> ts = states_of(transcripts), pts = pack(points, P_, "points");
        std::vector<uint8_t> pb, verdict(nb), tso(nb * BPGPU_TRANSCRIPT_BYTES);
        for (const Proof &p : proofs) {
            if (p.size() != pl) throw std::invalid_argument("a proof of this relation has 32 (E + S) bytes");
            pb.insert(pb.end(), p.begin(), p.end());
        }
        bpgpu_ctx *ctx = gens_.ctx();
        const int rc = combined ? bpgpu_sigma_verify_rlc_ts(ctx, rel_.get(), nb, pb.data(), pl, ts.data(), BPGPU_TRANSCRIPT_BYTES, pts.data(), weights64, verdict.data(),
                                                            nullptr, tso.data())
                                : bpgpu_sigma_verify_batch_ts(ctx, rel_.get(), nb, pb.data(), pl, ts.data(), BPGPU_TRANSCRIPT_BYTES, pts.data(), verdict.data(), nullptr,
                                                              tso.data());
        if (rc != BPGPU_OK) throw GpuError(bpgpu_last_error(ctx));
        for (size_t i = 0; i < nb; i++) {
            std::memcpy(transcripts[i].state_mut().data(), &tso[i * BPGPU_TRANSCRIPT_BYTES], BPGPU_TRANSCRIPT_BYTES);
            out.push_back(verdict[i] == 0 ? Status::Ok() : Status::Err(static_cast<ProofError>(verdict[i])));
        }
        return out;
    }
    BulletproofGens gens_;   // (a copy: it shares the context and keeps it alive as long as the relation)
    std::vector<uint8_t> descriptor_;
    std::shared_ptr<bpgpu_sigma_relation> rel_;
    size_t S_ = 0, P_ = 0, E_ = 0;
    std::array<uint8_t, 32> digest_{};
};
inline SigmaRelation SigmaStatement::compile() const { return SigmaRelation(gens_, descriptor()); }

}  // namespace bulletproofs
#endif
