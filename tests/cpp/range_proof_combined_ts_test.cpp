// RangeProof::verify_batch_combined of include/bulletproofs.hpp on PRE-BOUND transcripts: a transcript that already absorbed the
// application's messages is routed to bpgpu_rangeproof_verify_rlc_ts instead of being refused, and the overload with one Transcript per
// proof takes transcripts at differing positions.  Proofs are made on the GPU by the same mirror (prove_multiple_with_rng).
#include <cstdio>
#include <string>

#include "bulletproofs.hpp"

using namespace bulletproofs;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

static Transcript bound(size_t i, bool own_position) {
    Transcript t("payment-protocol v3");
    const std::string session = "session-" + std::to_string(i);
    t.append_message("session", reinterpret_cast<const uint8_t *>(session.data()), session.size());
    const std::string pad(own_position ? 3 + 5 * i : 3, 'x');
    t.append_message("context", reinterpret_cast<const uint8_t *>(pad.data()), pad.size());
    return t;
}

int main() {
    BulletproofGens bp_gens(16, 2);
    PedersenGens pc_gens = bp_gens.pedersen();
    const size_t nb = 5, n = 16;
    // one shared bound transcript
    {
        const Transcript shared = bound(0, false);
        CHECK(!shared.is_fresh());
        std::vector<std::vector<uint8_t>> proofs;
        std::vector<std::vector<CompressedRistretto>> coms;
        for (size_t i = 0; i < nb; i++) {
            Transcript pt = shared;
            ScalarBytes b0{}, b1{};
            b0[0] = (uint8_t)(1 + i), b1[0] = (uint8_t)(9 + i);
            auto made = RangeProof::prove_multiple_with_rng(bp_gens, pc_gens, pt, {1000 + i, 65535 - i}, {b0, b1}, n);
            proofs.push_back(made.first.to_bytes());
            coms.push_back(made.second);
        }
        auto ok = RangeProof::verify_batch_combined(bp_gens, pc_gens, shared, proofs, coms, n);
        for (size_t i = 0; i < nb; i++) CHECK(ok[i] == Status::Ok());
        proofs[3][130] ^= 1;
        auto res = RangeProof::verify_batch_combined(bp_gens, pc_gens, shared, proofs, coms, n);
        auto ref = RangeProof::verify_batch(bp_gens, pc_gens, shared, proofs, coms, n);
        for (size_t i = 0; i < nb; i++) CHECK(res[i] == ref[i] && res[i] == (i == 3 ? Status::Err(ProofError::VerificationError) : Status::Ok()));
        // the same proofs on another history: every one fails
        auto other = RangeProof::verify_batch_combined(bp_gens, pc_gens, bound(1, false), proofs, coms, n);
        for (size_t i = 0; i < nb; i++) CHECK(other[i] == Status::Err(ProofError::VerificationError));
    }
    // one transcript per proof, at differing positions
    {
        std::vector<Transcript> ts;
        std::vector<std::vector<uint8_t>> proofs;
        std::vector<std::vector<CompressedRistretto>> coms;
        for (size_t i = 0; i < nb; i++) {
            ts.push_back(bound(i, true));
            Transcript pt = ts.back();
            ScalarBytes b0{}, b1{};
            b0[0] = (uint8_t)(21 + i), b1[0] = (uint8_t)(31 + i);
            auto made = RangeProof::prove_multiple_with_rng(bp_gens, pc_gens, pt, {7 + i, 40000 + i}, {b0, b1}, n);
            proofs.push_back(made.first.to_bytes());
            coms.push_back(made.second);
        }
        CHECK(ts[0].state()[200] != ts[1].state()[200]);
        const auto before = ts[2].state();
        auto ok = RangeProof::verify_batch_combined(bp_gens, pc_gens, ts, proofs, coms, n);
        for (size_t i = 0; i < nb; i++) CHECK(ok[i] == Status::Ok());
        CHECK(ts[2].state() == before);   // the caller's transcripts are not advanced
        std::swap(ts[0], ts[4]);           // right proofs, wrong histories
        std::memset(&proofs[2][128], 0xff, 32);
        auto res = RangeProof::verify_batch_combined(bp_gens, pc_gens, ts, proofs, coms, n);
        CHECK(res[0] == Status::Err(ProofError::VerificationError) && res[4] == Status::Err(ProofError::VerificationError));
        CHECK(res[1] == Status::Ok() && res[3] == Status::Ok() && res[2] == Status::Err(ProofError::FormatError));
    }
    std::printf("range_proof_combined_ts: ok\n");
    return 0;
}
