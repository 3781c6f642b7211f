// include/bulletproofs.hpp: OpeningProof (bpgpu_opening_*) and BulletproofGens::prove_balance / verify_balance_proved -- proofs of
// knowledge of commitment openings in both forms, per proof and combined, on vectors of transcripts and on a TranscriptBatch.
// Runs on the GPU.
#include <cstdio>
#include <cstring>
#include <vector>

#include "bulletproofs.hpp"

using namespace bulletproofs;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

// a + b, a - b for scalars below 2^248 with a >= b (no reduction needed)
static ScalarBytes add_small(const ScalarBytes &a, const ScalarBytes &b, bool subtract = false) {
    ScalarBytes s{};
    int carry = 0;
    for (int i = 0; i < 32; i++) {
        const int t = subtract ? a[i] - b[i] - carry : a[i] + b[i] + carry;
        s[i] = static_cast<uint8_t>(t & 0xff);
        carry = subtract ? t < 0 : t >> 8;
    }
    return s;
}

static std::vector<Transcript> sessions(size_t n, const char *label) {
    std::vector<Transcript> ts;
    for (size_t i = 0; i < n; i++) {
        Transcript t(label);
        t.append_u64("session", 1000 + i);
        ts.push_back(t);
    }
    return ts;
}

int main() {
    BulletproofGens gens(8, 1);
    const size_t n = 70;   // more than one workgroup of 64 lanes
    std::vector<uint64_t> values;
    std::vector<ScalarBytes> blindings;
    std::vector<uint8_t> seeds(32 * n);
    for (size_t i = 0; i < n; i++) {
        values.push_back(i * i + 1);
        ScalarBytes b{};
        for (int q = 0; q < 30; q++) b[q] = static_cast<uint8_t>(29 * i + 5 * q + 1);
        blindings.push_back(b);
        for (int q = 0; q < 32; q++) seeds[32 * i + q] = static_cast<uint8_t>(i + 3 * q + 11);
    }
    for (int pub = 0; pub < 2; pub++) {
        std::vector<Transcript> tp = sessions(n, "opening client");
        auto made = OpeningProof::create_batch(gens, tp, values, blindings, pub != 0, seeds.data());
        const std::vector<OpeningProof> &proofs = made.first;
        const std::vector<CompressedRistretto> &coms = made.second;
        CHECK(proofs.size() == n && proofs[0].serialized_size() == (pub ? 64u : 96u));
        CHECK(OpeningProof::from_bytes(proofs[3].to_bytes().data(), proofs[3].serialized_size()).has_value());
        std::vector<Transcript> tv = sessions(n, "opening client"), tc = sessions(n, "opening client");
        const std::vector<uint64_t> *pv = pub ? &values : nullptr;
        for (const Status &s : OpeningProof::verify_batch(gens, tv, proofs, coms, pv)) CHECK(s.is_ok());
        for (const Status &s : OpeningProof::verify_batch_combined(gens, tc, proofs, coms, pv)) CHECK(s.is_ok());
        for (size_t i = 0; i < n; i++) CHECK(tv[i].state() == tp[i].state() && tc[i].state() == tp[i].state());   // both sides end in one state
        // one tampered proof, one proof under the wrong session, one wrong public value: rejected alone, by both calls alike
        std::vector<OpeningProof> bad = proofs;
        std::vector<uint8_t> raw = bad[64].to_bytes();
        raw[40] ^= 1;
        bad[64] = *OpeningProof::from_bytes(raw.data(), raw.size());
        std::vector<uint64_t> bad_v = values;
        if (pub) bad_v[5] += 1;
        std::vector<Transcript> t1 = sessions(n, "opening client"), t2 = sessions(n, "opening client");
        t1[9] = t1[10], t2[9] = t2[10];
        const std::vector<Status> a = OpeningProof::verify_batch(gens, t1, bad, coms, pub ? &bad_v : nullptr);
        const std::vector<Status> b = OpeningProof::verify_batch_combined(gens, t2, bad, coms, pub ? &bad_v : nullptr);
        for (size_t i = 0; i < n; i++) {
            const bool wrong = i == 64 || i == 9 || (pub && i == 5);
            CHECK(a[i] == b[i] && a[i].is_ok() == !wrong);
            if (wrong) CHECK(a[i] == Status::Err(ProofError::VerificationError));
            CHECK(t1[i].state() == t2[i].state());
        }
        // a TranscriptBatch in place of the vector, left advanced the same way
        TranscriptBatch tb(gens.ctx(), "opening client", n);
        std::vector<uint64_t> ids;
        for (size_t i = 0; i < n; i++) ids.push_back(1000 + i);
        tb.append_u64("session", ids);
        for (const Status &s : OpeningProof::verify_batch_combined(gens, tb, proofs, coms, pv)) CHECK(s.is_ok());
        CHECK(tb[7].state() == tp[7].state());
        // one proof
        Transcript one("single"), other("single");
        const OpeningProof p1 = OpeningProof::create(gens, one, values[2], blindings[2], coms[2], pub != 0, seeds.data());
        CHECK(p1.verify(gens, other, coms[2], pub ? &values[2] : nullptr).is_ok() && one.state() == other.state());
        Transcript wrong_label("double");
        CHECK(p1.verify(gens, wrong_label, coms[2], pub ? &values[2] : nullptr) == Status::Err(ProofError::VerificationError));
    }
    ProofError e = ProofError::VerificationError;
    std::vector<uint8_t> junk(64, 0xff);
    CHECK(!OpeningProof::from_bytes(junk.data(), 64, &e).has_value() && e == ProofError::FormatError);
    CHECK(!OpeningProof::from_bytes(junk.data(), 63).has_value());
    bool threw = false;
    try {
        std::vector<Transcript> t = sessions(1, "x");
        ScalarBytes big;
        big.fill(0xff);
        OpeningProof::create_batch(gens, t, std::vector<uint64_t>{1}, {big}, {CompressedRistretto{}});
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    CHECK(threw);
    // a block of 2-in 2-out transactions with fees 0 and 2^64 - 1: excess blinding = r_in0 + r_in1 - r_out0 - r_out1, value balance = fee
    {
        const uint64_t fee[2] = {0, ~0ull};
        BulletproofGens::Rows inputs, outputs;
        std::vector<ScalarBytes> excess;
        for (int r = 0; r < 2; r++) {
            // inputs carry (fee/2 + 5 + fee%2, 7), outputs (5, 7): the difference is the fee
            std::vector<uint64_t> v = {fee[r] / 2 + 5 + fee[r] % 2, fee[r] / 2 + 7, 5, 7};
            std::vector<ScalarBytes> bl(4);
            for (int k = 0; k < 4; k++)
                for (int q = 0; q < 29; q++) bl[k][q] = static_cast<uint8_t>((k < 2 ? 200 : 3) + 17 * r + q + k);
            const std::vector<CompressedRistretto> c = gens.commit_batch(v, &bl).first;
            inputs.push_back({c[0], c[1]});
            outputs.push_back({c[2], c[3]});
            excess.push_back(add_small(add_small(add_small(bl[0], bl[1]), bl[2], true), bl[3], true));
        }
        const std::vector<uint64_t> fees(fee, fee + 2);
        std::vector<Transcript> tp = sessions(2, "block"), tv = sessions(2, "block"), tw = sessions(2, "block");
        const std::vector<OpeningProof> proofs = gens.prove_balance(fees, excess, tp, inputs, outputs);
        for (const Status &s : gens.verify_balance_proved(inputs, outputs, fees, proofs, tv)) CHECK(s.is_ok());
        CHECK(tv[1].state() == tp[1].state());
        const std::vector<uint64_t> off_by_one = {0, ~0ull - 1};
        const std::vector<Status> vd = gens.verify_balance_proved(inputs, outputs, off_by_one, proofs, tw);
        CHECK(vd[0].is_ok() && vd[1] == Status::Err(ProofError::VerificationError));
    }
    std::printf("opening_proof_test ok\n");
    return 0;
}
