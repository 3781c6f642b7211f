// include/bulletproofs.hpp: RangeProof::prove_batch_rewindable / rewind_batch / rewind_single / rewind_seeds
// (bpgpu_rangeproof_prove_batch_rw, bpgpu_rangeproof_rewind_batch): a wallet proves its outputs, a validator verifies them, the wallet
// -- and nobody else -- gets value, blinding and message back out of (proof, commitment).  Runs on the GPU.
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

static std::vector<Transcript> sessions(size_t n, const char *label) {
    std::vector<Transcript> ts;
    for (size_t i = 0; i < n; i++) {
        Transcript t(label);
        t.append_u64("block", 7000 + i / 3);
        ts.push_back(t);
    }
    return ts;
}

int main() {
    BulletproofGens gens(64, 1);
    const PedersenGens pc = gens.pedersen();
    const size_t nb = 70, n = 64;   // more than one workgroup of 64 lanes
    std::vector<uint64_t> values;
    std::vector<ScalarBytes> blindings;
    std::vector<std::array<uint8_t, 16>> messages(nb);
    uint8_t key[32], other_key[32];
    for (int q = 0; q < 32; q++) key[q] = static_cast<uint8_t>(7 * q + 1), other_key[q] = static_cast<uint8_t>(5 * q + 2);
    for (size_t i = 0; i < nb; i++) {
        values.push_back(i == 0 ? 0 : i == 1 ? ~0ull : i == 2 ? 1ull << 63 : i * i * 1000003ull + 1);
        ScalarBytes b{};
        if (i) for (int q = 0; q < 31; q++) b[q] = static_cast<uint8_t>(29 * i + 5 * q + 1);
        blindings.push_back(b);
        for (int q = 0; q < 16; q++) messages[i][q] = static_cast<uint8_t>(i == 1 ? 0xff : i % 3 == 0 ? 0 : 11 * i + q);
    }
    // the wallet: commitments first (the seeds are derived from them), then the proofs
    const std::vector<CompressedRistretto> coms = gens.commit_batch(values, &blindings).first;
    const std::vector<uint8_t> seeds = RangeProof::rewind_seeds(gens.ctx(), key, coms), strangers = RangeProof::rewind_seeds(gens.ctx(), other_key, coms);
    CHECK(seeds.size() == 32 * nb && seeds != strangers && std::memcmp(&seeds[0], &seeds[32], 32) != 0);
    std::vector<Transcript> tp = sessions(nb, "rewind client");
    const auto made = RangeProof::prove_batch_rewindable(gens, pc, tp, values, blindings, n, seeds.data(), messages);
    std::vector<std::vector<uint8_t>> proofs;
    for (size_t i = 0; i < nb; i++) {
        CHECK(made[i].second == coms[i]);
        proofs.push_back(made[i].first.to_bytes());
    }
    // the validator: ordinary proofs
    for (size_t i = 0; i < nb; i += 23) CHECK(made[i].first.verify_single(gens, pc, sessions(nb, "rewind client")[i], coms[i], n).is_ok());
    // the wallet rewinds the block; a stranger's key finds nothing
    const auto mine = RangeProof::rewind_batch(gens, pc, sessions(nb, "rewind client"), proofs, coms, n, seeds.data());
    CHECK(mine.index() == 0);
    for (size_t i = 0; i < nb; i++) {
        const auto &r = std::get<0>(mine)[i];
        CHECK(r.has_value() && r->value == values[i] && r->blinding == blindings[i] && r->message == messages[i]);
    }
    const auto theirs = RangeProof::rewind_batch(gens, pc, sessions(nb, "rewind client"), proofs, coms, n, strangers.data());
    CHECK(theirs.index() == 0);
    for (const auto &r : std::get<0>(theirs)) CHECK(!r.has_value());
    // one row under another session, one tampered e_blinding, one row of somebody else's: missed alone
    std::vector<Transcript> ts = sessions(nb, "rewind client");
    ts[9] = ts[12];
    std::vector<std::vector<uint8_t>> bad = proofs;
    bad[64][192] ^= 1;
    std::vector<uint8_t> mixed = seeds;
    std::memcpy(&mixed[32 * 5], &strangers[32 * 5], 32);
    const auto some = RangeProof::rewind_batch(gens, pc, ts, bad, coms, n, mixed.data());
    CHECK(some.index() == 0);
    for (size_t i = 0; i < nb; i++) CHECK(std::get<0>(some)[i].has_value() == !(i == 9 || i == 64 || i == 5));
    // a scalar that is not canonical: FormatError, as from_bytes
    bad = proofs;
    std::memset(&bad[3][192], 0xff, 32);
    CHECK(std::holds_alternative<ProofError>(RangeProof::from_bytes(bad[3])));
    const auto fmt = RangeProof::rewind_batch(gens, pc, sessions(nb, "rewind client"), bad, coms, n, seeds.data());
    CHECK(fmt.index() == 1 && std::get<1>(fmt) == ProofError::FormatError);
    // one proof, one shared transcript, no messages
    Transcript one("single rewind");
    std::vector<Transcript> shared = {one};
    const auto two = RangeProof::prove_batch_rewindable(gens, pc, shared, {values[4], values[5]}, {blindings[4], blindings[5]}, n, &seeds[32 * 4]);
    const auto r4 = two[0].first.rewind_single(gens, pc, one, coms[4], n, &seeds[32 * 4]);
    const std::array<uint8_t, 16> no_message{};
    CHECK(r4.index() == 0 && std::get<0>(r4).has_value() && std::get<0>(r4)->value == values[4] && std::get<0>(r4)->message == no_message);
    const auto r5 = two[1].first.rewind_single(gens, pc, one, coms[5], n, &seeds[32 * 4]);
    CHECK(r5.index() == 0 && !std::get<0>(r5).has_value());
    bool threw = false;
    try {
        RangeProof::prove_batch_rewindable(gens, pc, shared, {values[4]}, {blindings[4]}, n, nullptr);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    CHECK(threw);
    std::printf("range_proof_rewind_test ok\n");
    return 0;
}
