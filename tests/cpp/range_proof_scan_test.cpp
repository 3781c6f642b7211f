// include/bulletproofs.hpp: RangeProof::scan_batch (bpgpu_rangeproof_scan_batch): a wallet service with several keys follows one chain;
// every output comes back under the key that made it, with value, blinding and message, from one transcript replay per row -- and equals
// what rewind_batch finds under that key's own seeds.  Runs on the GPU.
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
    const size_t nb = 70, n = 64, nkeys = 5;   // more than one workgroup of 64 lanes
    std::vector<uint64_t> values;
    std::vector<ScalarBytes> blindings;
    std::vector<std::array<uint8_t, 16>> messages(nb);
    std::vector<uint8_t> keys(32 * (nkeys + 1));   // the last one is a stranger's: the wallet does not hold it
    for (size_t q = 0; q < keys.size(); q++) keys[q] = static_cast<uint8_t>(7 * q + 1 + q / 32);
    for (size_t i = 0; i < nb; i++) {
        values.push_back(i == 0 ? 0 : i == 1 ? ~0ull : i == 2 ? 1ull << 63 : i * i * 1000003ull + 1);
        ScalarBytes b{};
        if (i) for (int q = 0; q < 31; q++) b[q] = static_cast<uint8_t>(29 * i + 5 * q + 1);
        blindings.push_back(b);
        for (int q = 0; q < 16; q++) messages[i][q] = static_cast<uint8_t>(i == 1 ? 0xff : i % 3 == 0 ? 0 : 11 * i + q);
    }
    // the senders: row i pays key i % (nkeys + 1) -- every sixth row goes to the stranger
    const std::vector<CompressedRistretto> coms = gens.commit_batch(values, &blindings).first;
    std::vector<std::vector<uint8_t>> per_key;
    for (size_t j = 0; j <= nkeys; j++) per_key.push_back(RangeProof::rewind_seeds(gens.ctx(), &keys[32 * j], coms));
    std::vector<uint8_t> seeds(32 * nb);
    for (size_t i = 0; i < nb; i++) std::memcpy(&seeds[32 * i], &per_key[i % (nkeys + 1)][32 * i], 32);
    std::vector<Transcript> tp = sessions(nb, "scan client");
    const auto made = RangeProof::prove_batch_rewindable(gens, pc, tp, values, blindings, n, seeds.data(), messages);
    std::vector<std::vector<uint8_t>> proofs;
    for (size_t i = 0; i < nb; i++) {
        CHECK(made[i].second == coms[i]);
        proofs.push_back(made[i].first.to_bytes());
    }
    // the wallet service scans the block under its five keys
    const auto found = RangeProof::scan_batch(gens, pc, sessions(nb, "scan client"), proofs, coms, n, keys.data(), nkeys);
    CHECK(found.index() == 0);
    for (size_t i = 0; i < nb; i++) {
        const auto &r = std::get<0>(found)[i];
        if (i % (nkeys + 1) == nkeys) {
            CHECK(!r.has_value());
            continue;
        }
        CHECK(r.has_value() && r->first == i % (nkeys + 1));
        CHECK(r->second.value == values[i] && r->second.blinding == blindings[i] && r->second.message == messages[i]);
    }
    // ... and finds what one rewind per key finds
    for (size_t j = 0; j < nkeys; j++) {
        const auto mine = RangeProof::rewind_batch(gens, pc, sessions(nb, "scan client"), proofs, coms, n, per_key[j].data());
        CHECK(mine.index() == 0);
        for (size_t i = 0; i < nb; i++) {
            const auto &s = std::get<0>(found)[i];
            CHECK(std::get<0>(mine)[i].has_value() == (s.has_value() && s->first == j));
        }
    }
    // with the stranger's key too, every row is found; a key listed twice reports the lower index
    const auto all = RangeProof::scan_batch(gens, pc, sessions(nb, "scan client"), proofs, coms, n, keys.data(), nkeys + 1);
    CHECK(all.index() == 0);
    for (size_t i = 0; i < nb; i++) CHECK(std::get<0>(all)[i].has_value() && std::get<0>(all)[i]->first == i % (nkeys + 1));
    std::vector<uint8_t> twice(keys.begin() + 32, keys.begin() + 64);
    twice.insert(twice.end(), keys.begin(), keys.begin() + 64);   // keys 1, 0, 1
    const auto dup = RangeProof::scan_batch(gens, pc, sessions(nb, "scan client"), proofs, coms, n, twice.data(), 3);
    CHECK(dup.index() == 0 && std::get<0>(dup)[1].has_value() && std::get<0>(dup)[1]->first == 0 && std::get<0>(dup)[0]->first == 1);
    // one shared transcript and a single key
    Transcript one("single scan");
    std::vector<Transcript> shared = {one};
    const auto two = RangeProof::prove_batch_rewindable(gens, pc, shared, {values[6], values[7]}, {blindings[6], blindings[7]}, n, &seeds[32 * 6]);
    const auto s1 = RangeProof::scan_batch(gens, pc, {one}, {two[0].first.to_bytes(), two[1].first.to_bytes()}, {coms[6], coms[7]}, n, &keys[32 * 1], 1);
    CHECK(s1.index() == 0 && !std::get<0>(s1)[0].has_value() && std::get<0>(s1)[1].has_value() && std::get<0>(s1)[1]->second.value == values[7]);
    // a scalar that is not canonical: FormatError; no keys: the library refuses
    std::vector<std::vector<uint8_t>> bad = proofs;
    std::memset(&bad[3][192], 0xff, 32);
    const auto fmt = RangeProof::scan_batch(gens, pc, sessions(nb, "scan client"), bad, coms, n, keys.data(), nkeys);
    CHECK(fmt.index() == 1 && std::get<1>(fmt) == ProofError::FormatError);
    bool threw = false;
    try {
        RangeProof::scan_batch(gens, pc, sessions(nb, "scan client"), proofs, coms, n, keys.data(), 0);
    } catch (const GpuError &) {
        threw = true;
    }
    CHECK(threw);
    std::printf("range_proof_scan_test ok\n");
    return 0;
}
