// include/bulletproofs.hpp: BulletproofGens::commit_batch / verify_openings -- many Pedersen commitments in one launch
// (bpgpu_pedersen_commit_batch / _open_batch) -- against BulletproofGens::commit row by row.  Runs on the GPU.
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

static ScalarBytes small_scalar(uint64_t x) {
    ScalarBytes s{};
    for (int i = 0; i < 8; i++) s[i] = static_cast<uint8_t>(x >> (8 * i));
    return s;
}

int main() {
    BulletproofGens gens(8, 1);
    const size_t nb = 70;   // more than one wavefront
    std::vector<uint64_t> values;
    std::vector<ScalarBytes> scalars, blindings;
    for (size_t i = 0; i < nb; i++) {
        values.push_back(i == 0 ? 0 : i == 1 ? ~0ull : 0x0123456789abcdefull * i);
        scalars.push_back(small_scalar(values.back()));
        ScalarBytes b{};
        for (int q = 0; q < 31; q++) b[q] = static_cast<uint8_t>(i == 0 ? 0 : 17 * i + 29 * q + 1);   // below 2^248: canonical
        blindings.push_back(b);
    }
    // given blindings: row i == commit(values[i], blindings[i]); u64 values and the same values as scalars: the same bytes
    auto [coms, bl] = gens.commit_batch(values, &blindings);
    auto [coms32, bl32] = gens.commit_batch(scalars, &blindings);
    CHECK(coms.size() == nb && bl == blindings && coms == coms32 && bl32 == blindings);
    for (size_t i = 0; i < nb; i += 9) CHECK(coms[i] == gens.commit(scalars[i], blindings[i]));
    CHECK(coms[0] == CompressedRistretto{});   // (0, 0): the identity's encoding
    // one seed for the batch: the blindings come back, open the commitments, and rows 3.. of the call are first_draw = 3
    uint8_t seed[32];
    std::memset(seed, 24, 32);
    auto [scoms, sbl] = gens.commit_batch(values, nullptr, seed);
    CHECK(scoms.size() == nb && sbl.size() == nb && sbl[0] != sbl[1]);
    for (size_t i = 0; i < nb; i += 13) CHECK(scoms[i] == gens.commit(scalars[i], sbl[i]));
    const std::vector<uint64_t> tail(values.begin() + 3, values.end());
    auto [tcoms, tbl] = gens.commit_batch(tail, nullptr, seed, 3);
    CHECK(tcoms == std::vector<CompressedRistretto>(scoms.begin() + 3, scoms.end()));
    CHECK(tbl == std::vector<ScalarBytes>(sbl.begin() + 3, sbl.end()));
    // the library's own seed: two calls differ, each call's blindings open its commitments
    auto [c1, b1] = gens.commit_batch(values, nullptr);
    auto [c2, b2] = gens.commit_batch(values, nullptr);
    CHECK(b1 != b2 && c1 != c2);
    for (const Status &s : gens.verify_openings(c1, values, b1)) CHECK(s.is_ok());
    for (const Status &s : gens.verify_openings(c2, scalars, b2)) CHECK(s.is_ok());
    // verdicts: a flipped commitment bit, a wrong value, an encoding that does not decode, a non-canonical blinding
    std::vector<CompressedRistretto> bad_c = c1;
    std::vector<uint64_t> bad_v = values;
    std::vector<ScalarBytes> bad_b = b1;
    bad_c[2][5] ^= 0x10;
    bad_v[4] ^= 1;
    bad_c[6].fill(0xff);
    bad_b[8].fill(0xff);
    const std::vector<Status> vd = gens.verify_openings(bad_c, bad_v, bad_b);
    for (size_t i = 0; i < nb; i++) {
        if (i == 2 || i == 4 || i == 6) CHECK(vd[i] == Status::Err(ProofError::VerificationError));
        else if (i == 8) CHECK(vd[i] == Status::Err(ProofError::FormatError));
        else CHECK(vd[i].is_ok());
    }
    // a non-canonical scalar in commit_batch throws, as commit does; mismatched lengths and blindings beside a seed are refused
    bool threw = false;
    try {
        gens.commit_batch(values, &bad_b);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    CHECK(threw);
    threw = false;
    try {
        gens.commit_batch(values, &blindings, seed);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    CHECK(threw);
    CHECK(gens.commit_batch(std::vector<uint64_t>{}, nullptr, seed).first.empty());
    std::printf("pedersen_test ok\n");
    return 0;
}
