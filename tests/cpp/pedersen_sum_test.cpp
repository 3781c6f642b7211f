// include/bulletproofs.hpp: BulletproofGens::sum_commitments / verify_balance -- signed sums of commitments and the balance check
// (bpgpu_pedersen_sum_batch / _balance_batch) -- against commit_batch and verify_openings.  Runs on the GPU.
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

// a + b for scalars below 2^248 (no reduction needed)
static ScalarBytes add_small(const ScalarBytes &a, const ScalarBytes &b) {
    ScalarBytes s{};
    unsigned carry = 0;
    for (int i = 0; i < 32; i++) {
        const unsigned t = a[i] + b[i] + carry;
        s[i] = static_cast<uint8_t>(t);
        carry = t >> 8;
    }
    return s;
}

int main() {
    BulletproofGens gens(8, 1);
    // 150 commitments to (i + 1, r_i), r_i below 2^240
    const size_t n = 150;
    std::vector<uint64_t> values;
    std::vector<ScalarBytes> blindings;
    for (size_t i = 0; i < n; i++) {
        values.push_back(i + 1);
        ScalarBytes b{};
        for (int q = 0; q < 30; q++) b[q] = static_cast<uint8_t>(31 * i + 7 * q + 3);
        blindings.push_back(b);
    }
    const std::vector<CompressedRistretto> coms = gens.commit_batch(values, &blindings).first;
    // rows of 0, 1, 2, 3, 64 and 80 inputs (the last two cross workgroups of 64 terms); the row's sum opens to (sum v_i, sum r_i)
    const size_t lens[6] = {0, 1, 2, 3, 64, 80};
    BulletproofGens::Rows inputs, none(6);
    std::vector<uint64_t> v_sum;
    std::vector<ScalarBytes> r_sum;
    size_t k = 0;
    for (size_t len : lens) {
        inputs.emplace_back(coms.begin() + k, coms.begin() + k + len);
        uint64_t v = 0;
        ScalarBytes r{};
        for (size_t i = k; i < k + len; i++) v += values[i], r = add_small(r, blindings[i]);
        v_sum.push_back(v);
        r_sum.push_back(r);
        k += len;
    }
    for (const Status &s : gens.verify_balance(inputs, none, &v_sum, &r_sum)) CHECK(s.is_ok());
    // the sums themselves: what commit_batch gives for (sum v_i, sum r_i); an empty row with no scalars is the identity's encoding
    const auto sums = gens.sum_commitments(inputs);
    const std::vector<CompressedRistretto> direct = gens.commit_batch(v_sum, &r_sum).first;
    CHECK(sums.size() == 6);
    for (size_t r = 0; r < 6; r++) CHECK(sums[r].has_value() && *sums[r] == direct[r]);
    CHECK(*sums[0] == CompressedRistretto{});
    // inputs - inputs + (v, r) is the commitment to (v, r); inputs - outputs with outputs = the row's own sum balances to (0, 0)
    const auto again = gens.sum_commitments(inputs, &inputs, &v_sum, &r_sum);
    for (size_t r = 0; r < 6; r++) CHECK(again[r].has_value() && *again[r] == direct[r]);
    BulletproofGens::Rows outputs;
    for (size_t r = 0; r < 6; r++) outputs.push_back({direct[r]});
    for (const Status &s : gens.verify_balance(inputs, outputs)) CHECK(s.is_ok());
    // verdicts: a wrong value, a flipped bit of one input, an encoding that does not decode, a non-canonical blinding
    std::vector<uint64_t> bad_v = v_sum;
    std::vector<ScalarBytes> bad_r = r_sum;
    BulletproofGens::Rows bad_in = inputs;
    bad_v[1] ^= 1;
    bad_in[2][1][3] ^= 0x20;
    bad_in[4][63].fill(0xff);
    bad_r[5].fill(0xff);
    const std::vector<Status> vd = gens.verify_balance(bad_in, none, &bad_v, &bad_r);
    for (size_t r = 0; r < 6; r++) {
        if (r == 1 || r == 2 || r == 4) CHECK(vd[r] == Status::Err(ProofError::VerificationError));
        else if (r == 5) CHECK(vd[r] == Status::Err(ProofError::FormatError));
        else CHECK(vd[r].is_ok());
    }
    BulletproofGens::Rows hole_in = inputs;
    hole_in[4][63].fill(0xff);
    const auto holes = gens.sum_commitments(hole_in);
    for (size_t r = 0; r < 6; r++) CHECK(holes[r].has_value() == (r != 4));
    bool threw = false;
    try {
        gens.sum_commitments(inputs, nullptr, &v_sum, &bad_r);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    CHECK(threw);
    threw = false;
    try {
        gens.verify_balance(inputs, BulletproofGens::Rows(5));
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    CHECK(threw);
    CHECK(gens.sum_commitments(BulletproofGens::Rows{}).empty() && gens.verify_balance(BulletproofGens::Rows{}, BulletproofGens::Rows{}).empty());
    std::printf("pedersen_sum_test ok\n");
    return 0;
}
