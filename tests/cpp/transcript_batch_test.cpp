// include/bulletproofs.hpp: TranscriptBatch -- many transcripts built and bound on the GPU by one script (bpgpu_transcript_batch) -- against
// the same sessions bound one by one with Transcript's host helpers, and in place of the std::vector<Transcript> that LinearProof's
// batch calls take.  Runs on the GPU.
#include <cstdio>
#include <cstring>
#include <string>
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

// session i: its id is i * 61 + 3 bytes long, so the transcripts stand at different STROBE positions
static std::vector<std::vector<uint8_t>> session_ids(size_t nb) {
    std::vector<std::vector<uint8_t>> out;
    for (size_t i = 0; i < nb; i++) out.emplace_back(i * 61 + 3, static_cast<uint8_t>(0x40 + i));
    return out;
}

int main() {
    const size_t n = 4, nb = 5;
    BulletproofGens gens(8, 1);
    bpgpu_ctx *ctx = gens.ctx();
    const std::vector<std::vector<uint8_t>> ids = session_ids(nb);

    // the same history row by row on the host and as one script on the device
    std::vector<Transcript> lone;
    std::vector<std::vector<uint8_t>> lone_binding(nb, std::vector<uint8_t>(16));
    std::vector<uint64_t> amounts;
    for (size_t i = 0; i < nb; i++) {
        Transcript t("payment-protocol v3");
        t.append_message("session", ids[i].data(), ids[i].size());
        t.append_u64("amount", 1000 + i);
        t.challenge_bytes("binding", lone_binding[i].data(), 16);
        t.append_message("context", reinterpret_cast<const uint8_t *>("shared"), 6);
        lone.push_back(t);
        amounts.push_back(1000 + i);
    }
    auto bound = [&]() {
        TranscriptBatch b(ctx, "payment-protocol v3", nb);
        b.append_message("session", ids);
        b.append_u64("amount", amounts);
        return b;
    };
    TranscriptBatch batch = bound();
    CHECK(batch.size() == nb);
    CHECK(batch.challenge_bytes("binding", 16) == lone_binding);
    batch.append_message("context", reinterpret_cast<const uint8_t *>("shared"), 6);
    for (size_t i = 0; i < nb; i++) CHECK(batch[i].state() == lone[i].state());
    CHECK(batch.states().size() == nb * BPGPU_TRANSCRIPT_BYTES);

    // clone, from_transcript, from_states, challenge_scalars
    TranscriptBatch other = batch.clone();
    other.append_u64("more", 7);
    Transcript l0 = lone[0];
    l0.append_u64("more", 7);
    CHECK(other[0].state() == l0.state() && batch[0].state() == lone[0].state());
    TranscriptBatch fanned = TranscriptBatch::from_transcript(ctx, lone[2], 3);
    fanned.append_u64("row", std::vector<uint64_t>{1, 2, 3});
    for (uint64_t r = 0; r < 3; r++) {
        Transcript t = lone[2];
        t.append_u64("row", r + 1);
        CHECK(fanned[r].state() == t.state());
    }
    TranscriptBatch again = TranscriptBatch::from_states(ctx, lone);
    const std::vector<ScalarBytes> xs = again.challenge_scalars("x");
    for (size_t i = 0; i < nb; i++) {
        Transcript t = lone[i];
        uint8_t wide[64];
        t.challenge_bytes("x", wide, 64);
        CHECK(again[i].state() == t.state());
        CHECK((xs[i][31] & 0xe0) == 0);                       // reduced mod l < 2^253 (the values: tests/test_gpu_transcript_batch.py)
    }

    // LinearProof on the batch == on the vector: the same proofs, the same verdicts, the same advanced states
    const std::vector<CompressedRistretto> G = gens.share_G(0, n);
    const CompressedRistretto F = gens.pedersen().B, B = gens.pedersen().B_blinding;
    std::vector<std::vector<ScalarBytes>> a_vecs(nb), b_vecs(nb);
    std::vector<ScalarBytes> rs(nb);
    std::vector<CompressedRistretto> Cs(nb);
    std::vector<uint8_t> seeds(32 * nb);
    for (size_t i = 0; i < nb; i++) {
        uint64_t c = 0;
        std::vector<uint8_t> sc, pt;
        for (size_t j = 0; j < n; j++) {
            const uint64_t a = 1000 * (i + 1) + 7 * j + 1, b = 31 * (j + 2) + i;
            a_vecs[i].push_back(small_scalar(a));
            b_vecs[i].push_back(small_scalar(b));
            c += a * b;
            sc.insert(sc.end(), a_vecs[i][j].begin(), a_vecs[i][j].end());
            pt.insert(pt.end(), G[j].begin(), G[j].end());
        }
        rs[i] = small_scalar(0x1234567890abcdefull + i);
        const ScalarBytes cs = small_scalar(c);
        sc.insert(sc.end(), rs[i].begin(), rs[i].end());
        pt.insert(pt.end(), B.begin(), B.end());
        sc.insert(sc.end(), cs.begin(), cs.end());
        pt.insert(pt.end(), F.begin(), F.end());
        const uint32_t nterms = static_cast<uint32_t>(n + 2);
        uint8_t st = 0xff;
        CHECK(bpgpu_msm_batch(ctx, 1, &nterms, sc.data(), pt.data(), Cs[i].data(), &st) == BPGPU_OK && st == 0);
        for (size_t q = 0; q < 32; q++) seeds[32 * i + q] = static_cast<uint8_t>(17 * i + 3 * q + 1);
    }
    std::vector<Transcript> pv = lone;
    TranscriptBatch pb = batch.clone();
    const std::vector<LinearProof> want = LinearProof::create_batch(ctx, pv, Cs, rs, a_vecs, b_vecs, G, F, B, seeds.data());
    const std::vector<LinearProof> got = LinearProof::create_batch(ctx, pb, Cs, rs, a_vecs, b_vecs, G, F, B, seeds.data());
    CHECK(got.size() == nb);
    for (size_t i = 0; i < nb; i++) CHECK(got[i].to_bytes() == want[i].to_bytes() && pb[i].state() == pv[i].state() && pv[i].state() != lone[i].state());
    std::vector<LinearProof> mixed = want;
    std::swap(mixed[1], mixed[3]);                            // two proofs on the wrong sessions
    for (int combined = 0; combined < 2; combined++) {
        std::vector<Transcript> vv = lone;
        TranscriptBatch vb = batch.clone();
        const std::vector<Status> r1 = combined ? LinearProof::verify_batch_combined(ctx, vv, mixed, Cs, G, F, B, b_vecs)
                                                : LinearProof::verify_batch(ctx, vv, mixed, Cs, G, F, B, b_vecs);
        const std::vector<Status> r2 = combined ? LinearProof::verify_batch_combined(ctx, vb, mixed, Cs, G, F, B, b_vecs)
                                                : LinearProof::verify_batch(ctx, vb, mixed, Cs, G, F, B, b_vecs);
        for (size_t i = 0; i < nb; i++) {
            const bool swapped = i == 1 || i == 3;
            CHECK(r1[i] == r2[i] && r1[i] == (swapped ? Status::Err(ProofError::VerificationError) : Status::Ok()));
            CHECK(vb[i].state() == vv[i].state());
        }
        CHECK(vb[0].state() == pv[0].state());
    }
    // RangeProof::prove_batch on the batch == on the vector
    {
        const PedersenGens pc = gens.pedersen();
        std::vector<std::vector<uint64_t>> values;
        std::vector<std::vector<ScalarBytes>> blindings;
        for (size_t i = 0; i < nb; i++) {
            values.push_back({17 * i + 3});
            blindings.push_back({small_scalar(0x9000 + i)});
        }
        std::vector<Transcript> rv = lone;
        TranscriptBatch rb = batch.clone();
        const auto want_rp = RangeProof::prove_batch(gens, pc, rv, values, blindings, 8, seeds.data());
        const auto got_rp = RangeProof::prove_batch(gens, pc, rb, values, blindings, 8, seeds.data());
        CHECK(got_rp.size() == nb);
        for (size_t i = 0; i < nb; i++) {
            CHECK(got_rp[i].first.to_bytes() == want_rp[i].first.to_bytes() && got_rp[i].second == want_rp[i].second);
            CHECK(rb[i].state() == rv[i].state() && rv[i].state() != lone[i].state());
        }
    }
    std::printf("transcript_batch_test ok\n");
    return 0;
}
