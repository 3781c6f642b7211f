// include/bulletproofs.hpp: LinearProof on one Transcript per proof -- create_batch and the std::vector<Transcript>& overloads of
// verify_batch / verify_batch_combined (bpgpu_linear_create_batch_ts, bpgpu_linear_verify_batch_ts, bpgpu_linear_verify_rlc_ts).  Every
// proof belongs to its own session: a transcript bound to that session before the sub-protocol starts.  Runs on the GPU.
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
static std::vector<Transcript> sessions(size_t nb) {
    std::vector<Transcript> out;
    for (size_t i = 0; i < nb; i++) {
        Transcript t("payment-protocol v3");
        std::vector<uint8_t> id(i * 61 + 3, static_cast<uint8_t>(0x40 + i));
        t.append_message("session", id.data(), id.size());
        out.push_back(t);
    }
    return out;
}

int main() {
    const size_t n = 8, nb = 4;
    BulletproofGens gens(64, 1);
    bpgpu_ctx *ctx = gens.ctx();
    const std::vector<CompressedRistretto> G = gens.share_G(0, n);
    const CompressedRistretto F = gens.pedersen().B, B = gens.pedersen().B_blinding;   // linear_proof.rs:405-411
    // witnesses small enough that c = <a, b> needs no reduction; C = <a, G> + r B + c F through the library's own MSM
    std::vector<std::vector<ScalarBytes>> a_vecs(nb), b_vecs(nb);
    std::vector<ScalarBytes> rs(nb);
    std::vector<CompressedRistretto> Cs(nb);
    std::vector<uint8_t> seeds(32 * nb);
    for (size_t i = 0; i < nb; i++) {
        uint64_t c = 0;
        for (size_t j = 0; j < n; j++) {
            const uint64_t a = 1000 * (i + 1) + 7 * j + 1, b = 31 * (j + 2) + i;
            a_vecs[i].push_back(small_scalar(a));
            b_vecs[i].push_back(small_scalar(b));
            c += a * b;
        }
        rs[i] = small_scalar(0x1234567890abcdefull + i);
        rs[i][20] = static_cast<uint8_t>(0x55 + i);
        std::vector<uint8_t> sc, pt;
        for (size_t j = 0; j < n; j++) {
            sc.insert(sc.end(), a_vecs[i][j].begin(), a_vecs[i][j].end());
            pt.insert(pt.end(), G[j].begin(), G[j].end());
        }
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

    // create: one pass, every prover transcript advanced; the same seeds give the same proofs, the library's own seeds fresh ones
    std::vector<Transcript> provers = sessions(nb);
    std::vector<LinearProof> proofs = LinearProof::create_batch(ctx, provers, Cs, rs, a_vecs, b_vecs, G, F, B, seeds.data());
    CHECK(proofs.size() == nb);
    const std::vector<Transcript> start = sessions(nb);
    for (size_t i = 0; i < nb; i++) {
        CHECK(proofs[i].serialized_size() == 32 * (2 * 3 + 3));
        CHECK(provers[i].state() != start[i].state() && !provers[i].is_fresh());
        for (size_t j = 0; j < i; j++) CHECK(proofs[i].to_bytes() != proofs[j].to_bytes());
    }
    {
        std::vector<Transcript> again = sessions(nb);
        std::vector<LinearProof> same = LinearProof::create_batch(ctx, again, Cs, rs, a_vecs, b_vecs, G, F, B, seeds.data());
        std::vector<Transcript> t3 = sessions(nb);
        std::vector<LinearProof> fresh = LinearProof::create_batch(ctx, t3, Cs, rs, a_vecs, b_vecs, G, F, B);
        for (size_t i = 0; i < nb; i++) {
            CHECK(same[i].to_bytes() == proofs[i].to_bytes() && again[i].state() == provers[i].state());
            CHECK(fresh[i].to_bytes() != proofs[i].to_bytes());
            Transcript v = start[i];
            CHECK(fresh[i].verify(ctx, v, Cs[i], G, F, B, b_vecs[i]) == Status::Ok() && v.state() == t3[i].state());
        }
    }

    // verify: per proof and combined, each verifier transcript ends where its prover's did -- and where the single-proof call ends
    std::vector<Transcript> v1 = sessions(nb), v2 = sessions(nb);
    std::vector<Status> r1 = LinearProof::verify_batch(ctx, v1, proofs, Cs, G, F, B, b_vecs);
    std::vector<Status> r2 = LinearProof::verify_batch_combined(ctx, v2, proofs, Cs, G, F, B, b_vecs);
    CHECK(r1.size() == nb && r2.size() == nb);
    for (size_t i = 0; i < nb; i++) {
        CHECK(r1[i] == Status::Ok() && r2[i] == Status::Ok());
        CHECK(v1[i].state() == provers[i].state() && v2[i].state() == provers[i].state());
        Transcript one = start[i];
        CHECK(proofs[i].verify(ctx, one, Cs[i], G, F, B, b_vecs[i]) == Status::Ok() && one.state() == v1[i].state());
    }

    // a proof does not verify on another session's transcript: rows 1 and 3 swapped fail on both paths, rows 0 and 2 still pass, and a
    // failed row's transcript is its own state right after innerproduct_domain_sep(n)
    std::vector<Transcript> w1 = sessions(nb), w2 = sessions(nb);
    std::swap(w1[1], w1[3]);
    std::swap(w2[1], w2[3]);
    r1 = LinearProof::verify_batch(ctx, w1, proofs, Cs, G, F, B, b_vecs);
    r2 = LinearProof::verify_batch_combined(ctx, w2, proofs, Cs, G, F, B, b_vecs);
    for (size_t i = 0; i < nb; i++) {
        const bool swapped = i == 1 || i == 3;
        CHECK(r1[i] == (swapped ? Status::Err(ProofError::VerificationError) : Status::Ok()) && r2[i] == r1[i]);
        CHECK(w1[i].state() == w2[i].state());
    }
    CHECK(w1[0].state() == provers[0].state() && w1[2].state() == provers[2].state());

    // a non-canonical scalar in one row: FormatError for that row alone, its transcript right behind the separator
    {
        std::vector<uint8_t> raw;
        raw = proofs[2].to_bytes();
        std::memset(&raw[raw.size() - 64], 0xff, 32);
        std::vector<uint8_t> pb, cb, bb, ts, verdict(nb), tso(nb * BPGPU_TRANSCRIPT_BYTES);
        for (size_t i = 0; i < nb; i++) {
            const std::vector<uint8_t> &p = i == 2 ? raw : proofs[i].to_bytes();
            pb.insert(pb.end(), p.begin(), p.end());
            cb.insert(cb.end(), Cs[i].begin(), Cs[i].end());
            for (const auto &x : b_vecs[i]) bb.insert(bb.end(), x.begin(), x.end());
            ts.insert(ts.end(), start[i].state().begin(), start[i].state().end());
        }
        CHECK(bpgpu_linear_verify_rlc_ts(ctx, n, nb, pb.data(), raw.size(), ts.data(), BPGPU_TRANSCRIPT_BYTES, cb.data(), G[0].data(), F.data(), B.data(),
                                         bb.data(), 0, nullptr, verdict.data(), nullptr, tso.data()) == BPGPU_OK);
        CHECK(verdict[0] == 0 && verdict[1] == 0 && verdict[2] == static_cast<uint8_t>(ProofError::FormatError) && verdict[3] == 0);
        Transcript sep = start[2];
        const uint8_t ipp[6] = {'i', 'p', 'p', ' ', 'v', '1'};
        sep.append_message("dom-sep", ipp, 6);
        sep.append_u64("n", n);
        CHECK(std::memcmp(&tso[2 * BPGPU_TRANSCRIPT_BYTES], sep.state().data(), BPGPU_TRANSCRIPT_BYTES) == 0);
        CHECK(std::memcmp(&tso[0], provers[0].state().data(), BPGPU_TRANSCRIPT_BYTES) == 0);
    }

    // the argument checks of the overloads
    {
        std::vector<Transcript> three = sessions(nb - 1);
        bool threw = false;
        try {
            LinearProof::verify_batch(ctx, three, proofs, Cs, G, F, B, b_vecs);
        } catch (const std::invalid_argument &) {
            threw = true;
        }
        CHECK(threw);
        std::vector<Transcript> none;
        CHECK(LinearProof::create_batch(ctx, none, {}, {}, {}, {}, G, F, B).empty());
    }
    std::printf("linear_proof_ts: ok\n");
    return 0;
}
