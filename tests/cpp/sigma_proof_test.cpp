// include/bulletproofs.hpp: SigmaStatement / SigmaRelation (bpgpu_sigma_*) -- a DLEQ relation and "one amount under two value bases"
// written once, proved and verified per proof and combined, on vectors of transcripts and on a TranscriptBatch.  Runs on the GPU.
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
        t.append_u64("session", 1000 + i);
        ts.push_back(t);
    }
    return ts;
}

// sum scalars[i] points[i] through bpgpu_msm_batch
static CompressedRistretto msm(const BulletproofGens &gens, const std::vector<ScalarBytes> &sc, const std::vector<CompressedRistretto> &pt) {
    std::vector<uint8_t> s, p;
    for (const auto &x : sc) s.insert(s.end(), x.begin(), x.end());
    for (const auto &x : pt) p.insert(p.end(), x.begin(), x.end());
    const uint32_t nt = static_cast<uint32_t>(sc.size());
    CompressedRistretto out{};
    uint8_t status = 0;
    if (bpgpu_msm_batch(gens.ctx(), 1, &nt, s.data(), p.data(), out.data(), &status) != BPGPU_OK || status != 0) throw GpuError("msm failed");
    return out;
}

static ScalarBytes small(size_t i, int salt) {
    ScalarBytes s{};
    for (int q = 0; q < 30; q++) s[q] = static_cast<uint8_t>(31 * i + 7 * q + salt);
    return s;
}

int main() {
    BulletproofGens gens(8, 1);
    const PedersenGens pc = gens.pedersen();
    const size_t n = 70;   // more than one workgroup of 64 lanes
    std::vector<uint8_t> seeds(32 * n);
    for (size_t i = 0; i < 32 * n; i++) seeds[i] = static_cast<uint8_t>(3 * i + 11);

    // DLEQ: A = x B, H = x Bp
    SigmaStatement st(gens);
    const auto x = st.secret();
    const auto A = st.point(), H = st.point(), Bp = st.point();
    st.equation(A, {{x, st.B}});
    st.equation(H, {{x, Bp}});
    const std::vector<uint8_t> want_desc = {1, 3, 2, 16, 1, 0, 1, 17, 1, 0, 18};
    CHECK(st.descriptor() == want_desc);
    const SigmaRelation dleq = st.compile();
    CHECK(dleq.secrets() == 1 && dleq.points() == 3 && dleq.equations() == 2 && dleq.proof_len() == 96);
    {
        uint8_t dg[32];
        CHECK(bpgpu_sigma_descriptor_check(want_desc.data(), want_desc.size(), 8, dg) == BPGPU_OK && std::memcmp(dg, dleq.digest().data(), 32) == 0);
    }
    SigmaRelation::SecretRows xs;
    SigmaRelation::PointRows pts;
    for (size_t i = 0; i < n; i++) {
        const ScalarBytes xi = small(i, 1), hi = small(i, 2);
        const CompressedRistretto bp = msm(gens, {hi}, {pc.B});
        xs.push_back({xi});
        pts.push_back({msm(gens, {xi}, {pc.B}), msm(gens, {xi}, {bp}), bp});
    }
    std::vector<Transcript> tp = sessions(n, "sigma client");
    const std::vector<SigmaRelation::Proof> proofs = dleq.create_batch(tp, xs, pts, seeds.data());
    CHECK(proofs.size() == n && proofs[0].size() == 96);
    std::vector<Transcript> tv = sessions(n, "sigma client"), tc = sessions(n, "sigma client");
    for (const Status &s : dleq.verify_batch(tv, proofs, pts)) CHECK(s.is_ok());
    for (const Status &s : dleq.verify_batch_combined(tc, proofs, pts)) CHECK(s.is_ok());
    for (size_t i = 0; i < n; i++) CHECK(tv[i].state() == tp[i].state() && tc[i].state() == tp[i].state());   // both sides end in one state
    // one tampered response, one proof under the wrong session, one false instance (H of another row): rejected alone, by both calls alike
    std::vector<SigmaRelation::Proof> bad = proofs;
    bad[64][70] ^= 1;
    SigmaRelation::PointRows bad_pts = pts;
    bad_pts[5][1] = pts[6][1];
    std::vector<Transcript> t1 = sessions(n, "sigma client"), t2 = sessions(n, "sigma client");
    t1[9] = t1[10], t2[9] = t2[10];
    const std::vector<Status> a = dleq.verify_batch(t1, bad, bad_pts), b = dleq.verify_batch_combined(t2, bad, bad_pts);
    for (size_t i = 0; i < n; i++) {
        const bool wrong = i == 64 || i == 9 || i == 5;
        CHECK(a[i] == b[i] && a[i].is_ok() == !wrong);
        if (wrong) CHECK(a[i] == Status::Err(ProofError::VerificationError));
        CHECK(t1[i].state() == t2[i].state());
    }
    // a response that is not canonical: FormatError
    bad = proofs;
    std::memset(bad[3].data() + 64, 0xff, 32);
    std::vector<Transcript> t3 = sessions(n, "sigma client");
    CHECK(dleq.verify_batch_combined(t3, bad, pts)[3] == Status::Err(ProofError::FormatError));
    // a TranscriptBatch in place of the vector, left advanced the same way
    TranscriptBatch tb(gens.ctx(), "sigma client", n);
    std::vector<uint64_t> ids;
    for (size_t i = 0; i < n; i++) ids.push_back(1000 + i);
    tb.append_u64("session", ids);
    for (const Status &s : dleq.verify_batch_combined(tb, proofs, pts)) CHECK(s.is_ok());
    CHECK(tb[7].state() == tp[7].state());
    // one proof
    Transcript one("single"), other("single"), wrong_label("double");
    const SigmaRelation::Proof p1 = dleq.create(one, xs[2], pts[2], seeds.data());
    CHECK(dleq.verify(other, p1, pts[2]).is_ok() && one.state() == other.state());
    CHECK(dleq.verify(wrong_label, p1, pts[2]) == Status::Err(ProofError::VerificationError));

    // one amount under two value bases: C1 = v B + r1 B_blinding, C2 = v Bp + r2 B_blinding
    SigmaStatement sa(gens);
    const auto v = sa.secret(), r1 = sa.secret(), r2 = sa.secret();
    const auto C1 = sa.point(), C2 = sa.point(), B2 = sa.point();
    sa.equation(C1, {{v, sa.B}, {r1, sa.B_blinding}});
    sa.equation(C2, {{v, B2}, {r2, sa.B_blinding}});
    const SigmaRelation same = sa.compile();
    CHECK(same.proof_len() == 160);
    SigmaRelation::SecretRows ys;
    SigmaRelation::PointRows qs;
    for (size_t i = 0; i < 3; i++) {
        const ScalarBytes vi = small(i, 5), a1 = small(i, 6), a2 = small(i, 7);
        const CompressedRistretto b2 = msm(gens, {small(i, 8)}, {pc.B});
        ys.push_back({vi, a1, a2});
        qs.push_back({gens.commit(vi, a1), msm(gens, {vi, a2}, {b2, pc.B_blinding}), b2});
    }
    std::vector<Transcript> sp = sessions(3, "bridge"), sv = sessions(3, "bridge");
    const std::vector<SigmaRelation::Proof> pr = same.create_batch(sp, ys, qs);   // (seeds drawn by the library)
    for (const Status &s : same.verify_batch_combined(sv, pr, qs)) CHECK(s.is_ok());
    CHECK(sv[2].state() == sp[2].state());

    // what the validator refuses, and what the prover refuses
    bool threw = false;
    try {
        SigmaStatement sb(gens);
        const auto y = sb.secret();
        sb.secret();   // never used
        const auto Q = sb.point();
        sb.equation(Q, {{y, sb.B}});
        sb.compile();
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    CHECK(threw);
    threw = false;
    try {
        std::vector<Transcript> t = sessions(1, "x");
        ScalarBytes big;
        big.fill(0xff);
        dleq.create_batch(t, {{big}}, {pts[0]});
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    CHECK(threw);
    std::printf("sigma_proof_test ok\n");
    return 0;
}
