"""Test twin of the reference's R1CS prover WITH its real randomness: r1cs_twin.Prover draws its blindings from a ShakeRng;
prover.rs:403-413 draws them from a TranscriptRng built on the transcript right after "m", rekeyed with every v_blinding and
finalized with 32 bytes of thread_rng().  Restated from merlin 2 (transcript.rs: build_rng, rekey_with_witness_bytes,
finalize; TranscriptRng::fill_bytes); nothing in the reference pins it.  TEST INFRASTRUCTURE ONLY.

Also: the hand-written gadgets that exercise allocate()'s pairing, prove / verify helpers over any gadget, and a host
evaluation of a recorded witness program (bulletproofs_amd.r1cs.Prover) for given challenge values."""
import bp_twin as T
import r1cs_twin as R

L = T.L


class TranscriptRng:
    """Built lazily on the first scalar(): the twin's prove() asks for its first blinding right after append_u64("m")."""

    def __init__(self, prover, rng32):
        self.p, self.rng32, self.s = prover, bytes(rng32), None

    def scalar(self):
        if self.s is None:
            s = self.p.t.strobe.clone()                                  # build_rng
            for vb in self.p.v_blinding:                                 # rekey_with_witness_bytes(b"v_blinding", vb)
                s.meta_ad(b"v_blinding", False)
                s.meta_ad((32).to_bytes(4, "little"), True)
                R.strobe_key(s, R.sc_bytes(vb))
            s.meta_ad(b"rng", False)                                     # finalize
            R.strobe_key(s, self.rng32)
            self.s = s
        self.s.meta_ad((64).to_bytes(4, "little"), False)                # fill_bytes(64) -> Scalar::from_bytes_mod_order_wide
        return int.from_bytes(self.s.prf(64), "little") % L


class Prover(R.Prover):
    """r1cs_twin.Prover with the reference's rng; records the challenge values it draws (self.challenges)"""

    def __init__(self, gens, transcript, rng32):
        super().__init__(gens, transcript)
        self.rng = TranscriptRng(self, rng32)
        self.challenges = []

    def challenge_scalar(self, label):
        c = self.t.challenge_scalar(label)
        self.challenges.append(c)
        return c


# ---- hand-written gadgets over two committed values (x, y); vals = (x, y) on the prover, None on the verifier --------------
def split_gadget(cs, vs, vals):
    """an allocate() pair split by another multiplier (prover.rs:121-140)"""
    a = cs.allocate(None if vals is None else vals[0])                  # L_0, the pair stays open
    _, _, o = cs.multiply(vs[0] + a, vs[1] - 2)                          # multiplier 1 reads L_0
    b = cs.allocate(None if vals is None else vals[1])                  # R_0: a_O[0] = x y
    cs.constrain(a - vs[0])
    cs.constrain(b - vs[1])


def open_gadget(cs, vs, vals):
    """pairs left open at the end of each phase (a_R = 0) and assignments that are expressions of a challenge"""
    a = cs.allocate(None if vals is None else vals[0])                  # L_0, open at the end of phase 1
    cs.constrain(a - vs[0])

    def cb(cs):
        z = cs.challenge_scalar(b"open challenge")
        l = cs.allocate(None if vals is None else vals[1] * z)          # L_1 = y z (an LC row in the recorder)
        r = cs.allocate(None if vals is None else 3)                    # R_1 = 3
        cs.constrain(l - vs[1] * z)
        cs.constrain(r - 3)
        d = cs.allocate(None if vals is None else vals[0] + z)          # L_2 = x + z, open at the end of phase 2
        cs.constrain(d - vs[0] - z)
        _, _, o = cs.multiply(l + 1, vs[0] - z)                          # multiplier 3 while pair 2 is open

    cs.specify_randomized_constraints(cb)


# ---- proofs -------------------------------------------------------------------------------------------------------------------
def prove(gens, cap, st0, vals, blindings, gadget, rng32):
    """Prover::new over the transcript state st0, commit every value, run gadget(cs, vars), prove:
    (proof, [V], twin prover) -- the prover's transcript is left as prove leaves it (twin.t)"""
    t = R.transcript_from_state(st0)
    P = Prover(gens, t, rng32)
    vars_, Vs = [], []
    for v, b in zip(vals, blindings):
        V, var = P.commit(v, b)
        Vs.append(V)
        vars_.append(var)
    gadget(P, vars_)
    return P.prove(cap), Vs, P


def verify(gens, cap, st0, proof_bytes, Vs, gadget, rng32=bytes(32)):
    return R.verify_with(gadget, gens, cap, st0, proof_bytes, Vs, rng32)[0]


# ---- the recorded witness program on the host -----------------------------------------------------------------------------
def eval_witness(rec, challenges):
    """a_L, a_R, a_O of a recorded bulletproofs_amd.r1cs.Prover for the given phase-2 challenge values"""
    from bulletproofs_amd import r1cs
    rec._finish()
    n = rec.num_vars
    aL, aR, aO = [0] * n, [0] * n, [0] * n

    def row(r):
        acc = 0
        for (kind, idx), ch, pw, k in rec.rows[r]:
            val = {r1cs.KIND_L: aL, r1cs.KIND_R: aR, r1cs.KIND_O: aO, r1cs.KIND_V: rec.v}.get(kind)
            x = 1 if kind == r1cs.KIND_ONE else val[idx]
            acc += k * (pow(challenges[ch], pw, L) if ch is not None else 1) * x
        return acc % L

    def src(s):
        if s == r1cs.SRC_ZERO:
            return 0
        if s & r1cs.SRC_FREE:
            return rec.free[s & ~r1cs.SRC_FREE]
        return row(s)

    for i in range(n):
        aL[i] = src(rec.src_left[i])
        aR[i] = src(rec.src_right[i])
        aO[i] = aL[i] * aR[i] % L
    return aL, aR, aO
