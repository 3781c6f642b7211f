"""Host-side mirror (Python) of the reference crate's `range_proof_mpc` module (src/range_proof/{party,dealer,messages}.rs,
docs/aggregation-api.md): the typestates of the multi-party aggregation protocol over the stateless batched entry points
bpgpu_mpc_* (Context.mpc_* in _lib.py) -- every class here is a batch of one.  No arithmetic happens here.

    party:   Party.new(...) -> PartyAwaitingPosition.assign_position[_with_rng](j) -> (PartyAwaitingBitChallenge, BitCommitment)
             .apply_challenge[_with_rng](BitChallenge) -> (PartyAwaitingPolyChallenge, PolyCommitment)
             .apply_challenge(PolyChallenge) -> ProofShare
    dealer:  Dealer.new(...) -> DealerAwaitingBitCommitments.receive_bit_commitments([...]) -> (DealerAwaitingPolyCommitments, BitChallenge)
             .receive_poly_commitments([...]) -> (DealerAwaitingProofShares, PolyChallenge)
             .receive_shares[_with_rng]([...]) / .receive_trusted_shares([...]) -> RangeProof

Rust moves a state into its transition; here a state object is CONSUMED by it: a second use raises StateConsumed.  A party state
holds the library's opaque blob (the party's secrets); it is overwritten with zeros when the state is consumed or dropped, as the
reference zeroizes on Drop (party.rs:148-260)."""
from .api import FormatError, RangeProof

MPC_OK, MPC_MALICIOUS_DEALER, MPC_MALFORMED_SHARES, MPC_BAD_SCALAR, MPC_BAD_POINT = 0, 1, 2, 3, 4


class MPCError(Exception):
    """src/errors.rs:56-123.  The variants are subclasses, reachable as MPCError.<Variant>."""


def _variant(name, doc):
    cls = type(name, (MPCError,), {"__doc__": doc})
    setattr(MPCError, name, cls)
    return cls


_variant("MaliciousDealer", "the dealer sent a zero poly challenge (party.rs:283-285)")
_variant("InvalidBitsize", "n is not 8, 16, 32 or 64")
_variant("InvalidAggregation", "m is not a power of two")
_variant("InvalidGeneratorsLength", "the generators are too small for n, m or the position")
_variant("WrongNumBitCommitments", "the dealer was given other than m bit commitments")
_variant("WrongNumPolyCommitments", "the dealer was given other than m poly commitments")
_variant("WrongNumProofShares", "the dealer was given other than m proof shares")


class _Malformed(MPCError):
    """the aggregated proof does not verify: bad_shares lists the parties whose shares fail the audit (dealer.rs:303-335)"""

    def __init__(self, bad_shares):
        super().__init__("MalformedProofShares { bad_shares: %r }" % (list(bad_shares),))
        self.bad_shares = list(bad_shares)


_Malformed.__name__ = _Malformed.__qualname__ = "MalformedProofShares"
MPCError.MalformedProofShares = _Malformed


class StateConsumed(RuntimeError):
    """a typestate object was used after the transition that consumed it"""


# ---- messages (src/range_proof/messages.rs) -----------------------------------------------------------------------------------
class _Message:
    SIZE = None   # bytes; None: variable (ProofShare)

    def __init__(self, raw):
        raw = bytes(raw)
        self._check(raw)
        self._raw = raw

    @classmethod
    def _check(cls, raw):
        if len(raw) != cls.SIZE:
            raise FormatError()

    @classmethod
    def from_bytes(cls, raw):
        return cls(raw)

    def to_bytes(self):
        return self._raw

    def __eq__(self, other):
        return type(self) is type(other) and self._raw == other._raw

    def __hash__(self):
        return hash((type(self), self._raw))


class BitCommitment(_Message):
    """V_j, A_j, S_j (compressed), 96 bytes"""
    SIZE = 96
    V_j = property(lambda self: self._raw[:32])
    A_j = property(lambda self: self._raw[32:64])
    S_j = property(lambda self: self._raw[64:])


class BitChallenge(_Message):
    """y, z, 64 bytes"""
    SIZE = 64
    y = property(lambda self: self._raw[:32])
    z = property(lambda self: self._raw[32:])


class PolyCommitment(_Message):
    """T_1_j, T_2_j (compressed), 64 bytes"""
    SIZE = 64
    T_1_j = property(lambda self: self._raw[:32])
    T_2_j = property(lambda self: self._raw[32:])


class PolyChallenge(_Message):
    """x, 32 bytes"""
    SIZE = 32
    x = property(lambda self: self._raw)


class ProofShare(_Message):
    """t_x, t_x_blinding, e_blinding, l_vec[n], r_vec[n]: 32 (3 + 2n) bytes"""

    @classmethod
    def _check(cls, raw):
        if len(raw) % 32 or len(raw) < 32 * 5 or (len(raw) // 32 - 3) % 2:
            raise FormatError()

    @property
    def n(self):
        return (len(self._raw) // 32 - 3) // 2


# ---- shared typestate plumbing ---------------------------------------------------------------------------------------------------
def _check_shape(bp_gens, n, m=None):
    if n not in (8, 16, 32, 64):
        raise MPCError.InvalidBitsize()
    if m is not None and (m == 0 or m & (m - 1)):
        raise MPCError.InvalidAggregation()
    if bp_gens.gens_capacity < n or (m is not None and bp_gens.party_capacity < m):
        raise MPCError.InvalidGeneratorsLength()


def _seeded_kw(rng_bytes, rng_seed32, first_draw):
    """keywords of the seeded party calls (Context.mpc_party_*_commit) for a batch of one; {} when the step is not seeded"""
    if rng_seed32 is None and first_draw is None:
        return {}
    if rng_bytes is not None or (rng_seed32 is not None and len(rng_seed32) != 32):
        raise ValueError("rng_seed32: 32 bytes, and not together with rng_bytes")
    return {"rng_seed32": None if rng_seed32 is None else bytes(rng_seed32), "first_draw": None if first_draw is None else [int(first_draw)]}


class _State:
    _blob = None   # party states: the secret blob (bytearray)

    def _consume(self):
        if getattr(self, "_used", False):
            raise StateConsumed("%s was already consumed by a transition" % type(self).__name__)
        self._used = True

    def zeroize(self):
        b = self._blob
        if b is not None:
            b[:] = bytes(len(b))

    def __del__(self):
        try:
            self.zeroize()
        except Exception:
            pass


# ---- party (src/range_proof/party.rs) --------------------------------------------------------------------------------------------
class Party:
    @staticmethod
    def new(bp_gens, pc_gens, v, v_blinding, n):
        """Party::new (party.rs:37-60).  v: int (u64; a value beyond n bits is accepted, as upstream), v_blinding: 32-byte scalar."""
        _check_shape(bp_gens, n)
        if hasattr(bp_gens, "_check_pedersen"):
            bp_gens._check_pedersen(pc_gens)
        return PartyAwaitingPosition(bp_gens, int(v), bytes(v_blinding), n)


class PartyAwaitingPosition(_State):
    def __init__(self, bp_gens, v, v_blinding, n):
        self.bp_gens, self.n, self._v = bp_gens, n, v
        self._blob = bytearray(v_blinding)

    def assign_position_with_rng(self, j, rng_bytes=None, *, rng_seed32=None, first_draw=None):
        """party.rs:73-144.  rng_bytes: the 64 (2n + 2) bytes the rng would hand Scalar::random (a_blinding, s_blinding, s_L, s_R), or
        None for the OS CSPRNG.  rng_seed32 instead: the rng is ChaChaRng::from_seed(rng_seed32), its scalars drawn on the device
        (bpgpu_mpc_party_bit_commit_seeded), first_draw (default 0) the number of scalars it has handed out before this step -- j (2n + 2)
        for party j of a prove_multiple_with_rng.  Returns (PartyAwaitingBitChallenge, BitCommitment)."""
        kw = _seeded_kw(rng_bytes, rng_seed32, first_draw)
        self._consume()
        try:
            if self.bp_gens.party_capacity <= j:
                raise MPCError.InvalidGeneratorsLength()
            bc, st = self.bp_gens.ctx.mpc_party_bit_commit(self.n, [j], [self._v], bytes(self._blob), rng_bytes, **kw)
        finally:
            self.zeroize()
            self._v = 0
        return PartyAwaitingBitChallenge(self.bp_gens, self.n, j, st), BitCommitment(bc)

    def assign_position(self, j):
        return self.assign_position_with_rng(j, None)


class PartyAwaitingBitChallenge(_State):
    def __init__(self, bp_gens, n, j, blob):
        self.bp_gens, self.n, self.j, self._blob = bp_gens, n, j, blob

    def apply_challenge_with_rng(self, vc, rng_bytes=None, *, rng_seed32=None, first_draw=None):
        """party.rs:182-237.  rng_bytes: 128 bytes (t_1_blinding, t_2_blinding) or None.  rng_seed32 / first_draw as in assign_position_with_rng
        (bpgpu_mpc_party_poly_commit_seeded); first_draw defaults to 2n + 2, the rng carried on from assign_position_with_rng -- m (2n + 2) + 2j
        for party j of a prove_multiple_with_rng.  Returns (PartyAwaitingPolyChallenge, PolyCommitment)."""
        kw = _seeded_kw(rng_bytes, rng_seed32, first_draw)
        self._consume()
        try:
            pc, st, status = self.bp_gens.ctx.mpc_party_poly_commit(self.n, self._blob, vc.to_bytes(), rng_bytes, **kw)
        finally:
            self.zeroize()
        if status[0] != MPC_OK:
            raise FormatError()   # y or z is not a canonical scalar (upstream: Scalar by type)
        return PartyAwaitingPolyChallenge(self.bp_gens, self.n, self.j, st), PolyCommitment(pc)

    def apply_challenge(self, vc):
        return self.apply_challenge_with_rng(vc, None)


class PartyAwaitingPolyChallenge(_State):
    def __init__(self, bp_gens, n, j, blob):
        self.bp_gens, self.n, self.j, self._blob = bp_gens, n, j, blob

    def apply_challenge(self, pc):
        """party.rs:279-311: the ProofShare; MPCError.MaliciousDealer for a zero challenge."""
        self._consume()
        try:
            sh, status = self.bp_gens.ctx.mpc_party_proof_share(self.n, self._blob, pc.to_bytes())
        finally:
            self.zeroize()
        if status[0] == MPC_MALICIOUS_DEALER:
            raise MPCError.MaliciousDealer()
        if status[0] != MPC_OK:
            raise FormatError()
        return ProofShare(sh)


# ---- dealer (src/range_proof/dealer.rs) ------------------------------------------------------------------------------------------
class Dealer:
    @staticmethod
    def new(bp_gens, pc_gens, transcript, n, m):
        """Dealer::new (dealer.rs:37-76).  `transcript` (api.Transcript) is advanced in place by every step, as &mut Transcript is."""
        _check_shape(bp_gens, n, m)
        if hasattr(bp_gens, "_check_pedersen"):
            bp_gens._check_pedersen(pc_gens)
        return DealerAwaitingBitCommitments(bp_gens, transcript, n, m)


class _DealerState(_State):
    def _advance(self, state):
        self.transcript.state = state
        self.transcript.fresh_label = None


class DealerAwaitingBitCommitments(_DealerState):
    def __init__(self, bp_gens, transcript, n, m):
        self.bp_gens, self.transcript, self.n, self.m = bp_gens, transcript, n, m
        self.initial = transcript.state   # what Dealer::new clones for the final check (dealer.rs:57-60)

    def receive_bit_commitments(self, bit_commitments):
        """dealer.rs:93-137 -> (DealerAwaitingPolyCommitments, BitChallenge)"""
        if len(bit_commitments) != self.m:
            raise MPCError.WrongNumBitCommitments()
        self._consume()
        raw = b"".join(b.to_bytes() for b in bit_commitments)
        ch, sums, ts, status = self.bp_gens.ctx.mpc_dealer_bit_challenge(self.n, self.m, raw, transcripts=self.transcript.state)
        if status[0] != MPC_OK:
            raise FormatError()   # an A_j / S_j that is no point (upstream: RistrettoPoint by type)
        self._advance(ts)
        return DealerAwaitingPolyCommitments(self, raw, ch, sums), BitChallenge(ch)


class DealerAwaitingPolyCommitments(_DealerState):
    def __init__(self, prev, bit_commitments, bit_challenge, AS):
        self.bp_gens, self.transcript, self.n, self.m, self.initial = prev.bp_gens, prev.transcript, prev.n, prev.m, prev.initial
        self.bit_commitments, self.bit_challenge, self.A, self.S = bit_commitments, bit_challenge, AS[:32], AS[32:]

    def receive_poly_commitments(self, poly_commitments):
        """dealer.rs:160-197 -> (DealerAwaitingProofShares, PolyChallenge)"""
        if len(poly_commitments) != self.m:
            raise MPCError.WrongNumPolyCommitments()
        self._consume()
        raw = b"".join(p.to_bytes() for p in poly_commitments)
        x, _, ts, status = self.bp_gens.ctx.mpc_dealer_poly_challenge(self.m, raw, self.transcript.state)
        if status[0] != MPC_OK:
            raise FormatError()
        self._advance(ts)
        return DealerAwaitingProofShares(self, raw, x), PolyChallenge(x)


class DealerAwaitingProofShares(_DealerState):
    def __init__(self, prev, poly_commitments, x):
        self.bp_gens, self.transcript, self.n, self.m, self.initial = prev.bp_gens, prev.transcript, prev.n, prev.m, prev.initial
        self.bit_commitments, self.poly_commitments, self.challenges = prev.bit_commitments, poly_commitments, prev.bit_challenge + x

    def _assemble(self, proof_shares, rng64, trusted):
        if len(proof_shares) != self.m:
            raise MPCError.WrongNumProofShares()
        self._consume()
        wrong = [j for j, s in enumerate(proof_shares) if s.n != self.n]   # ProofShare::check_size (messages.rs:57-82)
        if wrong:
            raise MPCError.MalformedProofShares(wrong)
        raw = b"".join(s.to_bytes() for s in proof_shares)
        proof, bad, status, ts = self.bp_gens.ctx.mpc_dealer_assemble(self.n, self.m, raw, self.bit_commitments, self.poly_commitments, self.challenges,
                                                                       self.transcript.state, initial_transcripts=self.initial, rng64=rng64, trusted=trusted)
        self._advance(ts)
        if status[0] == MPC_MALFORMED_SHARES:
            raise MPCError.MalformedProofShares([j for j in range(self.m) if bad[j]])
        if status[0] != MPC_OK:
            raise FormatError()
        return RangeProof(proof)

    def receive_shares_with_rng(self, proof_shares, rng64=None):
        """dealer.rs:303-335: assemble, verify the aggregated proof, audit the shares when it does not verify.  rng64: the 64 bytes the
        verifier's Scalar::random would draw, or None."""
        return self._assemble(proof_shares, rng64, False)

    def receive_shares(self, proof_shares):
        return self._assemble(proof_shares, None, False)

    def receive_trusted_shares(self, proof_shares):
        """dealer.rs:352-380: no validation of the shares -- the proof may not verify."""
        return self._assemble(proof_shares, None, True)
