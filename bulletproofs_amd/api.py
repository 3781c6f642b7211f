"""Host-side mirror (Python) of the reference crate's verification API over the C ABI -- same names,
argument meaning and error behaviour as src/lib.rs:34-45 exports for this path (RangeProof,
BulletproofGens, PedersenGens, ProofError, Transcript).  The C++ twin is include/bulletproofs.hpp.
No arithmetic happens here: parsing checks lengths / scalar canonicity, everything else is one call
into libbpgpu.so.  There is no CPU fallback."""
from ._lib import BpgpuError, Context, ERR_NAMES, transcript_new, transcript_append_message, transcript_challenge_bytes

_L = 2**252 + 27742317777372353535851937790883648493


class ProofError(Exception):
    """src/errors.rs:12-54"""
    code = None

    def __eq__(self, other):
        return isinstance(other, ProofError) and type(self) is type(other)

    def __hash__(self):
        return hash(type(self))


class VerificationError(ProofError):
    code = 1


class FormatError(ProofError):
    code = 2


class InvalidBitsize(ProofError):
    code = 3


class InvalidGeneratorsLength(ProofError):
    code = 4


_BY_CODE = {c.code: c for c in (VerificationError, FormatError, InvalidBitsize, InvalidGeneratorsLength)}


class PedersenGens:
    """src/generators.rs:30-53; PedersenGens::default() as held by a BulletproofGens on the device."""

    def __init__(self, B, B_blinding):
        self.B, self.B_blinding = B, B_blinding


class BulletproofGens:
    """BulletproofGens::new(gens_capacity, party_capacity) (src/generators.rs:157-166), derived on the GPU."""

    def __init__(self, gens_capacity, party_capacity, device=0, **ctx_options):
        self.gens_capacity, self.party_capacity, self.device = gens_capacity, party_capacity, device
        self.ctx = Context(device, **ctx_options)
        self.ctx.gens_create(gens_capacity, party_capacity)

    def pedersen(self):
        _, _, B, Bb = self.ctx.gens_export()
        return PedersenGens(B, Bb)

    def increase_capacity(self, new_capacity):
        """generators.rs:177-204: extends every party's chain to new_capacity (no-op if not larger); the device tables are rebuilt."""
        if self.gens_capacity >= new_capacity:
            return
        # the Pedersen bases the context holds now (custom ones if the caller went through Context.gens_load) must survive the rebuild
        _, _, B0, Bb0 = self.ctx.gens_export()
        self.ctx.gens_create(new_capacity, self.party_capacity)
        G1, H1, B1, Bb1 = self.ctx.gens_export()
        if (B0, Bb0) != (B1, Bb1):          # custom bases were loaded: keep them, with the extended G / H chains
            self.ctx.gens_load(new_capacity, self.party_capacity, G1, H1, B0, Bb0)
        self.gens_capacity = new_capacity
        self.__dict__.pop("_pc", None)

    def _flat(self):
        G, H, _, _ = self.ctx.gens_export()
        return G, H

    def G(self, n, m):
        """the aggregated iterator of generators.rs:207-232: the first n generators of each of the first m parties, compressed"""
        G, _ = self._flat()
        c = self.gens_capacity
        return [G[32 * (j * c + i):32 * (j * c + i) + 32] for j in range(m) for i in range(n)]

    def H(self, n, m):
        _, H = self._flat()
        c = self.gens_capacity
        return [H[32 * (j * c + i):32 * (j * c + i) + 32] for j in range(m) for i in range(n)]

    def share(self, j):
        """BulletproofGens::share(j) (generators.rs:168-175): .G(n) / .H(n) of party j"""
        return BulletproofGensShare(self, j)


    def commit(self, value, blinding):
        """PedersenGens::commit(value, blinding) (generators.rs:38-42) with this context's bases: value B + blinding B_blinding,
        compressed.  value: int or 32-byte scalar; blinding: 32-byte scalar.  (Variable time on the GPU, unlike the reference's
        constant-time multiscalar_mul.)"""
        v = value.to_bytes(32, "little") if isinstance(value, int) else bytes(value)
        _, _, B, Bb = self.ctx.gens_export()
        out, st = self.ctx.msm_batch([2], v + bytes(blinding), B + Bb)
        if st != bytes(1):
            raise ValueError("scalars must be canonical")
        return out

    def commit_batch(self, values, blindings=None, rng_seed32=None, first_draw=0):
        """len(values) calls of PedersenGens::commit in ONE GPU launch (bpgpu_pedersen_commit_batch; no counterpart in the crate).
        values: ints below 2^64, or 32-byte scalars -- one kind per call.  blindings: 32-byte scalars, or None: blinding i is the
        (first_draw + i)-th Scalar::random of ChaChaRng::from_seed(rng_seed32), drawn on the device (rng_seed32 None: the library
        draws the seed).  Returns ([32-byte commitments], [32-byte blindings]).  Variable time unless the context option
        prover_constant_time is set; row i equals commit(values[i], blindings[i])."""
        values = list(values)
        ints = [isinstance(v, int) for v in values]
        if any(ints) and not all(ints):
            raise TypeError("commit_batch takes ints or 32-byte scalars, not both in one call")
        if values and all(ints):
            if any(v < 0 or v >> 64 for v in values):
                raise ValueError("integer values must be below 2^64 (pass larger ones as 32-byte scalars)")
            packed, vb = b"".join(v.to_bytes(8, "little") for v in values), 8
        else:
            packed, vb = b"".join(bytes(v) for v in values), 32
            if len(packed) != 32 * len(values):
                raise ValueError("scalar values must be 32 bytes each")
        if blindings is not None:
            blindings = [bytes(b) for b in blindings]
            if len(blindings) != len(values) or any(len(b) != 32 for b in blindings):
                raise ValueError("one 32-byte blinding per value")
            if rng_seed32 is not None or first_draw:
                raise ValueError("blindings given: rng_seed32 and first_draw do not apply")
        if not values:
            return [], []
        out, st, blo = self.ctx.pedersen_commit_batch(packed, vb, None if blindings is None else b"".join(blindings),
                                                      None if rng_seed32 is None else bytes(rng_seed32), first_draw, want_blindings=True)
        if st != bytes(len(values)):
            raise ValueError("scalars must be canonical (row %d)" % next(i for i, x in enumerate(st) if x))
        return [out[32 * i:32 * i + 32] for i in range(len(values))], [blo[32 * i:32 * i + 32] for i in range(len(values))]

    def verify_openings(self, commitments, values, blindings):
        """does (values[i], blindings[i]) open commitments[i]? (bpgpu_pedersen_open_batch) -> a list of None / ProofError:
        VerificationError when it does not (also for a commitment that is no valid encoding), FormatError for a non-canonical scalar."""
        values, commitments, blindings = list(values), [bytes(c) for c in commitments], [bytes(b) for b in blindings]
        if not (len(values) == len(commitments) == len(blindings)):
            raise ValueError("one commitment and one blinding per value")
        ints = [isinstance(v, int) for v in values]
        if any(ints) and not all(ints):
            raise TypeError("verify_openings takes ints or 32-byte scalars, not both in one call")
        if not values:
            return []
        if all(ints) and all(0 <= v < 2 ** 64 for v in values):
            packed, vb = b"".join(v.to_bytes(8, "little") for v in values), 8
        elif all(ints):
            raise ValueError("integer values must be below 2^64 (pass larger ones as 32-byte scalars)")
        else:
            packed, vb = b"".join(bytes(v) for v in values), 32
        vd = self.ctx.pedersen_open_batch(b"".join(commitments), packed, vb, b"".join(blindings))
        return [None if x == 0 else _BY_CODE[x]() for x in vd]

    @staticmethod
    def _signed_rows(plus, minus, values, blindings, who):
        """(row_offsets, points, signs, packed values or None, value_bytes, packed blindings or None) of bpgpu_pedersen_sum_batch"""
        plus = [[bytes(c) for c in row] for row in plus]
        minus = [[] for _ in plus] if minus is None else [[bytes(c) for c in row] for row in minus]
        if len(minus) != len(plus):
            raise ValueError("one list of subtracted commitments per row")
        off, pts, sg = [0], [], bytearray()
        for a, s in zip(plus, minus):
            if any(len(c) != 32 for c in a + s):
                raise ValueError("commitments are 32 bytes each")
            pts += a + s
            sg += bytes(len(a)) + bytes([1]) * len(s)
            off.append(len(pts))
        packed, vb = None, 8
        if values is not None:
            values = list(values)
            if len(values) != len(plus):
                raise ValueError("one value per row")
            ints = [isinstance(v, int) for v in values]
            if any(ints) and not all(ints):
                raise TypeError("%s takes ints or 32-byte scalars, not both in one call" % who)
            if values and all(ints):
                if any(v < 0 or v >> 64 for v in values):
                    raise ValueError("integer values must be below 2^64 (pass larger ones as 32-byte scalars)")
                packed = b"".join(v.to_bytes(8, "little") for v in values)
            else:
                packed, vb = b"".join(bytes(v) for v in values), 32
                if len(packed) != 32 * len(values):
                    raise ValueError("scalar values must be 32 bytes each")
        if blindings is not None:
            blindings = [bytes(b) for b in blindings]
            if len(blindings) != len(plus) or any(len(b) != 32 for b in blindings):
                raise ValueError("one 32-byte blinding per row")
            blindings = b"".join(blindings)
        return off, b"".join(pts), bytes(sg), packed, vb, blindings

    def sum_commitments(self, plus, minus=None, values=None, blindings=None):
        """Row r: sum(plus[r]) - sum(minus[r]) + values[r] B + blindings[r] B_blinding, compressed, for every row in a few GPU launches
        (bpgpu_pedersen_sum_batch; no counterpart in the crate).  plus, minus: lists of lists of 32-byte commitments, one inner list
        per row; values: ints below 2^64 or 32-byte scalars, one kind per call, or None; blindings: 32-byte scalars or None.  Returns a
        list of 32-byte encodings; an entry is None where a term of the row did not decode.  ValueError for a non-canonical scalar."""
        off, pts, sg, packed, vb, bl = self._signed_rows(plus, minus, values, blindings, "sum_commitments")
        nb = len(off) - 1
        if nb == 0:
            return []
        out, st = self.ctx.pedersen_sum_batch(off, pts, sg, packed, vb, bl)
        if 2 in st:
            raise ValueError("scalars must be canonical (row %d)" % st.index(2))
        return [None if st[i] else out[32 * i:32 * i + 32] for i in range(nb)]

    def verify_balance(self, inputs, outputs, values=None, blindings=None):
        """does sum(inputs[r]) - sum(outputs[r]) open to (values[r], blindings[r])? (bpgpu_pedersen_balance_batch) -> a list of None /
        ProofError, as verify_openings: VerificationError when the row does not balance (also for a commitment that is no valid
        encoding), FormatError for a non-canonical scalar.  A missing value or blinding is zero."""
        off, pts, sg, packed, vb, bl = self._signed_rows(inputs, outputs, values, blindings, "verify_balance")
        if len(off) == 1:
            return []
        vd = self.ctx.pedersen_balance_batch(off, pts, sg, packed, vb, bl)
        return [None if x == 0 else _BY_CODE[x]() for x in vd]

    def prove_balance(self, fees, excess_blindings, transcripts, inputs, outputs, rng_seed32=None):
        """The excess proofs of a block of confidential transactions: row r proves knowledge of the blinding of
        E_r = sum(inputs[r]) - sum(outputs[r]) - fees[r] B, which is excess_blindings[r] B_blinding when the row balances -- a Schnorr
        signature under the key E_r (OpeningProof with the public value 0).  fees: ints below 2^64.  `transcripts` as in
        OpeningProof.create_batch.  Returns [OpeningProof]; raises ValueError for a commitment that does not decode or a scalar that
        is not canonical.  The prover needs no fee-free row: E_r is computed here, on the GPU (bpgpu_pedersen_sum_batch)."""
        fees = [int(f) for f in fees]
        if any(f < 0 or f >> 64 for f in fees):
            raise ValueError("fees must be below 2^64")
        E = self.sum_commitments(inputs, outputs, values=[((_L - f) % _L).to_bytes(32, "little") for f in fees])
        if any(e is None for e in E):
            raise ValueError("a commitment does not decode (row %d)" % next(i for i, e in enumerate(E) if e is None))
        return OpeningProof.create_batch(self, transcripts, [0] * len(fees), excess_blindings, commitments=E, public_values=True, rng_seed32=rng_seed32)

    def verify_balance_proved(self, inputs, outputs, fees, proofs, transcripts):
        """The validator's side of prove_balance, without any secret: E_r = sum(inputs[r]) - sum(outputs[r]) - fees[r] B on the GPU
        (bpgpu_pedersen_sum_batch_dev with the value l - fee) goes as a device buffer straight into the combined check of the excess
        proofs (bpgpu_opening_verify_rlc_ts_dev, form OPENING_BLINDING, value 0); the excess never visits the host.  Returns a list of
        None / ProofError.  A list of transcripts or a TranscriptBatch is left advanced as OpeningProof.verify_batch leaves it."""
        import torch
        fees = [int(f) for f in fees]
        if any(f < 0 or f >> 64 for f in fees):
            raise ValueError("fees must be below 2^64")
        off, pts, sg, packed, vb, _ = self._signed_rows(inputs, outputs, [((_L - f) % _L).to_bytes(32, "little") for f in fees], None, "verify_balance_proved")
        nb = len(off) - 1
        raw, pl = OpeningProof._raw(proofs, 64)
        if len(proofs) != nb:
            raise ValueError("verify_balance_proved: one proof per row")
        if nb == 0:
            return []
        per_proof = _per_proof(transcripts)
        if per_proof and len(transcripts) != nb:
            raise ValueError("verify_balance_proved: one transcript per row")
        c = self.ctx
        dev = torch.device("cuda:%d" % self.device)
        up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
        new = lambda n: torch.zeros(n, dtype=torch.uint8, device=dev)
        d_pts, d_sg, d_val, d_pr = up(pts) if pts else new(4), up(sg) if sg else new(4), up(packed), up(raw)
        d_ts = up(_states_of(transcripts)) if per_proof else None
        d_E, d_st, d_vd, d_to = new(32 * nb), new(nb), new(nb), new(208 * nb)
        torch.cuda.synchronize(dev)
        ptr = lambda t: None if t is None else t.data_ptr()
        c.pedersen_sum_batch_dev(off, ptr(d_pts), ptr(d_sg), ptr(d_val), vb, None, ptr(d_E), ptr(d_st))
        shared = None if per_proof else transcripts.state
        c.opening_verify_rlc_ts_dev(1, nb, ptr(d_pr), pl, shared, ptr(d_ts), ptr(d_E), None, 8, None, ptr(d_vd), None, ptr(d_to))
        c.synchronize()
        vd = bytes(d_vd.cpu().numpy())
        if 5 in vd:   # the combination did not decide: proof by proof, still on the device
            c.opening_verify_batch_ts_dev(1, nb, ptr(d_pr), pl, shared, ptr(d_ts), ptr(d_E), None, 8, ptr(d_vd))
            c.synchronize()
            vd = bytes(d_vd.cpu().numpy())
        st = bytes(d_st.cpu().numpy())
        if per_proof:
            _advance_all(transcripts, bytes(d_to.cpu().numpy()))
        # a row whose sum did not decode has no key: never verified, whatever its proof says about the placeholder
        return [VerificationError() if st[i] else (None if vd[i] == 0 else _BY_CODE[vd[i]]()) for i in range(nb)]

    def _check_pedersen(self, pc_gens):
        """The verifier multiplies by pc_gens.B / B_blinding (mod.rs:439-440); the device tables hold the bases this
        BulletproofGens was created with.  A different PedersenGens must be loaded with Context.gens_load."""
        if pc_gens is None:
            return
        if not hasattr(self, "_pc"):
            self._pc = self.pedersen()
        if (bytes(pc_gens.B), bytes(pc_gens.B_blinding)) != (self._pc.B, self._pc.B_blinding):
            raise ValueError("pc_gens differs from the Pedersen bases held in the device tables (use Context.gens_load for custom bases)")


class BulletproofGensShare:
    """generators.rs:262-292"""

    def __init__(self, gens, share):
        self.gens, self.share_index = gens, share

    def G(self, n):
        G, _ = self.gens._flat()
        o = self.share_index * self.gens.gens_capacity
        return [G[32 * (o + i):32 * (o + i) + 32] for i in range(n)]

    def H(self, n):
        _, H = self.gens._flat()
        o = self.share_index * self.gens.gens_capacity
        return [H[32 * (o + i):32 * (o + i) + 32] for i in range(n)]


class Transcript:
    """merlin::Transcript: held as its 208-byte STROBE state (include/bpgpu.h BPGPU_TRANSCRIPT_BYTES), so a transcript
    that already absorbed application messages can be handed to the verifier, which leaves it advanced exactly as
    verify_multiple_with_rng(&mut transcript, ...) does (mod.rs:345-353)."""

    def __init__(self, label, _state=None):
        self.state = _state if _state is not None else transcript_new(bytes(label))
        self.fresh_label = bytes(label) if _state is None else None   # set while the transcript is exactly Transcript::new(label)

    def clone(self):
        t = Transcript(None, self.state)
        t.fresh_label = self.fresh_label
        return t

    def append_message(self, label, message):
        self.state = transcript_append_message(self.state, bytes(label), bytes(message))
        self.fresh_label = None

    def append_u64(self, label, x):
        self.append_message(label, int(x).to_bytes(8, "little"))

    def challenge_bytes(self, label, n):
        self.state, out = transcript_challenge_bytes(self.state, bytes(label), n)
        self.fresh_label = None
        return out


class TranscriptBatch:
    """n transcripts built and bound on the GPU (bpgpu_transcript_batch): the rows share their labels, the messages are per row.
    Appends are recorded and sent as ONE script -- by the next challenge, by states(), or when the batch is consumed: wherever a list
    of Transcript is accepted (RangeProof.verify_batch / verify_batch_combined / prove_batch / rewind_batch / scan_batch, LinearProof.create_batch / verify_batch /
    verify_batch_combined, OpeningProof.create_batch / verify_batch / verify_batch_combined, verify_balance_proved) a TranscriptBatch is, and is left advanced where the list would be.  batch[i] is row i as a Transcript (for
    the items of RangeProof.verify_mixed_combined, say)."""

    def __init__(self, ctx, label, n, _shared=None, _states=None):
        self.ctx = getattr(ctx, "ctx", ctx)
        self.n = int(n)
        self._label = bytes(label) if (_shared is None and _states is None) else None    # the start is Transcript::new(label) ...
        self._shared, self._states = _shared, _states                                    # ... or one state for all rows, or one per row
        self._pending = []

    @staticmethod
    def from_transcript(ctx, transcript, n):
        """n rows that all start from one bound Transcript (which is not advanced)"""
        return TranscriptBatch(ctx, None, n, _shared=bytes(transcript.state))

    @staticmethod
    def from_states(ctx, states):
        """rows from per-row states: a list of Transcript / 208-byte states, or their concatenation"""
        if not isinstance(states, (bytes, bytearray)):
            states = b"".join(bytes(getattr(t, "state", t)) for t in states)
        if len(states) % 208:
            raise ValueError("from_states: 208 bytes per row")
        return TranscriptBatch(ctx, None, len(states) // 208, _states=bytes(states))

    def __len__(self):
        return self.n

    def clone(self):
        t = TranscriptBatch(self.ctx, self._label, self.n, self._shared, self._states)
        t._pending = list(self._pending)
        return t

    def _rows(self, what, values, scalar_types):
        if isinstance(values, scalar_types):
            return values
        values = list(values)
        if len(values) != self.n:
            raise ValueError("%s: one value per row (%d), or a single one for all rows" % (what, self.n))
        return values

    def append_message(self, label, messages):
        """messages: a list of n bytes objects of any lengths, or one bytes object for all rows"""
        msgs = self._rows("append_message", messages, (bytes, bytearray, memoryview))
        self._pending.append(("append", bytes(label), bytes(msgs) if isinstance(msgs, (bytes, bytearray, memoryview)) else [bytes(m) for m in msgs]))

    def append_u64(self, label, xs):
        xs = self._rows("append_u64", xs, int)
        self._pending.append(("append_u64", bytes(label), xs if isinstance(xs, int) else [int(x) for x in xs]))

    def _flush(self, last=None):
        """the recorded appends (and one challenge behind them) as scripts of at most TS_MAX_OPS operations"""
        from ._lib import TS_MAX_OPS
        script = self._pending + ([last] if last else [])
        outs = []
        for lo in range(0, max(len(script), 1), TS_MAX_OPS):
            chunk = script[lo:lo + TS_MAX_OPS]
            if self._label is not None:
                st, o = self.ctx.transcript_batch(self.n, chunk, label=self._label)
            else:
                st, o = self.ctx.transcript_batch(self.n, chunk, states=self._shared if self._states is None else self._states)
            self._label, self._shared, self._states = None, None, st
            self._pending = self._pending[len(chunk):]      # (a call that raises keeps its appends recorded)
            outs += o
        return outs

    def challenge_bytes(self, label, n):
        """n challenge bytes per row -> list of bytes objects"""
        return self._flush(("challenge", bytes(label), int(n)))[0]

    def challenge_scalars(self, label):
        """the crate's challenge_scalar per row -> list of 32-byte canonical scalars"""
        return self._flush(("challenge_scalar", bytes(label)))[0]

    def states(self):
        """the rows' states, n x 208 bytes (what the `_ts` entry points take as `transcripts`)"""
        if self._pending or self._states is None:
            self._flush()
        return self._states

    def __getitem__(self, i):
        if not -self.n <= i < self.n:
            raise IndexError(i)
        i %= self.n
        return Transcript(None, self.states()[208 * i:208 * i + 208])

    def _advance(self, ts):
        self._label, self._shared, self._states, self._pending = None, None, bytes(ts[:208 * self.n]), []


def _per_proof(transcript):
    return isinstance(transcript, (list, tuple, TranscriptBatch))


def _states_of(transcripts):
    return transcripts.states() if isinstance(transcripts, TranscriptBatch) else b"".join(t.state for t in transcripts)


def _advance_all(transcripts, ts):
    """the callers' transcripts, one per proof, left as the call left them"""
    if isinstance(transcripts, TranscriptBatch):
        transcripts._advance(ts)
        return
    for i, t in enumerate(transcripts):
        t.state = ts[208 * i:208 * i + 208]
        t.fresh_label = None


class RangeProof:
    def __init__(self, raw):
        self._raw = raw

    @staticmethod
    def from_bytes(b):
        """src/range_proof/mod.rs:504-538 + src/inner_product_proof.rs:373-407; raises FormatError."""
        b = bytes(b)
        if len(b) % 32 != 0 or len(b) < 7 * 32:
            raise FormatError()
        ne = (len(b) - 7 * 32) // 32
        if ne < 2 or (ne - 2) % 2 != 0 or (ne - 2) // 2 >= 32:
            raise FormatError()
        for off in (128, 160, 192, len(b) - 64, len(b) - 32):
            if int.from_bytes(b[off:off + 32], "little") >= _L:
                raise FormatError()
        return RangeProof(b)

    def to_bytes(self):
        return self._raw

    @staticmethod
    def prove_multiple_with_rng(bp_gens, pc_gens, transcript, values, blindings, n, rng_bytes=None, rng_seed32=None):
        """RangeProof::prove_multiple_with_rng (mod.rs:234-288) on the GPU (variable time: see include/bpgpu.h).  values: ints,
        blindings: 32-byte scalars; rng_bytes: the bytes the rng would hand Scalar::random, in the reference's draw order
        (None = OS CSPRNG).  rng_seed32 instead: the rng is ChaChaRng::from_seed(rng_seed32), its scalars drawn on the device
        (bpgpu_rangeproof_prove_batch_ts).  Returns (RangeProof, [commitment bytes]); `transcript` is left advanced."""
        bp_gens._check_pedersen(pc_gens)
        m = len(values)
        if rng_seed32 is not None:
            if rng_bytes is not None or len(rng_seed32) != 32:
                raise ValueError("rng_seed32: 32 bytes, and not together with rng_bytes")
            proofs, coms, ts = bp_gens.ctx.rangeproof_prove_batch_ts(n, m, list(values), b"".join(blindings), transcript.state, bytes(rng_seed32),
                                                                   want_transcripts=True)
        else:
            proofs, coms, ts = bp_gens.ctx.rangeproof_prove_batch(n, m, list(values), b"".join(blindings), transcript=transcript.state, rng=rng_bytes,
                                                                want_transcripts=True)
        transcript.state = ts
        transcript.fresh_label = None
        return RangeProof(proofs), [coms[32 * j:32 * j + 32] for j in range(m)]

    @staticmethod
    def prove_single_with_rng(bp_gens, pc_gens, transcript, v, v_blinding, n, rng_bytes=None, rng_seed32=None):
        proof, coms = RangeProof.prove_multiple_with_rng(bp_gens, pc_gens, transcript, [v], [v_blinding], n, rng_bytes, rng_seed32)
        return proof, coms[0]

    @staticmethod
    def prove_batch(bp_gens, pc_gens, transcript, values, blindings, n, rng32=None, rewind=False, messages=None):
        """len(values) proofs in ONE GPU pass (bpgpu_rangeproof_prove_batch_ts; no counterpart in the crate): values[i] / blindings[i]
        are the m values / 32-byte blindings of proof i.  `transcript`: one bound Transcript, the start state of every proof (not
        advanced, as in verify_batch), or a list of transcripts, one per proof, each left advanced as prove_multiple_with_rng
        leaves it.  rng32: 32 bytes per proof, proof i's rng being ChaChaRng::from_seed(rng32[32 i:32 i + 32]) (None: the library
        draws the seeds).  Returns [(RangeProof, [commitment bytes])].
        rewind=True: rewindable proofs (bpgpu_rangeproof_prove_batch_rw; m = 1, rng32 required): whoever holds proof i's seed gets
        (value, blinding, message) back with rewind_batch.  messages: one 16-byte message per proof (None entries and messages=None:
        zero).  A seed must never serve two (commitment, transcript) pairs: see rewind_seeds."""
        if not values:
            return []
        bp_gens._check_pedersen(pc_gens)
        nb, m = len(values), len(values[0])
        if any(len(v) != m for v in values) or len(blindings) != nb or any(len(b) != m for b in blindings):
            raise ValueError("prove_batch: m values and m blindings per proof")
        per_proof = _per_proof(transcript)
        if per_proof and len(transcript) != nb:
            raise ValueError("prove_batch: one transcript per proof")
        states = _states_of(transcript) if per_proof else transcript.state
        if rewind:
            if m != 1 or rng32 is None:
                raise ValueError("prove_batch(rewind=True): one value per proof, and the seeds rng32")
            if messages is not None:
                if len(messages) != nb or any(x is not None and len(x) != 16 for x in messages):
                    raise ValueError("prove_batch(rewind=True): one 16-byte message (or None) per proof")
                messages = b"".join(bytes(16) if x is None else bytes(x) for x in messages)
            proofs, coms, ts = bp_gens.ctx.rangeproof_prove_batch_rw(n, m, [x for v in values for x in v], b"".join(x for b in blindings for x in b), states,
                                                                   rng32, messages, want_transcripts=True)
        else:
            if messages is not None:
                raise ValueError("prove_batch: messages go with rewind=True")
            proofs, coms, ts = bp_gens.ctx.rangeproof_prove_batch_ts(n, m, [x for v in values for x in v], b"".join(x for b in blindings for x in b), states,
                                                                   rng32, want_transcripts=True)
        if per_proof:
            _advance_all(transcript, ts)
        pl = len(proofs) // nb
        return [(RangeProof(proofs[pl * i:pl * i + pl]), [coms[32 * (m * i + j):32 * (m * i + j) + 32] for j in range(m)]) for i in range(nb)]

    @staticmethod
    def rewind_seeds(ctx, key32, commitments):
        """One seed per commitment from a 32-byte wallet key, derived on the GPU with TranscriptBatch (the derivation fixed in
        include/bpgpu.h): Transcript::new(b"bpgpu rewind seed v1"), append_message(b"key", key32), append_message(b"C", commitment_i),
        challenge_bytes(b"seed", 32).  Returns the seeds concatenated, 32 bytes per commitment: the rng32 of prove_batch(rewind=True)
        and the seeds of rewind_batch."""
        if len(key32) != 32 or any(len(c) != 32 for c in commitments):
            raise ValueError("rewind_seeds: a 32-byte key and 32-byte commitments")
        if not commitments:
            return b""
        t = TranscriptBatch(ctx, b"bpgpu rewind seed v1", len(commitments))
        t.append_message(b"key", bytes(key32))
        t.append_message(b"C", [bytes(c) for c in commitments])
        return b"".join(t.challenge_bytes(b"seed", 32))

    @staticmethod
    def rewind_batch(bp_gens, pc_gens, transcripts, proofs, commitments, n, seeds):
        """Rewind every (proofs[i], commitments[i]) under seeds[32 i:32 i + 32] in ONE GPU launch (bpgpu_rangeproof_rewind_batch; no
        counterpart in the crate).  `transcripts`: one bound Transcript, the start state of every row, or a list of transcripts or a
        TranscriptBatch, one per row; none is advanced.  Returns, per row, (value, 32-byte blinding, 16-byte message) when the row is
        the seed holder's own, else None.  Raises FormatError where a proof is one that from_bytes rejects.  This does NOT verify the
        proofs: a recovered message is only as good as the proof's verification."""
        if not proofs:
            return []
        bp_gens._check_pedersen(pc_gens)
        raw = [p.to_bytes() if isinstance(p, RangeProof) else bytes(p) for p in proofs]
        nb, ln = len(raw), len(raw[0])
        if any(len(r) != ln for r in raw) or len(commitments) != nb or any(len(c) != 32 for c in commitments) or len(seeds) != 32 * nb:
            raise ValueError("rewind_batch: proofs of one length, one 32-byte commitment and one 32-byte seed per proof")
        if ln != 32 * (9 + 2 * (int(n).bit_length() - 1)):
            raise FormatError()
        if _per_proof(transcripts) and len(transcripts) != nb:
            raise ValueError("rewind_batch: one transcript per proof")
        states = _states_of(transcripts) if _per_proof(transcripts) else transcripts.state
        from ._lib import REWIND_FORMAT, REWIND_OK
        st, vals, msgs, bls = bp_gens.ctx.rangeproof_rewind_batch(n, b"".join(raw), ln, b"".join(bytes(c) for c in commitments), states, bytes(seeds))
        if nb == 1:
            st = bytes(st)
        if any(x == REWIND_FORMAT for x in st):
            raise FormatError()
        return [(vals[i], bls[32 * i:32 * i + 32], msgs[16 * i:16 * i + 16]) if st[i] == REWIND_OK else None for i in range(nb)]

    @staticmethod
    def scan_batch(bp_gens, pc_gens, transcripts, proofs, commitments, n, keys):
        """Scan every (proofs[i], commitments[i]) under the wallet keys `keys` (a list of 32-byte keys, or their concatenation; at most
        1024) with ONE transcript replay per row (bpgpu_rangeproof_scan_batch; no counterpart in the crate): the seed of (key j,
        commitment i) is rewind_seeds' derivation, and the lowest key that passes the 2^192 test decides a row.  `transcripts` as in
        rewind_batch (a bound Transcript, a list, or a TranscriptBatch); none is advanced.  Returns (status, key_index, values, messages,
        blindings): per row the status byte (REWIND_OK / REWIND_NOT_FOUND), the index of the key that opens it (None unless OK), the
        value, the 16-byte message and the 32-byte blinding (0 / zero bytes unless OK).  Raises FormatError where a proof is one that
        from_bytes rejects.  This does NOT verify the proofs."""
        keys32 = bytes(keys) if isinstance(keys, (bytes, bytearray)) else b"".join(bytes(k) for k in keys)
        if not keys32 or len(keys32) % 32 or (not isinstance(keys, (bytes, bytearray)) and any(len(k) != 32 for k in keys)):
            raise ValueError("scan_batch: 32-byte keys, at least one")
        if not proofs:
            return b"", [], [], [], []
        bp_gens._check_pedersen(pc_gens)
        raw = [p.to_bytes() if isinstance(p, RangeProof) else bytes(p) for p in proofs]
        nb, ln = len(raw), len(raw[0])
        if any(len(r) != ln for r in raw) or len(commitments) != nb or any(len(c) != 32 for c in commitments):
            raise ValueError("scan_batch: proofs of one length and one 32-byte commitment per proof")
        if ln != 32 * (9 + 2 * (int(n).bit_length() - 1)):
            raise FormatError()
        if _per_proof(transcripts) and len(transcripts) != nb:
            raise ValueError("scan_batch: one transcript per proof")
        states = _states_of(transcripts) if _per_proof(transcripts) else transcripts.state
        from ._lib import REWIND_FORMAT, REWIND_OK
        st, ki, vals, msgs, bls = bp_gens.ctx.rangeproof_scan_batch(n, b"".join(raw), ln, b"".join(bytes(c) for c in commitments), states, keys32)
        st = bytes(st)
        if any(x == REWIND_FORMAT for x in st):
            raise FormatError()
        return (st, [ki[i] if st[i] == REWIND_OK else None for i in range(nb)], vals, [msgs[16 * i:16 * i + 16] for i in range(nb)],
                [bls[32 * i:32 * i + 32] for i in range(nb)])

    def rewind_single(self, bp_gens, pc_gens, transcript, V, n, seed32):
        """(value, blinding, message) of the commitment V if this proof was made rewindable under seed32 on `transcript` (which is not
        advanced), else None.  Raises FormatError as from_bytes would."""
        return RangeProof.rewind_batch(bp_gens, pc_gens, transcript, [self], [V], n, seed32)[0]

    @staticmethod
    def prove_multiple(bp_gens, pc_gens, transcript, values, blindings, n):
        """RangeProof::prove_multiple (mod.rs:290-311): prove_multiple_with_rng with thread_rng() -- here the OS CSPRNG"""
        return RangeProof.prove_multiple_with_rng(bp_gens, pc_gens, transcript, values, blindings, n, None)

    @staticmethod
    def prove_single(bp_gens, pc_gens, transcript, v, v_blinding, n):
        """RangeProof::prove_single (mod.rs:141-158)"""
        return RangeProof.prove_single_with_rng(bp_gens, pc_gens, transcript, v, v_blinding, n, None)

    def verify_multiple_with_rng(self, bp_gens, pc_gens, transcript, value_commitments, n, rng64):
        """Ok(()) -> returns None; Err(e) -> raises e.  rng64 = the 64 bytes Scalar::random(rng) would draw (mod.rs:396);
        None = thread_rng()."""
        m = len(value_commitments)
        bp_gens._check_pedersen(pc_gens)
        v, ts = bp_gens.ctx.rangeproof_verify_batch_ts(n, m, self._raw, len(self._raw), b"".join(value_commitments), transcript.state, rng64,
                                                       want_transcripts=True)
        transcript.state = ts   # &mut Transcript: left advanced
        transcript.fresh_label = None
        if v[0] != 0:
            raise _BY_CODE[v[0]]()

    def verify_multiple(self, bp_gens, pc_gens, transcript, value_commitments, n):
        return self.verify_multiple_with_rng(bp_gens, pc_gens, transcript, value_commitments, n, None)

    def verify_single_with_rng(self, bp_gens, pc_gens, transcript, V, n, rng64):
        return self.verify_multiple_with_rng(bp_gens, pc_gens, transcript, [V], n, rng64)

    def verify_single(self, bp_gens, pc_gens, transcript, V, n):
        return self.verify_multiple_with_rng(bp_gens, pc_gens, transcript, [V], n, None)

    @staticmethod
    def verify_batch(bp_gens, pc_gens, transcript, proofs, commitments, n, rng64=None):
        """proofs[i].verify_multiple(bp_gens, pc_gens, &mut transcript.clone(), &commitments[i], n) for all i in one GPU pass
        -> list of None / ProofError.  `transcript` itself is not advanced.  A list of transcripts or a TranscriptBatch, one per
        proof: proof i starts from its own; they are not advanced either."""
        if not proofs:
            return []
        bp_gens._check_pedersen(pc_gens)
        raw = [p.to_bytes() if isinstance(p, RangeProof) else bytes(p) for p in proofs]
        m, ln = len(commitments[0]), len(raw[0])
        assert all(len(r) == ln for r in raw) and all(len(c) == m for c in commitments)
        if _per_proof(transcript) and len(transcript) != len(raw):
            raise ValueError("verify_batch: one transcript per proof")
        states = _states_of(transcript) if _per_proof(transcript) else transcript.state
        v = bp_gens.ctx.rangeproof_verify_batch_ts(n, m, b"".join(raw), ln, b"".join(b"".join(c) for c in commitments), states, rng64)
        if len(raw) == 1:
            v = bytes(v)
        return [None if x == 0 else _BY_CODE[x]() for x in v]

    @staticmethod
    def verify_batch_combined(bp_gens, pc_gens, transcript, proofs, commitments, n, rng64=None, weights64=None):
        """The same verdicts through the batch-combined check (bpgpu_rangeproof_verify_rlc / _rlc_ts; no counterpart in the crate): one
        identity test per batch when every proof verifies, per-proof re-verification inside the call when not.  `transcript`: a fresh
        Transcript(label), replayed from its label; or a transcript the caller has already bound to its transaction or session, the
        start state of every proof; or a list of transcripts, one per proof, at whatever positions their histories left them.  The
        caller's transcripts are not advanced, as in verify_batch."""
        if not proofs:
            return []
        bp_gens._check_pedersen(pc_gens)
        raw = [p.to_bytes() if isinstance(p, RangeProof) else bytes(p) for p in proofs]
        m, ln = len(commitments[0]), len(raw[0])
        assert all(len(r) == ln for r in raw) and all(len(c) == m for c in commitments)
        flat, coms = b"".join(raw), b"".join(b"".join(c) for c in commitments)
        if _per_proof(transcript):
            if len(transcript) != len(raw):
                raise ValueError("verify_batch_combined: one transcript per proof")
            v, _, _ = bp_gens.ctx.rangeproof_verify_rlc_ts(n, m, flat, ln, coms, _states_of(transcript), rng64, weights64)
        elif transcript.fresh_label is None:
            v, _, _ = bp_gens.ctx.rangeproof_verify_rlc_ts(n, m, flat, ln, coms, transcript.state, rng64, weights64)
        else:
            v, _, _ = bp_gens.ctx.rangeproof_verify_rlc(n, m, flat, ln, coms, transcript.fresh_label, rng64, weights64)
        return [None if x == 0 else _BY_CODE[x]() for x in v]

    @staticmethod
    def verify_mixed_combined(bp_gens, pc_gens, items, rng64=None, weights64=None, bound_transcripts=False):
        """Proofs of mixed shapes through ONE batch-combined check (bpgpu_rangeproof_verify_rlc_mixed; no counterpart in the crate).
        items: [(transcript, proof, commitments, n)] in any order; fresh Transcript(label) items are grouped by (n, m, proof length,
        label).  bound_transcripts=True also takes transcripts the caller has already bound to a transaction or session: those items
        are grouped by (n, m, proof length), every proof starting from its own state, and combined by
        bpgpu_rangeproof_verify_rlc_mixed_ts (a check of their own beside the fresh items'); without it a bound transcript is a
        ValueError, as before.  rng64 / weights64: 64 bytes per item, in the order of `items` (each row follows its item through the
        regrouping).  The caller's transcripts are not advanced.  Returns None / ProofError per item, in the caller's order."""
        if not items:
            return []
        bp_gens._check_pedersen(pc_gens)
        ni = len(items)
        if rng64 is not None and len(rng64) != 64 * ni:
            raise ValueError("rng64 must hold 64 bytes per item")
        if weights64 is not None and len(weights64) != 64 * ni:
            raise ValueError("weights64 must hold 64 bytes per item")
        groups, order = {}, []
        for i, (transcript, proof, commitments, n) in enumerate(items):
            label = transcript.fresh_label
            if label is None and not bound_transcripts:
                raise ValueError("verify_mixed_combined needs a fresh Transcript(label) per item unless bound_transcripts=True")
            raw = proof.to_bytes() if isinstance(proof, RangeProof) else bytes(proof)
            key = (label is None, n, len(commitments), len(raw), b"" if label is None else bytes(label))
            if key not in groups:
                groups[key] = []
                order.append(key)
            groups[key].append((i, raw, b"".join(commitments), transcript.state))
        out = [None] * ni
        for bound in (False, True):
            keys = [key for key in order if key[0] == bound]
            if not keys:
                continue
            index = [g[0] for key in keys for g in groups[key]]   # call position -> item
            call = [(key[1], key[2], b"".join(g[1] for g in groups[key]), key[3], b"".join(g[2] for g in groups[key]),
                     b"".join(g[3] for g in groups[key]) if bound else key[4]) for key in keys]
            rows = lambda buf: None if buf is None else b"".join(buf[64 * i:64 * i + 64] for i in index)
            fn = bp_gens.ctx.rangeproof_verify_rlc_mixed_ts if bound else bp_gens.ctx.rangeproof_verify_rlc_mixed
            v = fn(call, rows(rng64), rows(weights64))[0]
            for pos, i in enumerate(index):
                out[i] = None if v[pos] == 0 else _BY_CODE[v[pos]]()
        return out


class LinearProof:
    """src/linear_proof.rs (`pub use` lib.rs:36): the proof that <a, b> = c for a committed secret vector a and a public
    vector b.  Verification runs on the device (bpgpu_linear_verify_batch)."""

    def __init__(self, raw):
        self._raw = raw

    @staticmethod
    def from_bytes(b):
        """linear_proof.rs:350-394; raises FormatError."""
        b = bytes(b)
        ne = len(b) // 32
        if len(b) % 32 != 0 or ne < 3 or (ne - 3) % 2 != 0 or (ne - 3) // 2 >= 32:
            raise FormatError()
        for off in (len(b) - 64, len(b) - 32):
            if int.from_bytes(b[off:off + 32], "little") >= _L:
                raise FormatError()
        return LinearProof(b)

    def to_bytes(self):
        return self._raw

    def serialized_size(self):
        return len(self._raw)

    @staticmethod
    def create(transcript, rng_bytes, C, r, a_vec, b_vec, G_vec, F, B, ctx, rng_seed32=None):
        """LinearProof::create(transcript, rng, &C, r, a_vec, b_vec, G_vec, &F, &B) (linear_proof.rs:40-173) on the GPU (variable
        time, like the reference's).  rng_bytes: the 64 * (2 lg n + 2) bytes the rng would yield to Scalar::random, or None for
        the OS CSPRNG.  rng_seed32 instead: the rng is ChaChaRng::from_seed(rng_seed32), its scalars drawn on the device
        (bpgpu_linear_create_batch_ts).  The transcript is left advanced.  Raises ValueError for InvalidInputLength /
        InvalidGeneratorsLength."""
        c = getattr(ctx, "ctx", ctx)
        n = len(b_vec)
        if len(G_vec) != n:
            raise InvalidGeneratorsLength()
        if len(a_vec) != n or n == 0 or n & (n - 1):
            raise ValueError("InvalidInputLength")
        a, b, G = b"".join(bytes(x) for x in a_vec), b"".join(bytes(x) for x in b_vec), b"".join(bytes(g) for g in G_vec)
        if rng_seed32 is not None:
            if rng_bytes is not None or len(rng_seed32) != 32:
                raise ValueError("rng_seed32: 32 bytes, and not together with rng_bytes")
            proofs, status, ts = c.linear_create_batch_ts(n, transcript.state, bytes(C), bytes(r), a, b, G, bytes(F), bytes(B), rng32=bytes(rng_seed32),
                                                          want_transcripts=True)
        else:
            proofs, status, ts = c.linear_create_batch(n, bytes(C), bytes(r), a, b, G, bytes(F), bytes(B), transcript=transcript.state, rng=rng_bytes,
                                                       want_transcripts=True)
        if status[0] != 0:
            raise ValueError("an input point does not decode or a scalar is not canonical")
        transcript.state = ts
        transcript.fresh_label = None
        return LinearProof(proofs)

    def verify(self, transcript, C, G, F, B, b_vec, ctx):
        """LinearProof::verify(&self, transcript, C, G, F, B, b_vec) (linear_proof.rs:175-236): Ok(()) -> None, Err(e) -> raises e.
        C, F, B and the entries of G are 32-byte compressed points, b_vec 32-byte canonical scalars; ctx: the Context (or a
        BulletproofGens) whose device runs the check.  The transcript is left advanced as the reference leaves it when the proof
        is accepted; after an Err its state is unspecified (upstream has absorbed part of the public inputs at that point, this
        engine returns the state right after innerproduct_domain_sep(n) -- INTEGRATION.md 3c)."""
        c = getattr(ctx, "ctx", ctx)
        if len(G) != len(b_vec):
            raise InvalidGeneratorsLength()
        v, ts = c.linear_verify_batch(len(b_vec), self._raw, len(self._raw), bytes(C), b"".join(bytes(g) for g in G), bytes(F), bytes(B),
                                      b"".join(bytes(x) for x in b_vec), transcript=transcript.state, want_transcripts=True)
        transcript.state = ts
        transcript.fresh_label = None
        if v[0] != 0:
            raise _BY_CODE[v[0]]()

    @staticmethod
    def create_batch(ctx, transcripts, Cs, rs, a_vecs, b_vecs, G, F, B, rng_seed32=None):
        """len(Cs) proofs in ONE GPU pass (bpgpu_linear_create_batch_ts; no counterpart in the crate).  `transcripts`: one bound Transcript,
        the start state of every proof (not advanced), or a list of transcripts, one per proof, each left advanced as create() leaves
        it.  a_vecs: one secret vector per proof; b_vecs: one public vector per proof, or a single vector shared by all.
        rng_seed32: 32 bytes per proof, proof i's rng being ChaChaRng::from_seed(rng_seed32[32 i:32 i + 32]) (None: the library draws
        the seeds).  Returns [LinearProof]; raises ValueError when an input of some proof does not decode or is not canonical."""
        c = getattr(ctx, "ctx", ctx)
        if not Cs:
            return []
        nb, n = len(Cs), len(G)
        per_proof = _per_proof(transcripts)
        if per_proof and len(transcripts) != nb:
            raise ValueError("create_batch: one transcript per proof")
        if len(rs) != nb or len(a_vecs) != nb or any(len(a) != n for a in a_vecs) or n == 0 or n & (n - 1):
            raise ValueError("InvalidInputLength")
        shared = len(b_vecs) == n and isinstance(b_vecs[0], (bytes, bytearray))
        b = b"".join(bytes(x) for x in b_vecs) if shared else b"".join(b"".join(bytes(x) for x in v) for v in b_vecs)
        states = _states_of(transcripts) if per_proof else transcripts.state
        proofs, status, ts = c.linear_create_batch_ts(n, states, b"".join(bytes(x) for x in Cs), b"".join(bytes(x) for x in rs),
                                                      b"".join(b"".join(bytes(x) for x in a) for a in a_vecs), b, b"".join(bytes(g) for g in G), bytes(F),
                                                      bytes(B), rng32=rng_seed32, want_transcripts=True)
        if any(status):
            raise ValueError("an input point does not decode or a scalar is not canonical (proof %d)" % next(i for i, x in enumerate(status) if x))
        if per_proof:
            _advance_all(transcripts, ts)
        pl = len(proofs) // nb
        return [LinearProof(proofs[pl * i:pl * i + pl]) for i in range(nb)]

    @staticmethod
    def _batch_args(proofs, Cs, G, b_vecs):
        raw = [p.to_bytes() if isinstance(p, LinearProof) else bytes(p) for p in proofs]
        ln, n = len(raw[0]), len(G)
        assert all(len(r) == ln for r in raw)
        shared = len(b_vecs) == n and isinstance(b_vecs[0], (bytes, bytearray))
        b = b"".join(bytes(x) for x in b_vecs) if shared else b"".join(b"".join(bytes(x) for x in v) for v in b_vecs)
        return n, b"".join(raw), ln, b"".join(bytes(x) for x in Cs), b"".join(bytes(g) for g in G), b

    @staticmethod
    def verify_batch(ctx, transcript, proofs, Cs, G, F, B, b_vecs):
        """proofs[i].verify(&mut transcript.clone(), &Cs[i], G, F, B, b_vecs[i]) for all i in one GPU pass -> list of None /
        ProofError.  b_vecs: one vector per proof, or a single vector (list of scalars) shared by all.  `transcript`: one Transcript, the
        start state of every proof (not advanced), or a list of transcripts, one per proof (bpgpu_linear_verify_batch_ts), each left as
        verify() leaves it (after an Err: the state right after innerproduct_domain_sep(n), as in verify())."""
        c = getattr(ctx, "ctx", ctx)
        if not proofs:
            return []
        n, raw, ln, cs, g, b = LinearProof._batch_args(proofs, Cs, G, b_vecs)
        if _per_proof(transcript):
            if len(transcript) != len(proofs):
                raise ValueError("verify_batch: one transcript per proof")
            v, ts = c.linear_verify_batch_ts(n, raw, ln, _states_of(transcript), cs, g, bytes(F), bytes(B), b, want_transcripts=True)
            _advance_all(transcript, ts)
        else:
            v = c.linear_verify_batch(n, raw, ln, cs, g, bytes(F), bytes(B), b, transcript=transcript.state)
        return [None if x == 0 else _BY_CODE[x]() for x in v]

    @staticmethod
    def verify_batch_combined(ctx, transcript, proofs, Cs, G, F, B, b_vecs, weights64=None):
        """verify_batch's arguments and verdicts through the batch-combined check (bpgpu_linear_verify_rlc / _rlc_ts; no counterpart in
        the crate): one identity test per batch when every proof verifies, per-proof re-verification inside the call when not.
        weights64: 64 bytes per proof, unpredictable to the provers, or None (drawn by the library).  A list of transcripts, one per
        proof, is left advanced as in verify_batch."""
        c = getattr(ctx, "ctx", ctx)
        if not proofs:
            return []
        n, raw, ln, cs, g, b = LinearProof._batch_args(proofs, Cs, G, b_vecs)
        if _per_proof(transcript):
            if len(transcript) != len(proofs):
                raise ValueError("verify_batch_combined: one transcript per proof")
            v, _, _, ts = c.linear_verify_rlc_ts(n, raw, ln, _states_of(transcript), cs, g, bytes(F), bytes(B), b, weights64=weights64,
                                                 want_transcripts=True)
            _advance_all(transcript, ts)
        else:
            v, _, _ = c.linear_verify_rlc(n, raw, ln, cs, g, bytes(F), bytes(B), b, transcript=transcript.state, weights64=weights64)
        return [None if x == 0 else _BY_CODE[x]() for x in v]


class OpeningProof:
    """A proof of knowledge of the opening of a Pedersen commitment C = v B + r B_blinding under the context's bases (no counterpart in the
    crate; the protocol is fixed in include/bpgpu.h, bpgpu_opening_*).  Two forms: both v and r secret (96 bytes: R | s_v | s_r), or
    `public_values` -- v is known to the verifier, only r is secret (64 bytes: R | s_r); with v = 0 that is a Schnorr signature under
    the key C, the excess proof of a confidential transaction.  `transcripts` everywhere: one bound Transcript, the start state of
    every proof (not advanced), or a list of transcripts / a TranscriptBatch, one per proof, each left advanced."""

    def __init__(self, raw):
        self._raw = raw

    @staticmethod
    def from_bytes(b):
        """raises FormatError for a length other than 64 or 96 or a scalar that is not canonical"""
        b = bytes(b)
        if len(b) not in (64, 96):
            raise FormatError()
        for off in range(32, len(b), 32):
            if int.from_bytes(b[off:off + 32], "little") >= _L:
                raise FormatError()
        return OpeningProof(b)

    def to_bytes(self):
        return self._raw

    def serialized_size(self):
        return len(self._raw)

    @staticmethod
    def _raw(proofs, proof_len=None):
        raw = [p.to_bytes() if isinstance(p, OpeningProof) else bytes(p) for p in proofs]
        ln = proof_len if proof_len is not None else (len(raw[0]) if raw else 96)
        if any(len(r) != ln for r in raw):
            raise ValueError("every proof of a call has one form: %d bytes" % ln)
        return b"".join(raw), ln

    @staticmethod
    def _values(values, who):
        """ints below 2^64 or 32-byte scalars, one kind per call -> (packed, value_bytes)"""
        values = list(values)
        ints = [isinstance(v, int) for v in values]
        if any(ints) and not all(ints):
            raise TypeError("%s takes ints or 32-byte scalars, not both in one call" % who)
        if all(ints):
            if any(v < 0 or v >> 64 for v in values):
                raise ValueError("integer values must be below 2^64 (pass larger ones as 32-byte scalars)")
            return b"".join(v.to_bytes(8, "little") for v in values), 8
        packed = b"".join(bytes(v) for v in values)
        if len(packed) != 32 * len(values):
            raise ValueError("scalar values must be 32 bytes each")
        return packed, 32

    @staticmethod
    def create_batch(bp_gens, transcripts, values, blindings, commitments=None, public_values=False, rng_seed32=None):
        """len(values) proofs in ONE GPU launch (bpgpu_opening_create_batch_ts).  commitments: the 32-byte commitments the proofs are
        about, or None: they are made here with bp_gens.commit_batch(values, blindings).  rng_seed32: 32 bytes per proof, the seed of
        its ChaChaRng (None: the library draws them) -- never one seed for two statements or transcripts.  Returns [OpeningProof]
        (with commitments=None: ([OpeningProof], [commitments])); raises ValueError for a scalar that is not canonical."""
        c = getattr(bp_gens, "ctx", bp_gens)
        values, blindings = list(values), [bytes(b) for b in blindings]
        nb = len(values)
        if len(blindings) != nb or any(len(b) != 32 for b in blindings):
            raise ValueError("one 32-byte blinding per value")
        made = commitments is None
        if nb == 0:
            return ([], []) if made else []
        if made:
            commitments, _ = bp_gens.commit_batch(values, blindings)
        commitments = [bytes(x) for x in commitments]
        if len(commitments) != nb or any(len(x) != 32 for x in commitments):
            raise ValueError("one 32-byte commitment per value")
        per_proof = _per_proof(transcripts)
        if per_proof and len(transcripts) != nb:
            raise ValueError("create_batch: one transcript per proof")
        packed, vb = OpeningProof._values(values, "create_batch")
        states = _states_of(transcripts) if per_proof else transcripts.state
        form = 1 if public_values else 0
        proofs, status, ts = c.opening_create_batch_ts(form, states, b"".join(commitments), packed, vb, b"".join(blindings),
                                                       rng32=None if rng_seed32 is None else bytes(rng_seed32), want_transcripts=True)
        if any(status):
            raise ValueError("scalars must be canonical (proof %d)" % next(i for i, x in enumerate(status) if x))
        if per_proof:
            _advance_all(transcripts, ts)
        pl = len(proofs) // nb
        out = [OpeningProof(proofs[pl * i:pl * i + pl]) for i in range(nb)]
        return (out, commitments) if made else out

    @staticmethod
    def _verify(bp_gens, transcripts, proofs, commitments, public_values, combined, weights64):
        c = getattr(bp_gens, "ctx", bp_gens)
        if not proofs:
            return []
        form = 0 if public_values is None else 1
        raw, pl = OpeningProof._raw(proofs, 96 if form == 0 else 64)
        commitments = b"".join(bytes(x) for x in commitments)
        if len(commitments) != 32 * len(proofs):
            raise ValueError("one 32-byte commitment per proof")
        packed, vb = (None, 8) if public_values is None else OpeningProof._values(public_values, "verify_batch")
        if packed is not None and len(packed) != vb * len(proofs):
            raise ValueError("one public value per proof")
        per_proof = _per_proof(transcripts)
        if per_proof and len(transcripts) != len(proofs):
            raise ValueError("verify_batch: one transcript per proof")
        states = _states_of(transcripts) if per_proof else transcripts.state
        if combined:
            v, _, _, ts = c.opening_verify_rlc_ts(form, raw, pl, states, commitments, packed, vb, weights64=weights64, want_transcripts=True)
        else:
            v, ts = c.opening_verify_batch_ts(form, raw, pl, states, commitments, packed, vb, want_transcripts=True)
        if per_proof:
            _advance_all(transcripts, ts)
        return [None if x == 0 else _BY_CODE[x]() for x in v]

    @staticmethod
    def verify_batch(bp_gens, transcripts, proofs, commitments, public_values=None):
        """Every proof on its own (bpgpu_opening_verify_batch_ts) -> list of None / ProofError.  public_values: None for proofs with
        a secret value (96 bytes), else the public values (ints below 2^64 or 32-byte scalars) of 64-byte proofs."""
        return OpeningProof._verify(bp_gens, transcripts, proofs, commitments, public_values, False, None)

    @staticmethod
    def verify_batch_combined(bp_gens, transcripts, proofs, commitments, public_values=None, weights64=None):
        """verify_batch's arguments and verdicts through ONE combined check (bpgpu_opening_verify_rlc_ts): one multiscalar
        multiplication over two points per proof when every proof verifies, per-proof re-verification inside the call when not.
        weights64: 64 bytes per proof, unpredictable to the provers, or None (drawn by the library)."""
        return OpeningProof._verify(bp_gens, transcripts, proofs, commitments, public_values, True, weights64)

    @staticmethod
    def create(bp_gens, transcript, value, blinding, commitment, public_value=False, rng_seed32=None):
        """one proof; the transcript is left advanced.  Raises ValueError for a scalar that is not canonical."""
        return OpeningProof.create_batch(bp_gens, [transcript], [value], [blinding], commitments=[commitment], public_values=public_value,
                                         rng_seed32=rng_seed32)[0]

    def verify(self, bp_gens, transcript, commitment, public_value=None):
        """Ok(()) -> None, Err(e) -> raises e (a ProofError).  The transcript is left advanced as the contract of bpgpu_opening_* says."""
        e = OpeningProof.verify_batch(bp_gens, [transcript], [self], [commitment], None if public_value is None else [public_value])[0]
        if e is not None:
            raise e


class _SigmaSecret(int):
    """a secret scalar of a SigmaStatement, by index"""


class _SigmaBase(int):
    """a base of a SigmaStatement, by its id (0 B_blinding, 1 B, 2 + i G_i, 16 + p instance slot p)"""


class SigmaStatement:
    """A linear relation between points, written once (no counterpart in the crate; the `zkp` crate's pattern next to it): secrets, instance
    points and equations  point = sum secret * base , where a base is B, B_blinding or G(i) of bp_gens or another instance point.
    compile() records it on the GPU context (bpgpu_sigma_relation_create) and returns the SigmaRelation that proves and verifies batches.
        st = SigmaStatement(bp_gens); x = st.secret(); A, H, Bp = st.point(), st.point(), st.point()
        st.equation(A, [(x, st.B)]); st.equation(H, [(x, Bp)]); dleq = st.compile()
    At most 8 secrets, 8 points, 8 equations of 8 terms, 32 terms in all.  Public scalar coefficients are not part of a relation: fold them
    into an instance point first (sum_commitments)."""

    def __init__(self, bp_gens):
        self._gens = bp_gens
        self._S = self._P = 0
        self._eqs = []
        self.B_blinding, self.B = _SigmaBase(0), _SigmaBase(1)

    def secret(self):
        self._S += 1
        return _SigmaSecret(self._S - 1)

    def point(self):
        self._P += 1
        return _SigmaBase(16 + self._P - 1)

    def G(self, i):
        if not 0 <= i < 8:
            raise ValueError("G(i): i in 0 .. 7")
        return _SigmaBase(2 + i)

    def equation(self, lhs, terms):
        terms = list(terms)
        if not isinstance(lhs, _SigmaBase) or lhs < 16:
            raise TypeError("the left-hand side is an instance point (from .point())")
        if any(not isinstance(s, _SigmaSecret) or not isinstance(b, _SigmaBase) for s, b in terms):
            raise TypeError("terms are (secret, base) pairs")
        self._eqs.append((int(lhs), [(int(s), int(b)) for s, b in terms]))

    def descriptor(self):
        """the canonical bytes of include/bpgpu.h"""
        if max(self._S, self._P, len(self._eqs)) > 255 or any(len(t) > 255 for _, t in self._eqs):
            raise ValueError("a relation has at most 8 secrets, 8 points and 8 equations of 8 terms")
        out = bytearray([self._S, self._P, len(self._eqs)])
        for lhs, terms in self._eqs:
            out += bytes([lhs, len(terms)]) + b"".join(bytes(t) for t in terms)
        return bytes(out)

    def compile(self):
        """raises ValueError for what bpgpu_sigma_relation_create refuses (a count out of range, an unused secret or point, a G(i) beyond
        the generators)"""
        return SigmaRelation(self._gens, self.descriptor())


class SigmaRelation:
    """A recorded relation (SigmaStatement.compile, or canonical descriptor bytes).  A proof is T_1 | .. | T_E | s_1 | .. | s_S, 32 (E + S)
    bytes.  `transcripts` everywhere: one bound Transcript, the start state of every proof (not advanced), or a list of transcripts / a
    TranscriptBatch, one per proof, each left advanced.  secrets: per row S scalars (ints below the group order or 32-byte strings);
    points: per row P 32-byte encodings, slot order."""

    def __init__(self, bp_gens, descriptor):
        self._ctx = getattr(bp_gens, "ctx", bp_gens)
        self.descriptor = bytes(descriptor)
        try:
            self._h, self.S, self.P, self.E, self.digest = self._ctx.sigma_relation_create(self.descriptor)
        except BpgpuError as e:
            if str(e).startswith(ERR_NAMES[-1]):
                raise ValueError(str(e)) from None
            raise
        self.proof_len = 32 * (self.E + self.S)

    def close(self):
        if self._h is not None:
            self._ctx.sigma_relation_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _shape(self):
        return (self.S, self.P, self.E)

    def _points(self, points, nb=None):
        rows = [[bytes(x) for x in row] for row in points]
        if any(len(row) != self.P or any(len(x) != 32 for x in row) for row in rows) or (nb is not None and len(rows) != nb):
            raise ValueError("%d 32-byte points per row" % self.P)
        return b"".join(b"".join(row) for row in rows), len(rows)

    def create_batch(self, transcripts, secrets, points, rng_seed32=None):
        """len(points) proofs (bpgpu_sigma_create_batch_ts) -> [bytes].  rng_seed32: 32 bytes per row, the seed of its ChaChaRng (None: the
        library draws them) -- never one seed for two statements or transcripts.  Raises ValueError for a secret that is not canonical
        or an instance base that does not decode."""
        pts, nb = self._points(points)
        rows = [[int(x).to_bytes(32, "little") if isinstance(x, int) else bytes(x) for x in row] for row in secrets]
        if len(rows) != nb or any(len(row) != self.S or any(len(x) != 32 for x in row) for row in rows):
            raise ValueError("%d 32-byte secrets per row" % self.S)
        if nb == 0:
            return []
        per_proof = _per_proof(transcripts)
        if per_proof and len(transcripts) != nb:
            raise ValueError("create_batch: one transcript per proof")
        states = _states_of(transcripts) if per_proof else transcripts.state
        proofs, status, ts = self._ctx.sigma_create_batch_ts(self._h, self._shape(), states, pts, b"".join(b"".join(row) for row in rows),
                                                             rng32=None if rng_seed32 is None else bytes(rng_seed32), want_transcripts=True)
        if any(status):
            i = next(i for i, x in enumerate(status) if x)
            raise ValueError(("secrets must be canonical (row %d)" if status[i] == 2 else "an instance base does not decode (row %d)") % i)
        if per_proof:
            _advance_all(transcripts, ts)
        return [proofs[self.proof_len * i:self.proof_len * (i + 1)] for i in range(nb)]

    def _verify(self, transcripts, proofs, points, combined, weights64):
        proofs = [bytes(p) for p in proofs]
        if not proofs:
            return []
        if any(len(p) != self.proof_len for p in proofs):
            raise ValueError("a proof of this relation has %d bytes" % self.proof_len)
        pts, _ = self._points(points, len(proofs))
        per_proof = _per_proof(transcripts)
        if per_proof and len(transcripts) != len(proofs):
            raise ValueError("verify_batch: one transcript per proof")
        states = _states_of(transcripts) if per_proof else transcripts.state
        if combined:
            v, _, _, ts = self._ctx.sigma_verify_rlc_ts(self._h, self._shape(), b"".join(proofs), states, pts, weights64=weights64, want_transcripts=True)
        else:
            v, ts = self._ctx.sigma_verify_batch_ts(self._h, self._shape(), b"".join(proofs), states, pts, want_transcripts=True)
        if per_proof:
            _advance_all(transcripts, ts)
        return [None if x == 0 else _BY_CODE[x]() for x in v]

    def verify_batch(self, transcripts, proofs, points):
        """Every proof on its own (bpgpu_sigma_verify_batch_ts) -> list of None / ProofError."""
        return self._verify(transcripts, proofs, points, False, None)

    def verify_batch_combined(self, transcripts, proofs, points, weights64=None):
        """verify_batch's arguments and verdicts through ONE combined check (bpgpu_sigma_verify_rlc_ts): one multiscalar multiplication
        over P + E points per proof when every proof verifies, per-proof re-verification inside the call when not.  weights64: 64 bytes
        per (proof, equation), unpredictable to the provers, or None (drawn by the library)."""
        return self._verify(transcripts, proofs, points, True, weights64)

    def create(self, transcript, secrets, points, rng_seed32=None):
        """one proof; the transcript is left advanced"""
        return self.create_batch([transcript], [secrets], [points], rng_seed32=rng_seed32)[0]

    def verify(self, transcript, proof, points):
        """Ok(()) -> None, Err(e) -> raises e (a ProofError).  The transcript is left advanced."""
        e = self.verify_batch([transcript], [proof], [points])[0]
        if e is not None:
            raise e
