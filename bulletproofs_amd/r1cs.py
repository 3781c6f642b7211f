"""R1CS constraint-system proofs: the reference's r1cs::Verifier (src/r1cs/verifier.rs) as a RECORDER.

A gadget written against the reference's API (commit, multiply, allocate, allocate_multiplier, constrain,
specify_randomized_constraints and, inside a randomized callback, challenge_scalar) runs once against a ``Verifier``;
the constraints it adds are kept as data (challenges stay symbolic) and become a ``bpgpu_r1cs_circuit``.  The proofs are
then verified on the GPU (bpgpu_r1cs_verify_batch_ts): transcript, flattening, scalar assembly and the mega-check.
There is no host fallback.

    cs = Verifier(transcript_state)            # 208-byte merlin state (bulletproofs_amd.transcript_new(label) ...)
    xs = [cs.commit(V) for V in commitments]
    my_gadget(cs, xs)
    verdict = cs.verify(R1CSProof.from_bytes(proof_bytes), ctx)    # ctx: Context or Pool with generators loaded

``Verifier.circuit()`` returns the recorded ``Circuit``; ``Circuit.verify_batch`` verifies many proofs of the same gadget.
``verify_batch_combined`` (and ``Circuit.verify_batch_combined``) checks proofs of one or many gadgets in ONE random linear
combination (bpgpu_r1cs_verify_rlc), with the same verdicts; ``group_verifiers`` turns [(Verifier, proof)] into its groups.

Proving (src/r1cs/prover.rs): ``Prover`` records the same gadget the same way and, beside the constraints, HOW each multiplier
gets its inputs (a ``Witness``: free inputs, linear-combination rows that may hold the phase-2 challenges, or zero).  The proof
is then made on the GPU (bpgpu_r1cs_prove_batch):

    cs = Prover(transcript_state)
    xs = [cs.commit(v, v_blinding) for v, v_blinding in values]
    my_gadget(cs, xs)
    proof, V = cs.prove(ctx)                   # R1CSProof, the m commitments (32 bytes each)

Deviation from the reference: ``Prover.commit`` returns the ``Variable`` only; the commitments come back from proving.

Checking a witness (bellman's ``is_satisfied`` / ``which_is_unsatisfied``): ``Prover.check(ctx)`` raises ``Unsatisfied`` naming the
first constraint the assignment leaves unsatisfied, ``Prover.which_is_unsatisfied(ctx)`` returns its index or None, ``check_batch``
does the same for many provers of one gadget (bpgpu_r1cs_witness_check: no generators, no transcript, no blindings).
``prove(ctx, check=True)`` / ``prove_batch(..., check=True)`` run the same check inside the prover, on the proof's own challenges
(bpgpu_r1cs_prove_batch_checked).  ``Prover(transcript, locate=True)`` remembers where each constraint was added.
"""
import ctypes as C
import secrets
import sys

from . import _lib

L_ORDER = 2**252 + 27742317777372353535851937790883648493
KIND_L, KIND_R, KIND_O, KIND_V, KIND_ONE = 0, 1, 2, 3, 4
NO_CHALLENGE = 0xffffffff
MAX_POWER = 255
SRC_ZERO = 0xffffffff          # an allocate() pair left open: a_R = 0 (prover.rs:121-140)
SRC_FREE = 0x80000000          # | j: free input j of the proof

VERDICT_OK = 0
VERDICT_VERIFICATION_ERROR = 1
VERDICT_FORMAT_ERROR = 2
VERDICT_INVALID_GENERATORS_LENGTH = 4

SATISFIED = 0xffffffff         # BPGPU_R1CS_SATISFIED
STATUS_UNSATISFIED = 3         # BPGPU_R1CS_UNSATISFIED


class R1CSError(Exception):
    pass


class FormatError(R1CSError):
    pass


class Unsatisfied(R1CSError):
    """The witness leaves a constraint unsatisfied.  ``constraint``: the lowest failing index, in the order the gadget added them;
    ``where``: "file:line" of the call that added it (a ``Prover`` made with ``locate=True``), else None."""

    def __init__(self, constraint, where=None, position=None):
        self.constraint, self.where, self.position = constraint, where, position
        msg = "constraint %d is not satisfied" % constraint
        if where:
            msg += " (added at %s)" % where
        if position is not None:
            msg += " [proof %d of the batch]" % position
        super().__init__(msg)


# ---- variables and linear combinations (src/r1cs/linear_combination.rs) ------------------------------------------------
# a term is ((kind, index), challenge or None, power, coeff): coeff * ch^power * variable
def _as_lc(x):
    if isinstance(x, LinearCombination):
        return x
    if isinstance(x, Variable):
        return LinearCombination([((x.kind, x.index), None, 0, 1)])
    if isinstance(x, Challenge):
        return LinearCombination([((KIND_ONE, 0), x.index, 1, 1)])
    if isinstance(x, int):
        return LinearCombination([((KIND_ONE, 0), None, 0, x % L_ORDER)])
    raise TypeError("not a linear combination: %r" % (x,))


class _Arith:
    def __add__(self, o):
        return LinearCombination(_as_lc(self).terms + _as_lc(o).terms)

    def __radd__(self, o):
        return _as_lc(o) + self

    def __sub__(self, o):
        return self + (-_as_lc(o))

    def __rsub__(self, o):
        return _as_lc(o) + (-_as_lc(self))

    def __neg__(self):
        return _as_lc(self) * -1

    def __mul__(self, o):
        lc = _as_lc(self)
        if isinstance(o, int):
            return LinearCombination([(v, c, p, k * o % L_ORDER) for v, c, p, k in lc.terms])
        if isinstance(o, Challenge):
            out = []
            for v, c, p, k in lc.terms:
                if c is not None and c != o.index:
                    raise R1CSError("a product of two different challenges cannot be recorded")
                out.append((v, o.index, p + 1, k))
            return LinearCombination(out)
        if isinstance(o, LinearCombination) and o._is_challenge_monomial():   # k c^e, as c * c gives it (a Scalar in the reference)
            (_, oc, op, ok), = o.terms
            out = []
            for v, c, p, k in lc.terms:
                if c is not None and c != oc:
                    raise R1CSError("a product of two different challenges cannot be recorded")
                out.append((v, oc, p + op, k * ok % L_ORDER))
            return LinearCombination(out)
        if isinstance(o, (Variable, LinearCombination)) and lc._is_challenge_monomial():
            return _as_lc(o) * lc
        raise TypeError("a linear combination multiplies by a scalar (int), a challenge or a product of powers of one challenge only")

    def __rmul__(self, o):
        return self * o


class Variable(_Arith):
    def __init__(self, kind, index):
        self.kind, self.index = kind, index

    def __repr__(self):
        return "Variable(%s, %d)" % ("LROV1"[self.kind], self.index)


class Challenge(_Arith):
    """challenge_scalar's result: symbolic (its value is drawn per proof, on the device)"""

    def __init__(self, index, label):
        self.index, self.label = index, label


class LinearCombination(_Arith):
    def __init__(self, terms=None):
        self.terms = list(terms or [])

    def _is_challenge_monomial(self):
        """one ONE term that carries a challenge: coefficient * c^power"""
        return len(self.terms) == 1 and self.terms[0][0] == (KIND_ONE, 0) and self.terms[0][1] is not None


def ONE():
    return Variable(KIND_ONE, 0)


# ---- proofs (src/r1cs/proof.rs) -------------------------------------------------------------------------------------------
class R1CSProof:
    """The serialized proof, checked as R1CSProof::from_bytes does (proof.rs:129-204)."""
    NAMES = ("A_I1", "A_O1", "S1", "A_I2", "A_O2", "S2", "T_1", "T_3", "T_4", "T_5", "T_6", "t_x", "t_x_blinding", "e_blinding")

    def __init__(self, fields, ipp):
        self.fields, self.ipp = fields, ipp

    @staticmethod
    def from_bytes(b):
        b = bytes(b)
        if len(b) < 1 or (len(b) - 1) % 32 or b[0] not in (0, 1):
            raise FormatError()
        n_el = 11 if b[0] == 0 else 14
        rest = b[1:]
        if len(rest) < 32 * n_el:
            raise FormatError()
        els = [rest[32 * i:32 * i + 32] for i in range(n_el)]
        if b[0] == 0:
            els = els[:3] + [bytes(32)] * 3 + els[3:]
        ipp = rest[32 * n_el:]
        ne = len(ipp) // 32
        if ne < 2 or (ne - 2) % 2 or (ne - 2) // 2 >= 32:
            raise FormatError()
        for s in els[11:] + [ipp[-64:-32], ipp[-32:]]:
            if int.from_bytes(s, "little") >= L_ORDER:
                raise FormatError()
        return R1CSProof(els, ipp)

    def to_bytes(self):
        one_phase = all(x == bytes(32) for x in self.fields[3:6])
        els = self.fields[:3] + self.fields[6:] if one_phase else self.fields
        return bytes([0 if one_phase else 1]) + b"".join(els) + self.ipp


# ---- the recorder (src/r1cs/verifier.rs) ------------------------------------------------------------------------------------
class Verifier:
    def __init__(self, transcript):
        assert len(transcript) == _lib.TRANSCRIPT_BYTES
        self.transcript = bytes(transcript)
        self.V = []
        self.constraints = []
        self.num_vars = 0
        self.deferred = []
        self.pending_multiplier = None
        self.challenge_labels = []
        self._n1 = None
        self._circuit = None

    # ConstraintSystem (verifier.rs:67-127)
    def commit(self, commitment):
        assert len(commitment) == 32 and self._n1 is None
        self.V.append(bytes(commitment))
        return Variable(KIND_V, len(self.V) - 1)

    def multiply(self, left, right):
        var = self.num_vars
        self.num_vars += 1
        l_var, r_var, o_var = Variable(KIND_L, var), Variable(KIND_R, var), Variable(KIND_O, var)
        self.constrain(_as_lc(left) - l_var)
        self.constrain(_as_lc(right) - r_var)
        return l_var, r_var, o_var

    def allocate(self, assignment=None):
        if self.pending_multiplier is None:
            i = self.num_vars
            self.num_vars += 1
            self.pending_multiplier = i
            return Variable(KIND_L, i)
        i, self.pending_multiplier = self.pending_multiplier, None
        return Variable(KIND_R, i)

    def allocate_multiplier(self, input_assignments=None):
        var = self.num_vars
        self.num_vars += 1
        return Variable(KIND_L, var), Variable(KIND_R, var), Variable(KIND_O, var)

    def multipliers_len(self):
        return self.num_vars

    def constrain(self, lc):
        self.constraints.append(_as_lc(lc))

    # RandomizableConstraintSystem (verifier.rs:130-141, 175-179)
    def specify_randomized_constraints(self, callback):
        self.deferred.append(callback)

    def challenge_scalar(self, label):
        if self._n1 is None:
            raise R1CSError("challenge_scalar is available inside a randomized callback only")
        self.challenge_labels.append(bytes(label))
        return Challenge(len(self.challenge_labels) - 1, bytes(label))

    def _finish(self):
        """create_randomized_constraints (verifier.rs:300-321): the callbacks run once, their challenges stay symbolic"""
        if self._n1 is None:
            self._n1 = self.num_vars
            self.pending_multiplier = None
            self._two_phase = len(self.deferred) > 0
            for cb in self.deferred:
                cb(self)
            self.deferred = []
        return self

    def descriptor(self):
        """(m, n1, n2, two_phase, labels, constraints as [[((kind, index), challenge, power, coeff)]])"""
        self._finish()
        return (len(self.V), self._n1, self.num_vars - self._n1, self._two_phase, list(self.challenge_labels),
                [lc.terms for lc in self.constraints])

    def circuit(self):
        if self._circuit is None:
            self._circuit = Circuit(*self.descriptor())
        return self._circuit

    def verify(self, proof, gens, rng32=None, want_msm=False, want_transcript=False):
        """Verifier::verify with the generators of `gens` (a Context or Pool): the verdict (0 = Ok) [, msm] [, transcript]"""
        pb = proof.to_bytes() if isinstance(proof, R1CSProof) else bytes(proof)
        out = self.circuit().verify_batch(gens, [pb], b"".join(self.V), self.transcript, rng32=rng32, want_msm=want_msm,
                                          want_transcripts=want_transcript)
        if not isinstance(out, tuple):
            return out[0]
        return (out[0][0],) + tuple(out[1:])


class Prover(Verifier):
    """r1cs::Prover (src/r1cs/prover.rs) as a RECORDER: the same constraints as ``Verifier`` records for the same gadget, plus the
    witness program.  Assignments: an int becomes the next free input of the proof; a symbolic expression of challenges (inside
    a randomized callback) becomes an LC row evaluated on the device, as do multiply's inputs (Prover::eval, prover.rs:340-356)."""

    def __init__(self, transcript, locate=False):
        super().__init__(transcript)
        self.v, self.v_blinding, self.free = [], [], []
        self.src_left, self.src_right, self.rows = [], [], []
        self._witness = None
        self.locations = [] if locate else None   # per constraint: (file, line) of the gadget's constrain / multiply call

    def constrain(self, lc):
        if self.locations is not None:           # the nearest frame outside this module: the gadget's own line
            f = sys._getframe(1)
            while f is not None and f.f_code.co_filename == __file__:
                f = f.f_back
            self.locations.append((f.f_code.co_filename, f.f_lineno) if f is not None else None)
        super().constrain(lc)

    def where(self, constraint):
        """"file:line" of the call that added constraint `constraint`, or None (locate=False)"""
        if self.locations is None or not 0 <= constraint < len(self.locations) or self.locations[constraint] is None:
            return None
        return "%s:%d" % self.locations[constraint]

    def commit(self, v, v_blinding):
        """prover.rs:296-306; returns the Variable only (V_j is computed on the device and returned by prove)"""
        if self._n1 is not None:
            raise R1CSError("commit after the gadget was recorded")
        self.v.append(v % L_ORDER)
        self.v_blinding.append(v_blinding % L_ORDER)
        self.V.append(None)
        return Variable(KIND_V, len(self.V) - 1)

    def _row(self, x, i):
        lc = _as_lc(x)
        for (kind, idx), ch, pw, _ in lc.terms:
            if kind in (KIND_L, KIND_R, KIND_O) and idx >= i:
                raise R1CSError("an input of multiplier %d reads multiplier %d" % (i, idx))
            if kind in (KIND_R, KIND_O) and idx == self.pending_multiplier:
                raise R1CSError("an input reads the right half of an allocate() pair that is still open")
            if ch is not None and pw > MAX_POWER:
                raise R1CSError("challenge power %d above %d" % (pw, MAX_POWER))
        self.rows.append(list(lc.terms))
        return len(self.rows) - 1

    def _assign(self, x, i):
        if x is None:
            raise R1CSError("MissingAssignment: the prover needs every assignment")
        if isinstance(x, int):
            self.free.append(x % L_ORDER)
            return SRC_FREE | (len(self.free) - 1)
        return self._row(x, i)

    def multiply(self, left, right):                         # prover.rs:93-119
        i = self.num_vars
        self.src_left.append(self._row(left, i))
        self.src_right.append(self._row(right, i))
        return super().multiply(left, right)

    def allocate(self, assignment=None):                     # prover.rs:121-140
        if self.pending_multiplier is None:
            i = self.num_vars
            self.src_left.append(self._assign(assignment, i))
            self.src_right.append(SRC_ZERO)
        else:
            i = self.pending_multiplier
            self.src_right[i] = self._assign(assignment, i)
        return super().allocate()

    def allocate_multiplier(self, input_assignments=None):  # prover.rs:142-159
        if input_assignments is None:
            raise R1CSError("MissingAssignment: the prover needs every assignment")
        left, right = input_assignments
        i = self.num_vars
        self.src_left.append(self._assign(left, i))
        self.src_right.append(self._assign(right, i))
        return super().allocate_multiplier()

    def structure(self):
        """everything that must agree between the proofs of one batch: the constraints and the witness program"""
        self._finish()
        return (self.descriptor(), tuple(self.src_left), tuple(self.src_right), tuple(tuple(r) for r in self.rows), len(self.free))

    def witness(self):
        if self._witness is None:
            self._finish()
            self._witness = Witness(self.circuit(), len(self.free), self.src_left, self.src_right, self.rows)
        return self._witness

    def inputs(self):
        """(v, v_blinding, free inputs) of this proof as 32-byte scalars"""
        self._finish()
        enc = lambda xs: b"".join(x.to_bytes(32, "little") for x in xs)
        return enc(self.v), enc(self.v_blinding), enc(self.free)

    def prove(self, ctx, rng32=None, check=False):
        """Prover::prove with the generators of `ctx` (a Context): (R1CSProof, [V_j]).  check=True: ``Unsatisfied`` instead of a
        proof the verifier would reject (the check runs on the proof's own challenges)."""
        return prove_batch(ctx, [self], rng32, check=check)[0]

    def which_is_unsatisfied(self, ctx, challenges=None):
        """the lowest index of a constraint this prover's assignment leaves unsatisfied, or None (see ``check_batch``)"""
        return check_batch(ctx, [self], challenges)[0]

    def check(self, ctx, challenges=None):
        """raises ``Unsatisfied`` when the assignment leaves a constraint unsatisfied (see ``check_batch``)"""
        q = self.which_is_unsatisfied(ctx, challenges)
        if q is not None:
            raise Unsatisfied(q, self.where(q))


def _same_gadget(provers):
    st = provers[0].structure()
    if any(p.structure() != st for p in provers[1:]):
        raise R1CSError("the provers of one batch must record the same gadget")


def _challenge_bytes(challenges, nch, nbatch):
    """None, bytes (nbatch x nch x 32), nch ints (the same values for every proof) or nbatch lists of nch ints"""
    if challenges is None or isinstance(challenges, (bytes, bytearray)):
        return challenges
    rows = list(challenges)
    if not rows or isinstance(rows[0], int):
        rows = [rows] * nbatch
    if len(rows) != nbatch or any(len(r) != nch for r in rows):
        raise ValueError("challenges: %d values per proof" % nch)
    return b"".join((c % L_ORDER).to_bytes(32, "little") for r in rows for c in r)


def check_batch(ctx, provers, challenges=None, want_count=False, want_map=False):
    """Which constraint does each prover's assignment leave unsatisfied?  The provers must record the same gadget (R1CSError
    otherwise).  Returns a list with None (every constraint holds) or the lowest failing index per prover [, the failure counts]
    [, the failing sets as bytes: bit q % 8 of byte q / 8].  Needs a Context only: no generators, no transcript, no blindings.
    challenges: the phase-2 challenge values (bytes, ints for all proofs, or a list of ints per proof); None on a gadget that has
    challenges draws uniform scalars.  A witness that is right satisfies every constraint under any challenges.  One that is wrong
    fails under almost all of them."""
    if not provers:
        return ([],) * (1 + want_count + want_map) if (want_count or want_map) else []
    _same_gadget(provers)
    circuit = provers[0].circuit()
    ins = [p.inputs() for p in provers]
    nb = len(provers)
    res = provers[0].witness().check_batch(ctx, circuit, nb, b"".join(i[0] for i in ins), b"".join(i[2] for i in ins),
                                           _challenge_bytes(challenges, circuit.n_challenges, nb), want_count=want_count, want_map=want_map)
    first, status = res[0], res[1]
    if any(status):
        raise R1CSError("non-canonical input scalar (status %s)" % list(status))
    out = [None if q == SATISFIED else q for q in first]
    return (out,) + tuple(res[2:]) if (want_count or want_map) else out


def prove_batch(ctx, provers, rng32=None, check=False):
    """one proof per recorded Prover, all of the same gadget (R1CSError otherwise): [(R1CSProof, [V_j])] in order.
    rng32: len(provers) x 32 bytes (what finalize takes from thread_rng) or None (the OS generator).
    check=True: the witness check runs inside the prover on each proof's own challenges; ``Unsatisfied`` for the first proof whose
    witness fails (its position in the batch is in the message and in ``.position``)."""
    if not provers:
        return []
    _same_gadget(provers)
    w = provers[0].witness()
    ins = [p.inputs() for p in provers]
    res = w.prove_batch(ctx, provers[0].circuit(), len(provers), b"".join(i[0] for i in ins), b"".join(i[1] for i in ins),
                        b"".join(i[2] for i in ins), b"".join(p.transcript for p in provers), rng32, check=check)
    proofs, coms, status = res[:3]
    if any(st not in (0, STATUS_UNSATISFIED) for st in status):
        raise R1CSError("non-canonical input scalar (status %s)" % list(status))
    if check:
        for b, q in enumerate(res[3]):
            if q != SATISFIED:
                raise Unsatisfied(q, provers[b].where(q), position=b)
    m = provers[0].circuit().m
    return [(R1CSProof.from_bytes(pb), [coms[32 * (b * m + j):32 * (b * m + j + 1)] for j in range(m)]) for b, pb in enumerate(proofs)]


class Witness:
    """A recorded witness program as a bpgpu_r1cs_witness (host object; uploaded to each GPU on first use)."""

    def __init__(self, circuit, n_free, src_left, src_right, rows):
        L = lib()
        self.n_free = n_free
        row = [0]
        kind, index, chal, power, coeff = [], [], [], [], []
        for terms in rows:
            for (k_, i_), ch, pw, cf in terms:
                kind.append(k_)
                index.append(i_)
                chal.append(NO_CHALLENGE if ch is None else ch)
                power.append(0 if ch is None else pw)
                coeff.append((cf % L_ORDER).to_bytes(32, "little"))
            row.append(len(kind))
        u32 = C.c_uint32
        arr = lambda xs: (u32 * max(len(xs), 1))(*xs)
        self._h = C.c_void_p()
        rc = L.bpgpu_r1cs_witness_create(circuit._h, n_free, arr(src_left), arr(src_right), len(rows), arr(row), len(kind), bytes(kind),
                                         arr(index), arr(chal), arr(power), b"".join(coeff), C.byref(self._h))
        if rc:
            raise _lib.BpgpuError("bpgpu_r1cs_witness_create: %d" % rc)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().bpgpu_r1cs_witness_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check_batch(self, ctx, circuit, nbatch, v, free_inputs, challenges=None, want_count=False, want_map=False):
        """raw arrays through bpgpu_r1cs_witness_check: v nbatch x m x 32 bytes; free_inputs nbatch x n_free x 32; challenges
        nbatch x n_challenges x 32 bytes (canonical scalars, proof by proof in draw order) or None: uniform scalars are drawn.
        A witness that is right satisfies every constraint under any challenges.  One that is wrong fails under almost all of them.
        Returns (first failing index per proof or SATISFIED, status bytes[, counts][, maps as nbatch byte strings])."""
        nch, Q = circuit.n_challenges, circuit.n_constraints
        assert len(v) == 32 * circuit.m * nbatch and len(free_inputs) == 32 * self.n_free * nbatch
        if challenges is None and nch:
            challenges = b"".join(secrets.randbelow(L_ORDER).to_bytes(32, "little") for _ in range(nch * nbatch))
        assert challenges is None or len(challenges) == 32 * nch * nbatch
        nb = max(nbatch, 1)
        stride = max((Q + 7) // 8, 1)
        first, count = (C.c_uint32 * nb)(), (C.c_uint32 * nb)() if want_count else None
        maps = C.create_string_buffer(stride * nb) if want_map else None
        status = C.create_string_buffer(nb)
        rc = lib().bpgpu_r1cs_witness_check(ctx.h, circuit._h, self._h, nbatch, bytes(v), bytes(free_inputs), bytes(challenges) if nch else None,
                                            first, count, maps, stride if want_map else 0, status)
        ctx._chk(rc)
        res = (list(first[:nbatch]), status.raw[:nbatch])
        if want_count:
            res += (list(count[:nbatch]),)
        if want_map:
            res += ([maps.raw[b * stride:b * stride + (Q + 7) // 8] for b in range(nbatch)],)
        return res

    def prove_batch(self, ctx, circuit, nbatch, v, v_blinding, free_inputs, transcripts, rng32=None, want_transcripts=False, check=False):
        """raw arrays: v, v_blinding nbatch x m x 32 bytes; free_inputs nbatch x n_free x 32; transcripts one 208-byte state or
        nbatch of them.  Returns (proofs as bytes, commitments, status bytes[, transcripts]).  check=True
        (bpgpu_r1cs_prove_batch_checked): one more element, the first failing constraint per proof (SATISFIED: none); a proof
        whose witness fails has status STATUS_UNSATISFIED and no bytes."""
        TS = _lib.TRANSCRIPT_BYTES
        assert len(v) == len(v_blinding) == 32 * circuit.m * nbatch and len(free_inputs) == 32 * self.n_free * nbatch
        assert len(transcripts) in (TS, TS * nbatch) and (rng32 is None or len(rng32) == 32 * nbatch)
        ts_stride = TS if len(transcripts) == TS * nbatch and nbatch > 1 else 0
        stride = 1 + 32 * 14 + 32 * (2 * (circuit.padded_n.bit_length() - 1) + 2)
        nb = max(nbatch, 1)
        out = C.create_string_buffer(stride * nb)
        lens = (C.c_uint32 * nb)()
        coms = C.create_string_buffer(32 * circuit.m * nb + 1)
        status = C.create_string_buffer(nb)
        tso = C.create_string_buffer(TS * nb) if want_transcripts else None
        if check:
            first = (C.c_uint32 * nb)()
            rc = lib().bpgpu_r1cs_prove_batch_checked(ctx.h, circuit._h, self._h, nbatch, v, v_blinding, free_inputs, transcripts, ts_stride, rng32,
                                                      out, stride, lens, coms, status, tso, first)
        else:
            rc = lib().bpgpu_r1cs_prove_batch(ctx.h, circuit._h, self._h, nbatch, v, v_blinding, free_inputs, transcripts, ts_stride, rng32,
                                              out, stride, lens, coms, status, tso)
        ctx._chk(rc)
        proofs = [out.raw[b * stride:b * stride + lens[b]] for b in range(nbatch)]
        res = (proofs, coms.raw[:32 * circuit.m * nbatch], status.raw[:nbatch])
        if want_transcripts:
            res += (tso.raw[:TS * nbatch],)
        return res + (list(first[:nbatch]),) if check else res


def flattened_constraints(descriptor, z, challenges):
    """flattened_constraints (verifier.rs:260-298) of a recorded descriptor for given z and challenge values:
    (wL, wR, wO, wV, wc).  Host code for checking the recording; the verifier computes this on the device."""
    m, n1, n2, _, _, cons = descriptor
    n = n1 + n2
    w = {KIND_L: [0] * n, KIND_R: [0] * n, KIND_O: [0] * n, KIND_V: [0] * m, KIND_ONE: [0]}
    ez = z % L_ORDER
    for terms in cons:
        for (kind, idx), ch, pw, k in terms:
            c = k * (pow(challenges[ch], pw, L_ORDER) if ch is not None else 1) * ez
            w[kind][idx] = (w[kind][idx] + (-c if kind in (KIND_V, KIND_ONE) else c)) % L_ORDER
        ez = ez * z % L_ORDER
    return w[KIND_L], w[KIND_R], w[KIND_O], w[KIND_V], w[KIND_ONE][0]


class Circuit:
    """A recorded gadget as a bpgpu_r1cs_circuit (host object; uploaded to each GPU on first use)."""

    def __init__(self, m, n1, n2, two_phase, labels, constraints):
        L = lib()
        self.m, self.n1, self.n2, self.two_phase = m, n1, n2, bool(two_phase)
        self.n_challenges, self.n_constraints = len(labels), len(constraints)
        row = [0]
        kind, index, chal, power, coeff = [], [], [], [], []
        for terms in constraints:
            for (k_, i_), ch, pw, cf in terms:
                if pw > MAX_POWER:
                    raise R1CSError("challenge power %d above %d" % (pw, MAX_POWER))
                kind.append(k_)
                index.append(i_)
                chal.append(NO_CHALLENGE if ch is None else ch)
                power.append(0 if ch is None else pw)
                coeff.append((cf % L_ORDER).to_bytes(32, "little"))
            row.append(len(kind))
        nt = len(kind)
        u32 = C.c_uint32
        self._h = C.c_void_p()
        lbl = b"".join(labels)
        lens = (u32 * max(len(labels), 1))(*[len(x) for x in labels])
        rc = L.bpgpu_r1cs_circuit_create(m, n1, n2, 1 if two_phase else 0, len(labels), lbl, lens, len(constraints),
                                         (u32 * len(row))(*row), nt, bytes(kind), (u32 * max(nt, 1))(*index), (u32 * max(nt, 1))(*chal),
                                         (u32 * max(nt, 1))(*power), b"".join(coeff), C.byref(self._h))
        if rc:
            raise _lib.BpgpuError("bpgpu_r1cs_circuit_create: %d" % rc)
        pn, nu = C.c_size_t(), C.c_size_t()
        L.bpgpu_r1cs_circuit_shape(self._h, C.byref(pn), C.byref(nu))
        self.padded_n, self.n_unique = pn.value, nu.value

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().bpgpu_r1cs_circuit_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def verify_batch(self, gens, proofs, commitments, transcripts, rng32=None, want_msm=False, want_transcripts=False):
        """proofs: list of serialized proofs; commitments: nbatch x m x 32 bytes; transcripts: one 208-byte state or nbatch
        of them (concatenated); rng32: nbatch x 32 bytes or None.  Returns verdict bytes [, msm] [, transcripts]."""
        nb = len(proofs)
        stride = max([len(p) for p in proofs] + [1])
        stride = (stride + 3) & ~3
        buf = b"".join(bytes(p) + bytes(stride - len(p)) for p in proofs)
        lens = (C.c_uint32 * max(nb, 1))(*[len(p) for p in proofs])
        TS = _lib.TRANSCRIPT_BYTES
        assert len(commitments) == 32 * self.m * nb and len(transcripts) in (TS, TS * nb)
        assert rng32 is None or len(rng32) == 32 * nb
        ts_stride = TS if (len(transcripts) == TS * nb and nb != 1) or nb == 1 else 0
        verdict = C.create_string_buffer(max(nb, 1))
        msm = C.create_string_buffer(32 * max(nb, 1)) if want_msm else None
        tso = C.create_string_buffer(TS * max(nb, 1)) if want_transcripts else None
        L = lib()
        if isinstance(gens, _lib.Pool):
            rc = L.bpgpu_pool_r1cs_verify_ts(gens.h, self._h, nb, buf, stride, lens, commitments, transcripts, ts_stride, rng32, verdict, msm, tso)
        else:
            rc = L.bpgpu_r1cs_verify_batch_ts(gens.h, self._h, nb, buf, stride, lens, commitments, transcripts, ts_stride, rng32, verdict, msm, tso)
        gens._chk(rc)
        out = [verdict.raw[:nb]]
        if want_msm:
            out.append(msm.raw[:32 * nb])
        if want_transcripts:
            out.append(tso.raw[:TS * nb])
        return out[0] if len(out) == 1 else tuple(out)

    def verify_batch_combined(self, gens, proofs, commitments, transcripts, rng32=None, weights64=None, want_batch=False, want_transcripts=False):
        """verify_batch's arguments through ONE combined check (bpgpu_r1cs_verify_rlc): the same verdicts; weights64: nbatch x 64 bytes
        or None (drawn by the library).  Returns verdict bytes [, the 33 batch bytes] [, transcripts]."""
        return verify_batch_combined(gens, [(self, proofs, commitments, transcripts)], rng32=rng32, weights64=weights64, want_batch=want_batch,
                                     want_transcripts=want_transcripts)


def verify_batch_combined(gens, groups, rng32=None, weights64=None, want_batch=False, want_transcripts=False):
    """Proofs of one or many gadgets through ONE combined check (bpgpu_r1cs_verify_rlc / bpgpu_pool_r1cs_verify_rlc).
    groups: [(circuit, proofs, commitments, transcripts)], each as Circuit.verify_batch takes them; rng32 (32 bytes per proof) and
    weights64 (64) run over all proofs, the groups' in order, or are None.  Verdicts (VERDICT_*) are those of verify_batch.
    Returns verdict bytes [, batch bytes: [0] = 0 when the combination was the identity, [1..33) = its encoding] [, transcripts]."""
    groups = list(groups)
    if not groups:
        raise ValueError("verify_batch_combined: no groups")
    TS = _lib.TRANSCRIPT_BYTES
    ng = len(groups)
    sz = C.c_size_t
    u32p = C.POINTER(C.c_uint32)
    circ, nbs, strides, ts_strides = (C.c_void_p * ng)(), (sz * ng)(), (sz * ng)(), (sz * ng)()
    pr, coms, tss, lens = (C.c_char_p * ng)(), (C.c_char_p * ng)(), (C.c_char_p * ng)(), (u32p * ng)()
    keep = []
    total = 0
    for g, grp in enumerate(groups):
        if len(grp) != 4:
            raise ValueError("group %d: (circuit, proofs, commitments, transcripts) expected" % g)
        circuit, proofs, commitments, transcripts = grp
        proofs = [p.to_bytes() if isinstance(p, R1CSProof) else bytes(p) for p in proofs]
        nb = len(proofs)
        if len(commitments) != 32 * circuit.m * nb:
            raise ValueError("group %d: %d commitment bytes for %d proofs of m = %d" % (g, len(commitments), nb, circuit.m))
        if len(transcripts) not in (TS, TS * nb):
            raise ValueError("group %d: transcripts must be one state or one per proof" % g)
        stride = (max([len(p) for p in proofs] + [1]) + 3) & ~3
        buf = b"".join(p + bytes(stride - len(p)) for p in proofs)
        ln = (C.c_uint32 * max(nb, 1))(*[len(p) for p in proofs])
        cm, ts = bytes(commitments), bytes(transcripts)
        keep += [buf, ln, cm, ts]
        circ[g] = circuit._h.value
        nbs[g], strides[g] = nb, stride
        ts_strides[g] = TS if nb and len(ts) == TS * nb else 0
        pr[g], coms[g], tss[g] = buf, cm, ts
        lens[g] = C.cast(ln, u32p)
        total += nb
    if rng32 is not None and len(rng32) != 32 * total:
        raise ValueError("rng32: 32 bytes per proof")
    if weights64 is not None and len(weights64) != 64 * total:
        raise ValueError("weights64: 64 bytes per proof")
    verdict = C.create_string_buffer(max(total, 1))
    batch = C.create_string_buffer(33)
    tso = C.create_string_buffer(TS * max(total, 1)) if want_transcripts else None
    L = lib()
    fn = L.bpgpu_pool_r1cs_verify_rlc if isinstance(gens, _lib.Pool) else L.bpgpu_r1cs_verify_rlc
    rc = fn(gens.h, ng, circ, nbs, pr, strides, lens, coms, tss, ts_strides, rng32, weights64, verdict, batch, tso)
    gens._chk(rc)
    out = [verdict.raw[:total]]
    if want_batch:
        out.append(batch.raw[:33])
    if want_transcripts:
        out.append(tso.raw[:TS * total])
    return out[0] if len(out) == 1 else tuple(out)


def group_verifiers(pairs):
    """[(Verifier, proof)] -> (groups, index) for verify_batch_combined: verifiers that recorded an identical gadget (the same descriptor)
    share one Circuit; each group carries one transcript per proof.  index[i] is the position of pair i's verdict in the call's verdicts."""
    by_key, groups, members = {}, [], []
    for i, (cs, proof) in enumerate(pairs):
        key = repr(cs.descriptor())
        g = by_key.get(key)
        if g is None:
            g = by_key[key] = len(groups)
            groups.append((cs.circuit(), [], [], []))
            members.append([])
        groups[g][1].append(proof.to_bytes() if isinstance(proof, R1CSProof) else bytes(proof))
        groups[g][2].append(b"".join(cs.V))
        groups[g][3].append(cs.transcript)
        members[g].append(i)
    index = [0] * len(pairs)
    pos = 0
    for mem in members:
        for i in mem:
            index[i] = pos
            pos += 1
    return [(c, p, b"".join(cm), b"".join(ts)) for c, p, cm, ts in groups], index


def lib():
    L = _lib.lib()
    if not getattr(L, "_r1cs_bound", False):
        vp, sz, u8p, i = C.c_void_p, C.c_size_t, C.c_char_p, C.c_int
        u32p = C.POINTER(C.c_uint32)
        L.bpgpu_r1cs_circuit_create.argtypes = [sz, sz, sz, i, sz, u8p, u32p, sz, u32p, sz, u8p, u32p, u32p, u32p, u8p, C.POINTER(vp)]
        L.bpgpu_r1cs_circuit_destroy.argtypes = [vp]
        L.bpgpu_r1cs_circuit_destroy.restype = None
        L.bpgpu_r1cs_circuit_shape.argtypes = [vp, C.POINTER(sz), C.POINTER(sz)]
        L.bpgpu_r1cs_verify_batch_ts.argtypes = [vp, vp, sz, u8p, sz, u32p, u8p, u8p, sz, u8p, u8p, u8p, u8p]
        L.bpgpu_pool_r1cs_verify_ts.argtypes = [vp, vp, sz, u8p, sz, u32p, u8p, u8p, sz, u8p, u8p, u8p, u8p]
        szp, u8pp = C.POINTER(sz), C.POINTER(u8p)
        rlc_args = [vp, sz, C.POINTER(vp), szp, u8pp, szp, C.POINTER(u32p), u8pp, u8pp, szp, u8p, u8p, u8p, u8p, u8p]
        L.bpgpu_r1cs_verify_rlc.argtypes = rlc_args
        L.bpgpu_pool_r1cs_verify_rlc.argtypes = rlc_args
        L.bpgpu_r1cs_witness_create.argtypes = [vp, sz, u32p, u32p, sz, u32p, sz, u8p, u32p, u32p, u32p, u8p, C.POINTER(vp)]
        L.bpgpu_r1cs_witness_destroy.argtypes = [vp]
        L.bpgpu_r1cs_witness_destroy.restype = None
        L.bpgpu_r1cs_prove_batch.argtypes = [vp, vp, vp, sz, u8p, u8p, u8p, u8p, sz, u8p, u8p, sz, u32p, u8p, u8p, u8p]
        L.bpgpu_r1cs_prove_batch_checked.argtypes = L.bpgpu_r1cs_prove_batch.argtypes + [u32p]
        L.bpgpu_r1cs_witness_check.argtypes = [vp, vp, vp, sz, u8p, u8p, u8p, u32p, u32p, u8p, sz, u8p]
        L._r1cs_bound = True
    return L
