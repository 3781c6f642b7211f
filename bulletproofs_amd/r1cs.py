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
"""
import ctypes as C

from . import _lib

L_ORDER = 2**252 + 27742317777372353535851937790883648493
KIND_L, KIND_R, KIND_O, KIND_V, KIND_ONE = 0, 1, 2, 3, 4
NO_CHALLENGE = 0xffffffff
MAX_POWER = 255

VERDICT_OK = 0
VERDICT_VERIFICATION_ERROR = 1
VERDICT_FORMAT_ERROR = 2
VERDICT_INVALID_GENERATORS_LENGTH = 4


class R1CSError(Exception):
    pass


class FormatError(R1CSError):
    pass


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
        raise TypeError("a linear combination multiplies by a scalar (int) or a challenge only")

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
        L._r1cs_bound = True
    return L
