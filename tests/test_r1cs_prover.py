"""R1CS proof creation, host side (no GPU): the Prover recorder against r1cs.Verifier, its witness program against the twin's
a_L / a_R / a_O, the twin prover with the reference's TranscriptRng, and bpgpu_r1cs_witness_create's validation."""
import ctypes as C
import hashlib
import random

import pytest

import r1cs_prover_twin as P
import r1cs_twin as R

CAP = 128


@pytest.fixture(scope="module")
def gens(oracle):
    return oracle.Gens(CAP, 1).export()


def _scalars(tag, n):
    return [int.from_bytes(hashlib.shake_256(b"%s%d" % (tag, i)).digest(64), "little") % R.L for i in range(n)]


def _shuffle_case(k, seed):
    rnd = random.Random(seed)
    inp = [rnd.getrandbits(64) for _ in range(k)]
    out = inp[:]
    rnd.shuffle(out)
    return inp + out, lambda cs, v: R.shuffle_gadget(cs, v[:k], v[k:])


def _cases():
    """(name, values, gadget(cs, vars), gadget with the prover's assignments)"""
    out = []
    for k in (1, 2, 5):
        vals, g = _shuffle_case(k, k)
        out.append(("shuffle%d" % k, vals, g, g))
    ex = (3, 4, 6, 1, 40)
    g = lambda cs, v: R.example_gadget(cs, v[0], v[1], v[2], v[3], v[4], 9)
    out.append(("example", list(ex), g, g))
    v = 0xa5
    out.append(("range8", [v], lambda cs, x: R.range_gadget(cs, x[0], None, 8), lambda cs, x: R.range_gadget(cs, x[0], v, 8)))
    out.append(("split", [7, 11], lambda cs, x: P.split_gadget(cs, x, None), lambda cs, x: P.split_gadget(cs, x, (7, 11))))
    out.append(("open", [5, 13], lambda cs, x: P.open_gadget(cs, x, None), lambda cs, x: P.open_gadget(cs, x, (5, 13))))
    return out


CASES = _cases()


def _record(vals, gadget_p, tag=b"rec"):
    from bulletproofs_amd import r1cs
    cs = r1cs.Prover(bytes(208))
    bl = _scalars(tag, len(vals))
    xs = [cs.commit(v, b) for v, b in zip(vals, bl)]
    gadget_p(cs, xs)
    return cs, bl


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_prover_recorder_matches_verifier_descriptor(case):
    from bulletproofs_amd import r1cs
    _, vals, gadget_v, gadget_p = case
    cs, _ = _record(vals, gadget_p)
    ver = r1cs.Verifier(bytes(208))
    xs = [ver.commit(bytes(32)) for _ in vals]
    gadget_v(ver, xs)
    assert cs.descriptor() == ver.descriptor()
    assert len(cs.src_left) == len(cs.src_right) == cs.num_vars


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_witness_program_reproduces_twin_witness(gens, case):
    name, vals, _, gadget_p = case
    cs, bl = _record(vals, gadget_p)
    st0 = R.transcript_state(R.T.Transcript(b"witness-" + name.encode()))
    _, _, twin = P.prove(gens, CAP, st0, vals, bl, gadget_p, bytes(range(32)))
    aL, aR, aO = P.eval_witness(cs, twin.challenges)
    assert (aL, aR, aO) == (twin.a_L, twin.a_R, twin.a_O)
    cs.witness()   # the library accepts the recorded program


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_twin_proofs_with_transcript_rng_verify(gens, case):
    name, vals, gadget_v, gadget_p = case
    st0 = R.transcript_state(R.T.Transcript(b"twin-" + name.encode()))
    bl = _scalars(b"b" + name.encode(), len(vals))
    pf, Vs, _ = P.prove(gens, CAP, st0, vals, bl, gadget_p, hashlib.sha256(name.encode()).digest())
    assert P.verify(gens, CAP, st0, pf.to_bytes(), Vs, gadget_v) == R.OK
    pf2, _, _ = P.prove(gens, CAP, st0, vals, bl, gadget_p, bytes(32))
    assert pf2.to_bytes() != pf.to_bytes()           # the thread_rng bytes reach the blindings
    assert P.verify(gens, CAP, st0, pf2.to_bytes(), Vs, gadget_v) == R.OK


def test_recorder_refuses_missing_assignments_and_challenge_products():
    from bulletproofs_amd import r1cs
    cs = r1cs.Prover(bytes(208))
    with pytest.raises(r1cs.R1CSError):
        cs.allocate(None)
    with pytest.raises(r1cs.R1CSError):
        cs.allocate_multiplier(None)
    cs = r1cs.Prover(bytes(208))
    x = cs.commit(3, 4)

    def cb(cs):
        a, b = cs.challenge_scalar(b"a"), cs.challenge_scalar(b"b")
        cs.allocate((x * a) * b)

    cs.specify_randomized_constraints(cb)
    with pytest.raises(r1cs.R1CSError):
        cs.descriptor()
    cs = r1cs.Prover(bytes(208))
    a = cs.allocate(1)
    with pytest.raises(r1cs.R1CSError):   # the open pair's right half has no value yet
        cs.multiply(a + r1cs.Variable(r1cs.KIND_R, 0), 1)


def test_recorder_refuses_a_right_half_that_reads_a_later_multiplier():
    """the reference allows it (assignments are values there); the witness program fills multipliers in index order"""
    from bulletproofs_amd import r1cs
    cs = r1cs.Prover(bytes(208))
    x = cs.commit(3, 4)
    cs.allocate_multiplier((1, 2))
    a = cs.allocate(x * 1)                            # L_1: the pair stays open
    _, _, o2 = cs.multiply(x + a, x - 2)              # multiplier 2 reads L_1: fine
    with pytest.raises(r1cs.R1CSError, match="an input of multiplier 1 reads multiplier 2"):
        cs.allocate(o2 + 1)                           # R_1 from O_2
    cs = r1cs.Prover(bytes(208))
    x = cs.commit(3, 4)
    l0, _, o0 = cs.allocate_multiplier((1, 2))
    a = cs.allocate(x * 1)
    cs.multiply(x + a, x - 2)
    cs.allocate(o0 + l0)                              # R_1 from multiplier 0, allocated before the pair was opened: recorded
    assert cs.src_right[1] == len(cs.rows) - 1 and len(cs.src_left) == 3


# ---- bpgpu_r1cs_witness_create through the library (host only) ---------------------------------------------------------------
def _circuit():
    """m = 2, n1 = 1, n2 = 2, one challenge"""
    from bulletproofs_amd import r1cs
    return r1cs.Circuit(2, 1, 2, True, [b"c"], [[((R.KIND_L, 0), None, 0, 1)]])


BASE_ROWS = [[(R.KIND_V, 0, 0xffffffff, 0, 1), (R.KIND_ONE, 0, 0xffffffff, 0, 2)],       # row 0: v_0 + 2 (phase 1)
             [(R.KIND_L, 0, 0xffffffff, 0, 3), (R.KIND_V, 1, 0, 1, 5)],                   # row 1: 3 L_0 + 5 c v_1
             [(R.KIND_O, 1, 0xffffffff, 0, 1), (R.KIND_ONE, 0, 0, 2, 7)]]                 # row 2: O_1 + 7 c^2


def _wcreate(circuit, n_free=2, src_left=None, src_right=None, rows=None, row_ptr=None):
    from bulletproofs_amd import r1cs
    L = r1cs.lib()
    FREE = r1cs.SRC_FREE
    src_left = [0, 1, FREE | 0] if src_left is None else src_left
    src_right = [FREE | 1, r1cs.SRC_ZERO, 2] if src_right is None else src_right
    rows = BASE_ROWS if rows is None else rows
    terms = [t for r in rows for t in r]
    if row_ptr is None:
        row_ptr = [0]
        for r in rows:
            row_ptr.append(row_ptr[-1] + len(r))
    u32 = C.c_uint32
    arr = lambda xs: (u32 * max(len(xs), 1))(*xs)
    coeff = b"".join((t[4] if isinstance(t[4], bytes) else t[4].to_bytes(32, "little")) for t in terms)
    h = C.c_void_p()
    rc = L.bpgpu_r1cs_witness_create(circuit._h, n_free, arr(src_left), arr(src_right), len(row_ptr) - 1, arr(row_ptr), len(terms),
                                     bytes(t[0] for t in terms), arr([t[1] for t in terms]), arr([t[2] for t in terms]),
                                     arr([t[3] for t in terms]), coeff, C.byref(h))
    if rc == 0:
        L.bpgpu_r1cs_witness_destroy(h)
    else:
        assert not h.value
    return rc


def test_witness_create_accepts_a_valid_program():
    assert _wcreate(_circuit()) == 0


@pytest.mark.parametrize("what", ["kind", "L index", "V index", "ONE index", "challenge index", "power without challenge",
                                  "challenge without power", "power too big", "coeff", "row_ptr end", "row_ptr decreasing",
                                  "row out of range", "reads a later multiplier", "reads itself", "challenge in phase 1",
                                  "free out of range", "free used twice", "free unused", "too many free"])
def test_witness_create_refuses_malformed_fields(what):
    from bulletproofs_amd import r1cs
    FREE = r1cs.SRC_FREE
    rows = [list(r) for r in BASE_ROWS]
    kw = {}
    if what == "kind":
        rows[1][0] = (5, 0, 0xffffffff, 0, 3)
    elif what == "L index":
        rows[1][0] = (R.KIND_L, 3, 0xffffffff, 0, 3)
    elif what == "V index":
        rows[0][0] = (R.KIND_V, 2, 0xffffffff, 0, 1)
    elif what == "ONE index":
        rows[0][1] = (R.KIND_ONE, 1, 0xffffffff, 0, 2)
    elif what == "challenge index":
        rows[1][1] = (R.KIND_V, 1, 1, 1, 5)
    elif what == "power without challenge":
        rows[0][0] = (R.KIND_V, 0, 0xffffffff, 1, 1)
    elif what == "challenge without power":
        rows[1][1] = (R.KIND_V, 1, 0, 0, 5)
    elif what == "power too big":
        rows[1][1] = (R.KIND_V, 1, 0, 256, 5)
    elif what == "coeff":
        rows[0][1] = (R.KIND_ONE, 0, 0xffffffff, 0, R.L)
    elif what == "row_ptr end":
        kw["row_ptr"] = [0, 2, 4, 5]
    elif what == "row_ptr decreasing":
        kw["row_ptr"] = [0, 3, 2, 6]
    elif what == "row out of range":
        kw["src_left"] = [0, 3, FREE | 0]
    elif what == "reads a later multiplier":
        rows[1][0] = (R.KIND_L, 2, 0xffffffff, 0, 3)
    elif what == "reads itself":
        rows[1][0] = (R.KIND_R, 1, 0xffffffff, 0, 3)
    elif what == "challenge in phase 1":   # multiplier 0 from a row over V_1 alone, with the challenge
        rows.append([(R.KIND_V, 1, 0, 1, 5)])
        kw["src_left"] = [3, 1, FREE | 0]
    elif what == "free out of range":
        kw["src_right"] = [FREE | 2, r1cs.SRC_ZERO, 2]
    elif what == "free used twice":
        kw["src_right"] = [FREE | 0, r1cs.SRC_ZERO, 2]
    elif what == "free unused":
        kw["n_free"] = 3
    elif what == "too many free":
        kw["n_free"] = 7
    assert _wcreate(_circuit(), rows=rows, **kw) == -1
