"""R1CS proofs, host side (no GPU): the test twin's prove -> verify round trips (tests/r1cs.rs of the reference), the
recorder's descriptor against the twin's own flattening, and bpgpu_r1cs_circuit_create's validation through the library."""
import ctypes as C
import random

import pytest

import r1cs_twin as R

CAP = 128


@pytest.fixture(scope="module")
def gens(oracle):
    return oracle.Gens(CAP, 1).export()


def _shuffle_vals(k, seed):
    rnd = random.Random(seed)
    inp = [rnd.getrandbits(64) for _ in range(k)]
    out = inp[:]
    rnd.shuffle(out)
    return inp, out


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 24, 42])
def test_twin_shuffle_round_trip(gens, k):
    inp, out = _shuffle_vals(k, k)
    pf, Vs, st0 = R.prove_shuffle(gens, CAP, b"ShuffleProofTest", inp, out, b"shuffle%d" % k)
    code, _, _ = R.verify_shuffle(gens, CAP, st0, pf.to_bytes(), Vs, bytes(32))
    assert code == R.OK
    # a tampered proof and a wrong statement are rejected
    bad = bytearray(pf.to_bytes())
    bad[1 + 32 * 11 + 3] ^= 1                       # inside t_x (one-phase) or T_5 (two-phase)
    assert R.verify_shuffle(gens, CAP, st0, bytes(bad), Vs, bytes(32))[0] != R.OK
    assert R.verify_shuffle(gens, CAP, st0, pf.to_bytes(), Vs[1:2] + Vs[1:], bytes(32))[0] != R.OK


def _example(cs, v, c2):
    R.example_gadget(cs, v[0], v[1], v[2], v[3], v[4], c2)


def test_twin_example_gadget_and_serialization(gens):
    pf, Vs, st0 = R.prove_example(gens, CAP, (3, 4, 6, 1, 40), 9, b"example")
    for b in (pf.to_bytes(), pf.to_bytes(force_two_phase=True)):
        assert R.verify_with(lambda cs, v: _example(cs, v, 9), gens, CAP, st0, b, Vs, bytes(32))[0] == R.OK
        assert R.verify_with(lambda cs, v: _example(cs, v, 10), gens, CAP, st0, b, Vs, bytes(32))[0] == R.VERIFICATION_ERROR
    assert len(pf.to_bytes()) + 96 == len(pf.to_bytes(force_two_phase=True))


@pytest.mark.parametrize("n", [2, 10, 32, 63])
def test_twin_range_gadget(gens, n):
    v = random.Random(n).getrandbits(n)
    pf, Vs, st0 = R.prove_range(gens, CAP, v, n, b"range%d" % n)
    assert R.verify_with(lambda cs, x: R.range_gadget(cs, x[0], None, n), gens, CAP, st0, pf.to_bytes(), Vs, bytes(32))[0] == R.OK
    pf, Vs, st0 = R.prove_range(gens, CAP, 1 << n, n, b"range-out%d" % n)      # out of range (tests/r1cs.rs:416)
    assert R.verify_with(lambda cs, x: R.range_gadget(cs, x[0], None, n), gens, CAP, st0, pf.to_bytes(), Vs, bytes(32))[0] == R.VERIFICATION_ERROR


def test_twin_exit_paths(gens):
    pf, Vs, st0 = R.prove_example(gens, CAP, (3, 4, 6, 1, 40), 9, b"exits")
    good = pf.to_bytes()
    run = lambda b, vs=Vs: R.verify_with(lambda cs, v: _example(cs, v, 9), gens, CAP, st0, b, vs, bytes(32))
    assert run(good[:-1])[0] == R.FORMAT_ERROR and run(good[:-1])[2] == st0        # from_bytes: transcript untouched
    assert run(bytes([2]) + good[1:])[0] == R.FORMAT_ERROR
    assert run(good[:1 + 32 * 8] + b"\xff" * 32 + good[1 + 32 * 9:])[0] == R.FORMAT_ERROR   # t_x not canonical
    assert run(good[:1] + bytes(32) + good[33:])[0] == R.VERIFICATION_ERROR              # identity A_I1
    assert run(good + bytes(64))[0] == R.VERIFICATION_ERROR                              # IPP of the wrong length
    assert run(good, Vs[1:] + Vs[:1])[0] == R.VERIFICATION_ERROR
    assert R.verify_with(lambda cs, v: _example(cs, v, 9), gens, 0, st0, good, Vs, bytes(32))[0] == R.INVALID_GENERATORS_LENGTH


# ---- the product's recorder ------------------------------------------------------------------------------------------------
def _record(gadget, m, st0=bytes(208)):
    from bulletproofs_amd import r1cs
    cs = r1cs.Verifier(st0)
    vs = [cs.commit(bytes(32)) for _ in range(m)]
    gadget(cs, vs)
    return cs


def _twin_weights(gadget, m, z, challenges):
    """the twin verifier run directly, its challenge draws replaced by the given values"""
    return R.flattened_with(gadget, m, z, challenges)


@pytest.mark.parametrize("name,m,gadget", [
    ("shuffle5", 10, lambda cs, v: R.shuffle_gadget(cs, v[:5], v[5:])),
    ("shuffle1", 2, lambda cs, v: R.shuffle_gadget(cs, v[:1], v[1:])),
    ("example", 5, lambda cs, v: R.example_gadget(cs, v[0], v[1], v[2], v[3], v[4], 9)),
    ("range", 1, lambda cs, v: R.range_gadget(cs, v[0], None, 8)),
])
def test_recorder_descriptor_flattens_like_the_twin(name, m, gadget):
    from bulletproofs_amd import r1cs
    rnd = random.Random(name)
    for _ in range(3):
        z = rnd.randrange(R.L)
        cs = _record(gadget, m)
        d = cs.descriptor()
        ch = [rnd.randrange(R.L) for _ in d[4]]
        assert r1cs.flattened_constraints(d, z, ch) == _twin_weights(gadget, m, z, ch)
    assert d[3] == (name.startswith("shuffle") and name != "shuffle1")


def test_recorder_refuses_products_of_two_challenges():
    from bulletproofs_amd import r1cs
    cs = r1cs.Verifier(bytes(208))
    x = cs.commit(bytes(32))

    def cb(cs):
        a, b = cs.challenge_scalar(b"a"), cs.challenge_scalar(b"b")
        cs.constrain((x - a) * a)          # the same challenge twice: power 2, fine
        with pytest.raises(r1cs.R1CSError):
            (x - a) * b
    cs.specify_randomized_constraints(cb)
    d = cs.descriptor()
    assert d[4] == [b"a", b"b"] and any(pw == 2 for (_, ch, pw, _) in d[5][0])


def test_recorder_accepts_a_challenge_monomial_on_the_right():
    """lc * (c * c): c * c is a Scalar in the reference, a pure challenge monomial (one ONE term with a challenge) here"""
    from bulletproofs_amd import r1cs
    cs = r1cs.Verifier(bytes(208))
    x, y = cs.commit(bytes(32)), cs.commit(bytes(32))

    def cb(cs):
        a, b = cs.challenge_scalar(b"a"), cs.challenge_scalar(b"b")
        lc = x * 5 - y + 7
        assert (lc * (a * a)).terms == (lc * a * a).terms == ((a * a) * lc).terms
        assert (lc * (a * a * 3)).terms == (lc * 3 * a * a).terms
        assert ((lc * a) * (a * a)).terms == (lc * a * a * a).terms and all(t[2] == 3 for t in (lc * a * (a * a)).terms)
        assert (x * (b * b)).terms == [((r1cs.KIND_V, 0), 1, 2, 1)]
        cs.constrain(lc * (a * a) - lc * a * a)
        with pytest.raises(r1cs.R1CSError):
            (lc * a) * (b * b)              # two different challenges
        with pytest.raises(TypeError):
            lc * (a * a + 1)                # not a monomial
        with pytest.raises(TypeError):
            lc * (x * a)                    # a variable times a challenge is no scalar
        with pytest.raises(TypeError):
            lc * lc
    cs.specify_randomized_constraints(cb)
    d = cs.descriptor()
    z, ch = 12345, [777, 999]
    assert r1cs.flattened_constraints(d, z, ch) == ([], [], [], [0, 0], 0)
    g = lambda cs_, v: cs_.specify_randomized_constraints(lambda c: c.constrain((v[0] * 5 - v[1] + 7) * (lambda a: a * a)(c.challenge_scalar(b"a"))))
    rec = _record(g, 2)
    assert r1cs.flattened_constraints(rec.descriptor(), z, ch[:1]) == _twin_weights(g, 2, z, ch[:1])


def test_proof_serialization_round_trip(gens):
    from bulletproofs_amd import r1cs
    pf, _, _ = R.prove_example(gens, CAP, (3, 4, 6, 1, 40), 9, b"ser")
    b0, b1 = pf.to_bytes(), pf.to_bytes(force_two_phase=True)
    assert r1cs.R1CSProof.from_bytes(b0).to_bytes() == b0 and r1cs.R1CSProof.from_bytes(b1).to_bytes() == b0
    for bad in (b"", bytes([3]) + b0[1:], b0[:-1], b0[:1 + 32 * 10]):
        with pytest.raises(r1cs.FormatError):
            r1cs.R1CSProof.from_bytes(bad)


# ---- bpgpu_r1cs_circuit_create through the library (host only) ---------------------------------------------------------------
def _create(m=2, n1=1, n2=1, two_phase=1, labels=(b"c",), rows=None, terms=None):
    from bulletproofs_amd import r1cs
    L = r1cs.lib()
    if terms is None:   # (kind, index, challenge, power, coeff)
        terms = [(R.KIND_L, 0, 0xffffffff, 0, 1), (R.KIND_V, 1, 0, 1, 5), (R.KIND_ONE, 0, 0, 2, R.L - 1), (R.KIND_O, 1, 0xffffffff, 0, 3)]
    if rows is None:
        rows = [0, 2, len(terms)]
    u32 = C.c_uint32
    nt = len(terms)
    h = C.c_void_p()
    arr = lambda xs: (u32 * max(len(xs), 1))(*xs)
    coeff = b"".join((t[4] if isinstance(t[4], bytes) else t[4].to_bytes(32, "little")) for t in terms)
    rc = L.bpgpu_r1cs_circuit_create(m, n1, n2, two_phase, len(labels), b"".join(labels), arr([len(x) for x in labels]), len(rows) - 1,
                                     arr(rows), nt, bytes(t[0] for t in terms), arr([t[1] for t in terms]), arr([t[2] for t in terms]),
                                     arr([t[3] for t in terms]), coeff, C.byref(h))
    if rc == 0:
        pn, nu = C.c_size_t(), C.c_size_t()
        assert L.bpgpu_r1cs_circuit_shape(h, C.byref(pn), C.byref(nu)) == 0
        L.bpgpu_r1cs_circuit_destroy(h)
        return rc, pn.value, nu.value
    assert not h.value
    return rc, None, None


def test_circuit_create_accepts_valid_circuits():
    assert _create() == (0, 2, 11 + 2 + 2)
    assert _create(m=0, n1=0, n2=0, two_phase=0, labels=(), rows=[0], terms=[]) == (0, 1, 11)    # n = 0: padded_n = 1, no IPP rounds
    assert _create(n1=3, n2=2)[:2] == (0, 8)


@pytest.mark.parametrize("what", ["kind", "L index", "V index", "ONE index", "challenge", "power without challenge",
                                  "challenge without power", "power too big", "coeff", "rows", "rows decreasing", "one-phase with n2",
                                  "one-phase with challenges", "two_phase flag", "too many vars", "label too long"])
def test_circuit_create_refuses_malformed_fields(what):
    base = [(R.KIND_L, 0, 0xffffffff, 0, 1), (R.KIND_V, 1, 0, 1, 5), (R.KIND_ONE, 0, 0, 2, 7), (R.KIND_O, 1, 0xffffffff, 0, 3)]
    kw = {}
    t = list(base)
    if what == "kind":
        t[0] = (5, 0, 0xffffffff, 0, 1)
    elif what == "L index":
        t[0] = (R.KIND_L, 2, 0xffffffff, 0, 1)
    elif what == "V index":
        t[1] = (R.KIND_V, 2, 0, 1, 5)
    elif what == "ONE index":
        t[2] = (R.KIND_ONE, 1, 0, 2, 7)
    elif what == "challenge":
        t[1] = (R.KIND_V, 1, 1, 1, 5)
    elif what == "power without challenge":
        t[0] = (R.KIND_L, 0, 0xffffffff, 1, 1)
    elif what == "challenge without power":
        t[1] = (R.KIND_V, 1, 0, 0, 5)
    elif what == "power too big":
        t[1] = (R.KIND_V, 1, 0, 256, 5)
    elif what == "coeff":
        t[3] = (R.KIND_O, 1, 0xffffffff, 0, R.L)
    elif what == "rows":
        kw["rows"] = [0, 2, 3]
    elif what == "rows decreasing":
        kw["rows"] = [0, 3, 2, 4]
    elif what == "one-phase with n2":
        kw.update(two_phase=0, labels=())
        t = [x for x in t if x[2] == 0xffffffff]
        kw["rows"] = [0, len(t)]
    elif what == "one-phase with challenges":
        kw.update(two_phase=0, n1=2, n2=0)
    elif what == "two_phase flag":
        kw["two_phase"] = 2
    elif what == "too many vars":
        kw["n1"] = 65536
    elif what == "label too long":
        kw["labels"] = (b"x" * 1025,)
    assert _create(terms=t, **kw)[0] == -1
