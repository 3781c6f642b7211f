"""The R1CS witness check on the GPU: bpgpu_r1cs_witness_check on hand-built circuits whose failing sets are known exactly, on rows
of every length around the chunk size, on challenge powers, and on recorded gadgets against the pure-Python twin
(tests/r1cs_check_twin.py); bpgpu_r1cs_prove_batch_checked against bpgpu_r1cs_prove_batch byte for byte."""
import ctypes as C
import hashlib
import random

import pytest

import r1cs_check_twin as K
import r1cs_corpus as G
import r1cs_prover_twin as P
import r1cs_twin as R

pytestmark = pytest.mark.gpu

CAP = 128
L = R.L
SAT = 0xffffffff
V, ONE = 3, 4


@pytest.fixture(scope="module")
def gens(oracle):
    return oracle.Gens(CAP, 1).export()


@pytest.fixture(scope="module")
def ctx():
    import bulletproofs_amd as bp
    c = bp.Context(0)
    c.gens_create(CAP, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bare():
    """a context on which gens_create was never called"""
    import bulletproofs_amd as bp
    c = bp.Context(0)
    yield c
    c.close()


def _enc(xs):
    return b"".join((x % L).to_bytes(32, "little") for x in xs)


def _hand(m, cons, labels=()):
    """a circuit over committed variables only, through bpgpu_r1cs_circuit_create, and its (empty) witness program"""
    from bulletproofs_amd import r1cs
    circuit = r1cs.Circuit(m, 0, 0, bool(labels), list(labels), cons)
    return circuit, r1cs.Witness(circuit, 0, [], [], [])


def _raw(c, circuit, witness, nb, v, free=b"", chal=None, stride=None, fill=0xff):
    """bpgpu_r1cs_witness_check itself, the outputs pre-filled: (rc, first, count, maps, status)"""
    from bulletproofs_amd import r1cs
    Q = circuit.n_constraints
    stride = (Q + 7) // 8 if stride is None else stride
    first, count = (C.c_uint32 * max(nb, 1))(*[7] * max(nb, 1)), (C.c_uint32 * max(nb, 1))(*[7] * max(nb, 1))
    maps = C.create_string_buffer(bytes([fill]) * (stride * max(nb, 1)), stride * max(nb, 1) + 1)
    status = C.create_string_buffer(b"\x07" * max(nb, 1), max(nb, 1) + 1)
    rc = r1cs.lib().bpgpu_r1cs_witness_check(c.h, circuit._h, witness._h, nb, v, free, chal, first, count, maps, stride, status)
    return rc, list(first[:nb]), list(count[:nb]), [maps.raw[b * stride:(b + 1) * stride] for b in range(nb)], status.raw[:nb]


def _map(bad, stride):
    mp = bytearray(stride)
    for q in bad:
        mp[q // 8] |= 1 << (q % 8)
    return bytes(mp)


# ---- 1. hand-built circuits: V_j - c_j ONE ---------------------------------------------------------------------------------
def _consts(Q):
    return [1000 + 17 * j for j in range(Q)]


def _vj_circuit(Q):
    return _hand(Q, [[((V, j), None, 0, 1), ((ONE, 0), None, 0, -c % L)] for j, c in enumerate(_consts(Q))])


@pytest.mark.parametrize("nb", [1, 63, 64, 65])
@pytest.mark.parametrize("Q", [1, 8, 9, 33])
def test_hand_built_failing_sets(bare, Q, nb):
    circuit, witness = _vj_circuit(Q)
    rnd = random.Random(Q * 100 + nb)
    everyone = list(range(Q))
    plans = {
        "mixed": lambda p: [0] if p == 0 else [Q - 1] if p == nb - 1 else everyone if p == 1 else sorted(rnd.sample(everyone, rnd.randrange(Q + 1))) if p % 5 == 2 else [],
        "proof0": lambda p: everyone if p == 0 else [],
        "last": lambda p: [Q - 1] if p == nb - 1 else [],
        "none": lambda p: [],
    }
    stride = (Q + 7) // 8 + 3
    for name, plan in plans.items():
        bad = [plan(p) for p in range(nb)]
        v = b"".join(_enc([c + (1 if j in bad[p] else 0) for j, c in enumerate(_consts(Q))]) for p in range(nb))
        rc, first, count, maps, status = _raw(bare, circuit, witness, nb, v, stride=stride)
        assert rc == 0 and status == bytes(nb), name
        assert first == [b[0] if b else SAT for b in bad], name
        assert count == [len(b) for b in bad], name
        assert maps == [_map(b, stride) for b in bad], name      # (the bytes past ceil(Q / 8) are zero)


def test_empty_circuit_and_empty_constraint(bare):
    circuit, witness = _hand(0, [])                                  # Q = 0, n = 0, m = 0
    rc, first, count, maps, status = _raw(bare, circuit, witness, 3, b"", stride=2)
    assert (rc, first, count, maps, status) == (0, [SAT] * 3, [0] * 3, [bytes(2)] * 3, bytes(3))
    assert _raw(bare, circuit, witness, 0, b"")[0] == 0              # nbatch = 0
    circuit, witness = _hand(1, [[], [((V, 0), None, 0, 1)], []])    # empty constraints around one that fails for v != 0
    rc, first, count, maps, status = _raw(bare, circuit, witness, 2, _enc([0, 5]))
    assert (rc, first, count, maps, status) == (0, [SAT, 1], [0, 1], [b"\x00", b"\x02"], bytes(2))


def test_argument_checks_with_a_context(bare):
    from bulletproofs_amd import r1cs
    circuit, witness = _hand(2, [[((V, 0), 0, 1, 1), ((V, 1), None, 0, 1)]] * 9, labels=[b"c"])
    other, other_w = _vj_circuit(1)
    v, ch = _enc([0, 0]), _enc([3])
    assert _raw(bare, circuit, witness, 1, v, chal=ch)[0] == 0
    assert _raw(bare, circuit, witness, 1, v, chal=None)[0] == -1
    assert _raw(bare, circuit, witness, 1, v, chal=ch, stride=1)[0] == -1
    assert _raw(bare, circuit, other_w, 1, v, chal=ch)[0] == -1
    assert r1cs.STATUS_UNSATISFIED == 3 and r1cs.SATISFIED == SAT


# ---- 2. reduction mod l ------------------------------------------------------------------------------------------------------
def test_residual_is_reduced_mod_l(bare):
    circuit, witness = _hand(2, [[((V, 0), None, 0, 1), ((V, 1), None, 0, 1)]])
    rc, first, count, _, status = _raw(bare, circuit, witness, 2, _enc([1, L - 1]) + _enc([1, L - 2]))
    assert (rc, first, count, status) == (0, [SAT, 0], [0, 1], bytes(2))


# ---- 3. row lengths ------------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 600]


def test_chunk(tmp_path):
    lib = C.CDLL(K.build_harness(tmp_path))
    assert lib.r1ch_chunk() in (32, 64, 128, 256)


def test_row_lengths(bare):
    """every length satisfied, and once with its last term's variable off by one: that row alone fails"""
    from bulletproofs_amd import r1cs
    broken = [r for r, ln in enumerate(LENGTHS) if ln]
    provers = [K.long_row_prover(LENGTHS)] + [K.long_row_prover(LENGTHS, broken=r) for r in broken]
    first, count, maps = r1cs.check_batch(bare, provers, want_count=True, want_map=True)
    assert first == [None] + broken and count == [0] + [1] * len(broken)
    assert maps == [_map([], 2)] + [_map([r], 2) for r in broken]


def test_short_row_failing_behind_a_long_one(bare):
    from bulletproofs_amd import r1cs
    lengths = [600, 3, 257, 2, 0, 129, 1]
    provers = [K.long_row_prover(lengths, broken=r) for r in (1, 3, 6, 2, None)]
    assert r1cs.check_batch(bare, provers) == [1, 3, 6, 2, None]


# ---- 4. challenge arithmetic -------------------------------------------------------------------------------------------------
def test_challenge_powers_indices_and_per_proof_values(bare):
    # row 0: c0^255 V_0 - c0^255 V_1; row 1: c1 V_2 - c1^2 V_3 with v_2 = c1 v_3
    cons = [[((V, 0), 0, 255, 1), ((V, 1), 0, 255, L - 1)], [((V, 2), 1, 1, 1), ((V, 3), 1, 2, L - 1)]]
    circuit, witness = _hand(4, cons, labels=[b"first", b"second"])
    nb = 65
    rnd = random.Random(4)
    ch = [[rnd.randrange(1, L), rnd.randrange(1, L)] for _ in range(nb)]
    base = [[rnd.randrange(L)] * 2 + [c[1] * (7 + p) % L, 7 + p] for p, c in enumerate(ch)]
    chal = b"".join(_enc(c) for c in ch)
    rc, first, count, _, status = _raw(bare, circuit, witness, nb, b"".join(_enc(v) for v in base), chal=chal)
    assert (rc, first, count, status) == (0, [SAT] * nb, [0] * nb, bytes(nb))
    # v_0 moves by one in the even proofs (row 0 fails), v_2 in the odd ones (row 1 fails)
    moved = [[v[0] + 1, v[1], v[2], v[3]] if p % 2 == 0 else [v[0], v[1], v[2] + 1, v[3]] for p, v in enumerate(base)]
    rc, first, count, _, status = _raw(bare, circuit, witness, nb, b"".join(_enc(v) for v in moved), chal=chal)
    assert (rc, first, count, status) == (0, [p % 2 for p in range(nb)], [1] * nb, bytes(nb))
    # the proofs' challenge rows swapped round: v_2 = c1 v_3 no longer holds under a neighbour's c1
    swapped = b"".join(_enc(ch[(p + 1) % nb]) for p in range(nb))
    rc, first, count, _, status = _raw(bare, circuit, witness, nb, b"".join(_enc(v) for v in base), chal=swapped)
    assert (rc, first, count) == (0, [1] * nb, [1] * nb)


# ---- 5. status ---------------------------------------------------------------------------------------------------------------
def test_non_canonical_inputs_void_their_proof_only(bare):
    from bulletproofs_amd import r1cs
    circuit = r1cs.Circuit(1, 1, 0, True, [b"c"], [[((V, 0), None, 0, 1), ((ONE, 0), None, 0, L - 5)]])
    witness = r1cs.Witness(circuit, 2, [r1cs.SRC_FREE | 0], [r1cs.SRC_FREE | 1], [])
    big = b"\xff" * 32
    v = big + _enc([6, 6, 6])                                        # proof 0: v >= l
    free = _enc([1, 2]) + _enc([1])[:32] + big + _enc([1, 2, 1, 2])  # proof 1: a free input >= l
    chal = _enc([3, 3]) + big + _enc([3])                            # proof 2: a challenge >= l
    rc, first, count, maps, status = _raw(bare, circuit, witness, 4, v, free=free, chal=chal)
    assert rc == 0 and list(status) == [2, 2, 2, 0]
    assert first == [SAT, SAT, SAT, 0] and count == [0, 0, 0, 1] and maps == [b"\x00"] * 3 + [b"\x01"]


# ---- 6. recorded gadgets -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.CASES, ids=[c[0] for c in K.CASES])
def test_recorded_gadgets_match_the_twin(bare, case):
    from bulletproofs_amd import r1cs
    _, _, _, Q, nch, bad = case
    rec = K.record(case)
    first, count, maps = r1cs.check_batch(bare, [rec, rec], [K.CHALLENGE] * nch, want_count=True, want_map=True)
    assert first == [bad[0] if bad else None] * 2 and count == [len(bad)] * 2 and maps == [_map(bad, (Q + 7) // 8)] * 2
    assert rec.which_is_unsatisfied(bare) == (bad[0] if bad else None)      # (challenges drawn by the call)


def test_check_raises_unsatisfied(bare):
    from bulletproofs_amd import r1cs
    rec = K.record(K.CASES[1], locate=True)
    with pytest.raises(r1cs.Unsatisfied) as e:
        rec.check(bare)
    assert e.value.constraint == 8 and "r1cs_twin.py" in e.value.where
    K.record(K.CASES[0]).check(bare)


@pytest.mark.parametrize("name", ["n5", "powers", "open_ends"])
def test_two_phase_corpus_case_is_satisfied(bare, name):
    from bulletproofs_amd import r1cs
    case = [c for c in G.SMALL if c.name == name][0]
    provers = [G.record_prover(case, idx) for idx in range(3)]
    assert provers[0].descriptor()[3] and provers[0].descriptor()[2] > 0
    first, count = r1cs.check_batch(bare, provers, want_count=True)
    assert first == [None] * 3 and count == [0] * 3


# ---- 7. the checked prover -----------------------------------------------------------------------------------------------------
def _scalars(tag, n):
    return [int.from_bytes(hashlib.shake_256(tag + b"%d" % i).digest(64), "little") % L for i in range(n)]


def _checked_against_unchecked(c, gens, gadget, vals_list, bad_at, want_first, tag):
    from bulletproofs_amd import r1cs
    nb = len(vals_list)
    st0s = [R.transcript_state(R.T.Transcript(tag + b"%d" % b)) for b in range(nb)]
    rng = hashlib.shake_256(b"checked rng " + tag).digest(32 * nb)
    provers, bls = [], []
    for b, vals in enumerate(vals_list):
        cs = r1cs.Prover(st0s[b])
        bls.append(_scalars(tag + b"bl%d-" % b, len(vals)))
        gadget(cs, [cs.commit(v, x) for v, x in zip(vals, bls[b])])
        provers.append(cs)
    ins = [p.inputs() for p in provers]
    args = (c, provers[0].circuit(), nb, b"".join(i[0] for i in ins), b"".join(i[1] for i in ins), b"".join(i[2] for i in ins), b"".join(st0s), rng)
    w = provers[0].witness()
    proofs0, coms0, status0, ts0 = w.prove_batch(*args, want_transcripts=True)
    proofs, coms, status, ts, first = w.prove_batch(*args, want_transcripts=True, check=True)
    assert status0 == bytes(nb) and coms == coms0
    for b in range(nb):
        if b == bad_at:
            continue
        assert proofs[b] == proofs0[b] and len(proofs[b]) > 0 and ts[208 * b:208 * (b + 1)] == ts0[208 * b:208 * (b + 1)], b
    assert list(status) == [r1cs.STATUS_UNSATISFIED if b == bad_at else 0 for b in range(nb)]
    assert first == [want_first if b == bad_at else SAT for b in range(nb)]
    assert proofs[bad_at] == b"" and ts[208 * bad_at:208 * (bad_at + 1)] == st0s[bad_at]
    # the index is the twin's under the challenges the proof's own transcript produced
    _, _, twin = P.prove(gens, CAP, st0s[bad_at], vals_list[bad_at], bls[bad_at], gadget, rng[32 * bad_at:32 * bad_at + 32])
    assert K.unsatisfied(provers[bad_at], twin.challenges)[0] == want_first
    with pytest.raises(r1cs.Unsatisfied, match=r"proof %d of the batch" % bad_at) as e:
        r1cs.prove_batch(c, provers, rng, check=True)
    assert e.value.constraint == want_first and e.value.position == bad_at
    good = [p for b, p in enumerate(provers) if b != bad_at]
    rng_good = b"".join(rng[32 * b:32 * b + 32] for b in range(nb) if b != bad_at)
    assert [p.to_bytes() for p, _ in r1cs.prove_batch(c, good, rng_good, check=True)] == [proofs0[b] for b in range(nb) if b != bad_at]
    assert c.get_option("staging_residue") == 0


@pytest.mark.parametrize("ct", [0, 1])
def test_checked_prover_shuffle(ctx, gens, ct):
    ctx.set_option("prover_constant_time", ct)
    try:
        vals = [[1, 2, 3, 3, 1, 2], [4, 5, 6, 6, 5, 4], [1, 2, 3, 3, 1, 4], [7, 8, 9, 7, 8, 9], [2, 2, 3, 3, 2, 2]]
        _checked_against_unchecked(ctx, gens, lambda cs, v: R.shuffle_gadget(cs, v[:3], v[3:]), vals, 2, 8, b"checked shuffle %d/" % ct)
    finally:
        ctx.set_option("prover_constant_time", 0)


def test_checked_prover_one_phase(ctx, gens):
    g = lambda cs, v: R.example_gadget(cs, v[0], v[1], v[2], v[3], v[4], 9)
    vals = [[3, 4, 6, 1, 40], [3, 4, 6, 1, 41], [1, 2, 3, 0, 0]]
    _checked_against_unchecked(ctx, gens, g, vals, 1, 2, b"checked example/")


def test_checked_prover_keeps_bad_scalar_status(ctx):
    from bulletproofs_amd import r1cs
    provers = [K.record(K.CASES[1]) for _ in range(2)]               # both unsatisfied; proof 0 also non-canonical
    ins = [p.inputs() for p in provers]
    v = bytearray(ins[0][0] + ins[1][0])
    v[31] = 0xff
    out = provers[0].witness().prove_batch(ctx, provers[0].circuit(), 2, bytes(v), ins[0][1] + ins[1][1], b"", bytes(208),
                                           hashlib.shake_256(b"bs").digest(64), check=True)
    assert list(out[2]) == [2, r1cs.STATUS_UNSATISFIED] and out[3] == [SAT, 8]


# ---- 8, 9. no generators; nothing left behind ----------------------------------------------------------------------------------
def test_check_needs_no_generators_and_leaves_no_secrets():
    import bulletproofs_amd as bp
    from bulletproofs_amd import r1cs
    c = bp.Context(0)
    try:
        provers = [K.record(K.CASES[i % 2], st0=bytes(208)) for i in range(33)]
        assert r1cs.check_batch(c, provers) == [None, 8] * 16 + [None]
        assert c.get_option("staging_residue") == 0
        long_rows = [K.long_row_prover([600, 3], broken=b % 3 if b % 3 < 2 else None) for b in range(5)]
        assert r1cs.check_batch(c, long_rows) == [0, 1, None, 0, 1]
        assert c.get_option("staging_residue") == 0
    finally:
        c.close()
