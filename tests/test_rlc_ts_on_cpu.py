"""The front end of the mixed-shape combined check on caller-supplied transcripts without a GPU: rlc_mix.h's lane body rm_front_thread compiled
for the host (tests/rlc_ts_harness) in its two forms -- the per-shape script from ts_in and the byte-wise replay -- at EVERY STROBE start
position, against each other and against the oracle's verify_ts."""
import ctypes as C
import hashlib
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(8, 1), (8, 2)]
NPOS = 166   # STROBE's rate: the positions a transcript can sit at


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rlcts") / "librlcts.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "rlc_ts_harness", "harness.cpp")])
    lib = C.CDLL(so)
    lib.rlcts_field_words.restype = C.c_uint32
    return lib


def bound_state(oracle, tag, length):
    """a history like _bound_state of tests/test_gpu_transcripts.py -- a session message, a challenge the application drew -- that ends in a
    message `length` bytes long (a challenge resets the position, so the message follows it): one more byte moves the start position of
    everything the verifier appends by one"""
    st = oracle.transcript_new(b"payment-protocol v3")
    st = oracle.transcript_append_message(st, b"session", hashlib.shake_256(b"sess" + tag).digest(40))
    st, _ = oracle.transcript_challenge_bytes(st, b"binding", 16)
    st = oracle.transcript_append_message(st, b"amount-commitment-context", hashlib.shake_256(b"ctx" + tag).digest(length))
    return st


def front(harness, n, m, proofs, pl, coms, rng, rho, states, form):
    nb = len(proofs) // pl
    k = (n * m).bit_length() - 1
    U = 4 + 2 * k + m
    nf = harness.rlcts_field_words(n, m, nb)
    status, ts = C.create_string_buffer(nb), C.create_string_buffer(208 * nb)
    fields, uniq = (C.c_uint32 * nf)(), (C.c_uint32 * (nb * U * 8))()
    rc = harness.rlcts_front(n, m, nb, proofs, pl, coms, rng, rho, states, form, status, ts, fields, uniq)
    return rc, status.raw, ts.raw, bytes(fields), bytes(uniq)


@pytest.fixture(scope="module")
def sweep(oracle, oracle_gens_64_8):
    """per shape and per session length 0 .. 165: four proofs on two states of one position -- two good ones, a copy with a non-canonical
    t_x, a copy with the identity as L_1 -- and the oracle's verdict and end state of each.  Computed once, read by every test."""
    out = {}
    for n, m in SHAPES:
        pl = oracle.proof_len(n, m)
        rows = []
        for ln in range(NPOS):
            sts, prs, cms = [], [], []
            for j in range(2):
                st = bound_state(oracle, b"%d-%d-%d" % (m, ln, j), ln)
                vals = [int.from_bytes(hashlib.shake_256(b"cv%d-%d-%d" % (ln, j, i)).digest(1), "little") for i in range(m)]
                bl = b"".join(hashlib.shake_256(b"cb%d-%d-%d" % (ln, j, i)).digest(31) + b"\x00" for i in range(m))
                pr, cm, _ = oracle.prove_ts(oracle_gens_64_8, vals, bl, n, st, b"cs%d-%d" % (ln, j))
                sts.append(st), prs.append(pr), cms.append(cm)
            bad_sc = prs[0][:128] + b"\xff" * 32 + prs[0][160:]               # t_x >= l: from_bytes fails, the transcript is never touched
            id_l1 = prs[1][:224 + 64] + bytes(32) + prs[1][224 + 96:]         # L_1 = the identity encoding: the replay ends before that message
            proofs, coms, states = prs[0] + prs[1] + bad_sc + id_l1, cms[0] + cms[1] + cms[0] + cms[1], sts[0] + sts[1] + sts[0] + sts[1]
            rng = hashlib.shake_256(b"cr%d" % ln).digest(64 * 4)
            rho = hashlib.shake_256(b"cw%d" % ln).digest(64 * 4)
            exp = [oracle.verify_ts(oracle_gens_64_8, proofs[pl * i:pl * (i + 1)], coms[32 * m * i:32 * m * (i + 1)], n, states[208 * i:208 * (i + 1)],
                                    rng[64 * i:64 * i + 64]) for i in range(4)]
            rows.append((proofs, coms, states, rng, rho, exp))
        out[(n, m)] = rows
    return out


@pytest.mark.parametrize("n,m", SHAPES)
def test_every_start_position_occurs(sweep, n, m):
    """166 consecutive message lengths walk the start position through the whole rate, the positions where the rate boundary falls inside
    the domain separator and inside a 32-byte record among them"""
    assert {row[2][200] for row in sweep[(n, m)]} == set(range(NPOS))
    assert all(row[2][200:203] == row[2][208 + 200:208 + 203] for row in sweep[(n, m)])


@pytest.mark.parametrize("n,m", SHAPES)
def test_script_and_replay_agree_and_leave_the_oracles_state(harness, oracle, sweep, n, m):
    pl = oracle.proof_len(n, m)
    for ln, (proofs, coms, states, rng, rho, exp) in enumerate(sweep[(n, m)]):
        rc0, st0, ts0, f0, u0 = front(harness, n, m, proofs, pl, coms, rng, rho, states, 0)
        rc1, st1, ts1, f1, u1 = front(harness, n, m, proofs, pl, coms, rng, rho, states, 1)
        assert rc0 == 0 and rc1 == 0, ln
        assert st0 == st1 and ts0 == ts1 and f0 == f1 and u0 == u1, ln
        assert [e[0] for e in exp] == [0, 0, 2, 1] and list(st0) == [0, 0, 2, 1], ln
        for i in range(4):
            assert ts0[208 * i:208 * (i + 1)] == exp[i][2], (ln, i)
        assert ts0[208 * 2:208 * 3] == states[:208]                     # FormatError: the input state back
        assert ts0[208 * 3:208 * 4] not in (states[208:416], exp[1][2])  # identity L_1: neither the start nor the end state


@pytest.mark.parametrize("n,m", SHAPES)
def test_replay_takes_states_at_differing_positions(harness, oracle, sweep, n, m):
    """one proof of every position in ONE group: the script refuses it (the host would not choose it), the byte-wise replay gives every
    proof what it got among its own position's proofs"""
    pl = oracle.proof_len(n, m)
    rows = sweep[(n, m)]
    pick = lambda buf, sz, i: buf[sz * i:sz * (i + 1)]
    idx = [ln % 4 for ln in range(NPOS)]     # good, good, non-canonical, identity L_1 in turn
    proofs = b"".join(pick(r[0], pl, i) for r, i in zip(rows, idx))
    coms = b"".join(pick(r[1], 32 * m, i) for r, i in zip(rows, idx))
    states = b"".join(pick(r[2], 208, i) for r, i in zip(rows, idx))
    rng = b"".join(pick(r[3], 64, i) for r, i in zip(rows, idx))
    rho = b"".join(pick(r[4], 64, i) for r, i in zip(rows, idx))
    assert front(harness, n, m, proofs, pl, coms, rng, rho, states, 0)[0] == -2
    rc, st, ts, _, _ = front(harness, n, m, proofs, pl, coms, rng, rho, states, 1)
    assert rc == 0
    for ln, (r, i) in enumerate(zip(rows, idx)):
        assert st[ln] == r[5][i][0] and ts[208 * ln:208 * (ln + 1)] == r[5][i][2], ln
