"""Scanning range proofs under many wallet keys on the GPU (bpgpu_rangeproof_scan_batch[_dev], RangeProof.scan_batch, bulletproofs.hpp) at
n = 8 and n = 64, batches of 1, 65 and 130 rows (lane 0 alone, the lanes past the batch, a third workgroup), proofs made by
prove_batch(rewind=True) under seeds derived from (key, commitment).
REFERENCE: the existing path, run once per key -- RangeProof.rewind_seeds + bpgpu_rangeproof_rewind_batch -- and the first OK among the
keys (the header's consequence for rows where at most one key passes the 2^192 test: every row here but the forged one); at n = 8 also
tests/scan_twin.py, which states the contract itself (the lowest key that passes the test decides)."""
import ctypes as C
import hashlib
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 65, 130]
NB = 130
NS = [8, 64]
NKEYS = 5
POSITIONS = (0, 40, 100, 150, 165)
TS = 208
OK, NOT_FOUND, FORMAT = 0, 1, 2
NONE = 0xFFFFFFFF
MISS = (NOT_FOUND, NONE, 0, bytes(16), 0)
TWIN_ROWS = 6


def _pl(n):
    return 32 * (9 + 2 * (n.bit_length() - 1))


def key_of(j):
    return hashlib.sha256(b"scan wallet key %d" % j).digest()


KEYS = [key_of(j) for j in range(NKEYS)]


@pytest.fixture(scope="module")
def tw(oracle):
    import scan_twin
    return scan_twin


@pytest.fixture(scope="module")
def contexts():
    """prover_constant_time -> a context with gens_create(64, 1), made once per module"""
    import bulletproofs_amd as bp
    made = {}

    def get(ct=0):
        if ct not in made:
            ctx = bp.Context(0)
            if ct:
                ctx.set_option("prover_constant_time", 1)
            ctx.gens_create(64, 1)
            made[ct] = ctx
        return made[ct]
    yield get
    for ctx in made.values():
        ctx.close()


def _prove(ctx, n, rows, states=None):
    return ctx.rangeproof_prove_batch_rw(n, 1, [r["v"] for r in rows], b"".join(r["g"].to_bytes(32, "little") for r in rows),
                                         states if states is not None else b"".join(r["state"] for r in rows), b"".join(r["seed"] for r in rows),
                                         b"".join(r["msg"] for r in rows))


def _statements(ctx, tw, n, owner_of, tag):
    """NB statements (value, blinding, message, one of five states, owner key); the commitment comes first, the seed from (owner's key,
    commitment), then the proofs from ONE prover call"""
    import bulletproofs_amd as bp
    R = tw.R
    states = [R.state_at(pos, b"wallet") for pos in POSITIONS]
    vs, gs, ms = [0, 1, 2**n - 1], [0, 1, tw.L - 1], [bytes(16), b"\xff" * 16]
    rows = []
    for i in range(NB):
        v = vs[i] if i < 3 else R.det_scalar(tag + b"v%d" % n, i) % 2**n
        g = gs[i] if i < 3 else R.det_scalar(tag + b"g%d" % n, i)
        msg = ms[i] if i < 2 else hashlib.sha256(tag + b"msg%d" % i).digest()[:16]
        rows.append(dict(v=v, g=g, msg=msg, state=states[i % 5], owner=owner_of(i)))
    coms = ctx.pedersen_commit_batch(b"".join(r["v"].to_bytes(8, "little") for r in rows), 8, b"".join(r["g"].to_bytes(32, "little") for r in rows))[0]
    coms = [coms[32 * i:32 * i + 32] for i in range(NB)]
    per_key = {j: bp.RangeProof.rewind_seeds(ctx, key_of(j), coms) for j in sorted(set(r["owner"] for r in rows))}
    for i, r in enumerate(rows):
        r["seed"] = per_key[r["owner"]][32 * i:32 * i + 32]
    proofs, cm = _prove(ctx, n, rows)
    assert cm == b"".join(coms)
    pl = _pl(n)
    for i, r in enumerate(rows):
        r["proof"], r["V"] = proofs[pl * i:pl * i + pl], coms[i]
    return rows


@pytest.fixture(scope="module")
def ref(tw, contexts):
    """Per n, computed once and left unchanged: 130 rows whose owner is a different key per row (i mod 5; row 0 is (0, 0), V of 32 zero
    bytes), and for every key the existing path's answer for the whole batch: rewind_seeds + rangeproof_rewind_batch"""
    import bulletproofs_amd as bp
    ctx = contexts()
    out = {}
    for n in NS:
        rows = _statements(ctx, tw, n, lambda i: i % NKEYS, b"scan")
        assert rows[0]["V"] == bytes(32)
        out[n] = rows
        out[n, "per_key"] = [_rewind_under(ctx, n, rows, k) for k in KEYS]
    return out


def _rewind_under(ctx, n, rows, key, states=None):
    """the existing path for one key: (status, value, message, blinding) per row"""
    import bulletproofs_amd as bp
    coms = [r["V"] for r in rows]
    seeds = bp.RangeProof.rewind_seeds(ctx, key, coms)
    st, vals, msgs, bls = ctx.rangeproof_rewind_batch(n, b"".join(r["proof"] for r in rows), _pl(n), b"".join(coms),
                                                      states if states is not None else b"".join(r["state"] for r in rows), seeds)
    return [(st[i], vals[i], msgs[16 * i:16 * i + 16], int.from_bytes(bls[32 * i:32 * i + 32], "little")) for i in range(len(rows))]


def first_ok(per_key, nrows):
    """the first-OK rule over the per-key passes -> what the scan must return"""
    out = []
    for i in range(nrows):
        hit = [(j, pk[i]) for j, pk in enumerate(per_key) if pk[i][0] == OK]
        fmt = any(pk[i][0] == FORMAT for pk in per_key)
        out.append((OK, hit[0][0]) + hit[0][1][1:] if hit else ((FORMAT if fmt else NOT_FOUND), NONE, 0, bytes(16), 0))
    return out


def _scan(ctx, n, rows, keys, states=None):
    st, ki, vals, msgs, bls = ctx.rangeproof_scan_batch(n, b"".join(r["proof"] for r in rows), _pl(n), b"".join(r["V"] for r in rows),
                                                        states if states is not None else b"".join(r["state"] for r in rows), b"".join(keys))
    return [(st[i], ki[i], vals[i], msgs[16 * i:16 * i + 16], int.from_bytes(bls[32 * i:32 * i + 32], "little")) for i in range(len(rows))]


def _scan_dev(ctx, n, rows, keys, stream=None):
    import torch
    dev = torch.device("cuda:0")
    nb = len(rows)
    up = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)
    d_pr, d_cm, d_ts = (up(b"".join(r[k] for r in rows)) for k in ("proof", "V", "state"))
    d_k = up(b"".join(keys))
    d_st, d_m, d_g = (torch.full((k * nb,), 255, dtype=torch.uint8, device=dev) for k in (1, 16, 32))
    d_v = torch.full((nb,), -1, dtype=torch.int64, device=dev)
    d_ki = torch.full((nb,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.rangeproof_scan_batch_dev(n, nb, d_pr.data_ptr(), _pl(n), d_cm.data_ptr(), d_ts.data_ptr(), TS, d_k.data_ptr(), len(keys), d_st.data_ptr(), d_ki.data_ptr(),
                                  d_v.data_ptr(), d_m.data_ptr(), d_g.data_ptr(), stream.cuda_stream if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    else:
        ctx.synchronize()
    st, m, g = (bytes(t.cpu().numpy()) for t in (d_st, d_m, d_g))
    vals = [x % 2**64 for x in d_v.cpu().tolist()]
    ki = [x % 2**32 for x in d_ki.cpu().tolist()]
    return [(st[i], ki[i], vals[i], m[16 * i:16 * i + 16], int.from_bytes(g[32 * i:32 * i + 32], "little")) for i in range(nb)]


def _want(rows, keys=KEYS):
    idx = {k: j for j, k in reversed(list(enumerate(keys)))}
    return [(OK, idx[key_of(r["owner"])], r["v"], r["msg"], r["g"]) if key_of(r["owner"]) in idx else MISS for r in rows]


# ---- the contract -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", SIZES)
@pytest.mark.parametrize("n", NS)
def test_a_different_owner_per_row_equals_the_first_ok_of_the_per_key_passes(contexts, ref, n, nb):
    """host form, prover_constant_time, and the _dev form on a caller's stream: all identical, and equal to the existing path"""
    import torch
    rows = ref[n][:nb]
    want = first_ok([pk[:nb] for pk in ref[n, "per_key"]], nb)
    assert want == _want(rows)
    assert _scan(contexts(), n, rows, KEYS) == want
    assert _scan(contexts(1), n, rows, KEYS) == want
    stream = torch.cuda.Stream()
    assert _scan_dev(contexts(), n, rows, KEYS, stream) == want
    assert _scan_dev(contexts(1), n, rows, KEYS) == want


@pytest.mark.parametrize("n", NS)
def test_the_owner_is_key_0_or_the_last_key_and_a_duplicated_key_reports_the_lower_index(contexts, ref, n):
    rows = ref[n]
    for ct in (0, 1):
        ctx = contexts(ct)
        for owner in (0, NKEYS - 1):
            mine = [r for r in rows if r["owner"] == owner]
            got = _scan(ctx, n, mine, KEYS)
            assert got == [(OK, owner, r["v"], r["msg"], r["g"]) for r in mine], (ct, owner)
        dup = [KEYS[3], KEYS[1], KEYS[3], KEYS[1], KEYS[0]]
        assert _scan(ctx, n, rows[:65], dup) == _want(rows[:65], dup)
    assert [w[1] for w in _want(rows[:5], dup)] == [4, 1, NONE, 0, NONE]


@pytest.mark.parametrize("n", NS)
def test_a_batch_where_no_row_is_the_wallets(contexts, ref, n):
    strangers = [key_of(100 + j) for j in range(7)]
    for ct in (0, 1):
        assert _scan(contexts(ct), n, ref[n], strangers) == [MISS] * NB
    assert first_ok([_rewind_under(contexts(), n, ref[n][:65], k) for k in strangers[:2]], 65) == [MISS] * 65


@pytest.mark.parametrize("n", NS)
def test_one_key_equals_rewind_batch_byte_for_byte(contexts, ref, n):
    """nkeys = 1: status, value, message and blinding buffers are those of rangeproof_rewind_batch under that key's seeds"""
    import bulletproofs_amd as bp
    rows, ctx = ref[n], contexts()
    proofs, coms, states = (b"".join(r[k] for r in rows) for k in ("proof", "V", "state"))
    for j in (0, 2):
        seeds = bp.RangeProof.rewind_seeds(ctx, KEYS[j], [r["V"] for r in rows])
        st, vals, msgs, bls = ctx.rangeproof_rewind_batch(n, proofs, _pl(n), coms, states, seeds)
        st2, ki, vals2, msgs2, bls2 = ctx.rangeproof_scan_batch(n, proofs, _pl(n), coms, states, KEYS[j])
        assert (st2, vals2, msgs2, bls2) == (st, vals, msgs, bls)
        assert ki == [0 if s == OK else NONE for s in st] and list(st).count(OK) == NB // NKEYS


@pytest.mark.parametrize("n", NS)
def test_each_way_to_miss_stands_alone_among_good_rows(contexts, tw, ref, n):
    """One bad row per batch of 130, at the batch's start, a workgroup edge or its end: a FORMAT scalar, A / S / T_1 / T_2 of 32 zero
    bytes.  The bad row equals the per-key passes' answer, has zero outputs and key index 0xFFFFFFFF; no other row moves."""
    good = ref[n]
    pl = _pl(n)
    lb = tw.L.to_bytes(32, "little")
    zero = lambda off: (lambda r: r.update(proof=r["proof"][:off] + bytes(32) + r["proof"][off + 32:]))
    cases = [
        ("e_blinding = l", 0, lambda r: r.update(proof=r["proof"][:192] + lb + r["proof"][224:]), FORMAT),
        ("b = l", 129, lambda r: r.update(proof=r["proof"][:pl - 32] + lb), FORMAT),
        ("A of 32 zero bytes", 63, zero(0), NOT_FOUND),
        ("S of 32 zero bytes", 64, zero(32), NOT_FOUND),
        ("T_1 of 32 zero bytes", 65, zero(64), NOT_FOUND),
        ("T_2 of 32 zero bytes", 128, zero(96), NOT_FOUND),
    ]
    want = _want(good)
    for name, at, change, status in cases:
        rows = [dict(r) for r in good]
        change(rows[at])
        assert first_ok([_rewind_under(contexts(), n, [rows[at]], k) for k in KEYS], 1) == [(status,) + MISS[1:]], name
        for ct in (0, 1):
            got = _scan(contexts(ct), n, rows, KEYS)
            assert got[at] == (status,) + MISS[1:], (name, ct)
            assert got[:at] + got[at + 1:] == want[:at] + want[at + 1:], (name, ct)


def test_an_e_blinding_rewritten_for_a_lower_key_makes_the_row_not_found(contexts, tw, ref):
    """e_blinding is absorbed after x, so it can be rewritten to make another key j' pass the 2^192 test (below the owner's index or
    above it: the owner's own candidate moves away with the rewrite).  j' passes step 2 and fails at the commitment: the row is
    NOT_FOUND with zero outputs and key index 0xFFFFFFFF although the owner's key is listed, and no other row moves.  The forgery is
    made in the twin's integers on the GPU's proof; at n = 8 the twin's scan agrees and names j' as the only key that passes."""
    for n in NS:
        good = ref[n]
        for at, jp in ((64, 1), (66, 0), (129, 2), (3, 4)):       # owners 4, 1, 4, 3
            r = dict(good[at])
            assert r["owner"] == at % NKEYS and r["owner"] != jp
            r["proof"] = tw.forge_e_blinding(r["state"], r["proof"], r["V"], n, KEYS[jp], e=r["v"])
            rows = good[:at] + [r] + good[at + 1:]
            want = _want(good)
            for ct in (0, 1):
                got = _scan(contexts(ct), n, rows, KEYS)
                assert got[at] == MISS, (n, at, ct)
                assert got[:at] + got[at + 1:] == want[:at] + want[at + 1:]
            # key j' alone passes step 2 and fails step 3 -- with every other key removed the answer is the same
            assert _scan(contexts(), n, [r], [KEYS[jp]]) == [MISS]
            if n == 8:
                pc = tw.T.PedersenGens()
                assert tw.scan(pc, r["state"], r["proof"], r["V"], n, KEYS)[:5] == MISS
                x = tw.replay(r["state"], r["proof"], r["V"], n)[2]
                eb = int.from_bytes(r["proof"][192:224], "little")
                passing = [j for j, k in enumerate(KEYS) if tw.candidate(k, r["V"], x, eb)[0] >> 192 == 0]
                assert passing == [jp]


def test_rows_equal_the_twin_at_n_8(tw, ref, contexts):
    """the contract in integers, on the first rows and on one miss of each kind; the twin asserts the one-permutation claim on the way"""
    pc = tw.T.PedersenGens()
    rows = [dict(r) for r in ref[8][:TWIN_ROWS]]
    rows[1]["proof"] = bytes(32) + rows[1]["proof"][32:]
    rows[2]["proof"] = rows[2]["proof"][:192] + tw.L.to_bytes(32, "little") + rows[2]["proof"][224:]
    keys = [KEYS[4], KEYS[0], KEYS[0], KEYS[3]]
    got = _scan(contexts(), 8, rows, keys)
    for i, r in enumerate(rows):
        want = tw.scan(pc, r["state"], r["proof"], r["V"], 8, keys)
        assert got[i] == want[:5], i
        assert want[5] in (None, tw.PRF_POS)
    assert [g[0] for g in got] == [OK, NOT_FOUND, FORMAT, OK, OK, OK] and [g[1] for g in got] == [1, NONE, NONE, 3, 0, 1]


# ---- call forms -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_one_shared_state(contexts, tw, ref, n):
    """stride 0 equals per-row copies of the state, and both equal the per-key passes"""
    ctx = contexts()
    shared = tw.R.state_at(150, b"shared")
    rows = [dict(r, state=shared) for r in ref[n][:65]]
    proofs, _ = _prove(ctx, n, rows, states=shared)
    pl = _pl(n)
    for i, r in enumerate(rows):
        r["proof"] = proofs[pl * i:pl * i + pl]
    want = first_ok([_rewind_under(ctx, n, rows, k, states=shared) for k in KEYS], 65)
    assert want == _want(rows)
    for ct in (0, 1):
        assert _scan(contexts(ct), n, rows, KEYS, states=shared) == want
        assert _scan(contexts(ct), n, rows, KEYS) == want
    assert _scan(ctx, n, rows[:1], KEYS, states=shared) == want[:1]


def test_many_keys_and_the_owner_among_them(contexts, ref):
    """1 024 keys, the most a call takes, the owners' keys at 1 023, 0, 517, ...: every row found under its index"""
    rows = ref[64][:65]
    keys = [key_of(1000 + j) for j in range(1024)]
    at = [1023, 0, 517, 64, 63]
    for j, a in enumerate(at):
        keys[a] = KEYS[j]
    want = [(OK, at[r["owner"]], r["v"], r["msg"], r["g"]) for r in rows]
    assert _scan(contexts(), 64, rows, keys) == want
    assert _scan(contexts(1), 64, rows[:3], keys) == want[:3]


def test_python_api_scan_batch(tw):
    """RangeProof.scan_batch over a list of Transcript, one bound Transcript and a TranscriptBatch; keys as a list or concatenated; a
    FORMAT row raises as from_bytes would"""
    import bulletproofs_amd as bp
    gens = bp.BulletproofGens(64, 1)
    try:
        pc, n, nb = gens.pedersen(), 64, 5
        keys = [hashlib.sha256(b"api wallet %d" % j).digest() for j in range(3)]
        vals = [[0], [1], [2**64 - 1], [2**63], [12345]]
        bls = [[tw.R.det_scalar(b"api-scan", i).to_bytes(32, "little")] for i in range(nb)]
        msgs = [None, bytes(16), b"\xff" * 16, b"memo: rent, May.", None]
        owner = [2, 0, 1, None, 2]
        coms = [gens.ctx.pedersen_commit_batch(v[0].to_bytes(8, "little"), 8, b[0])[0] for v, b in zip(vals, bls)]
        per_key = [bp.RangeProof.rewind_seeds(gens, k, coms) for k in keys + [hashlib.sha256(b"a stranger").digest()]]
        seeds = b"".join(per_key[3 if o is None else o][32 * i:32 * i + 32] for i, o in enumerate(owner))
        mk = lambda: [bp.Transcript(b"api scan %d" % (i % 2)) for i in range(nb)]
        proofs = [p for p, _ in bp.RangeProof.prove_batch(gens, pc, mk(), vals, bls, n, rng32=seeds, rewind=True, messages=msgs)]
        want = (bytes([OK, OK, OK, NOT_FOUND, OK]), owner, [v[0] if o is not None else 0 for v, o in zip(vals, owner)],
                [(m or bytes(16)) if o is not None else bytes(16) for m, o in zip(msgs, owner)], [b[0] if o is not None else bytes(32) for b, o in zip(bls, owner)])
        assert bp.RangeProof.scan_batch(gens, pc, mk(), proofs, coms, n, keys) == want
        assert bp.RangeProof.scan_batch(gens, pc, bp.TranscriptBatch.from_states(gens, mk()), proofs, coms, n, b"".join(keys)) == want
        for j in range(3):      # ... what rewind_batch gives key by key
            mine = bp.RangeProof.rewind_batch(gens, pc, mk(), proofs, coms, n, per_key[j])
            assert [m is not None for m in mine] == [o == j for o in owner]
        one = bp.Transcript(b"api scan shared")
        shared = [p for p, _ in bp.RangeProof.prove_batch(gens, pc, one, vals, bls, n, rng32=seeds, rewind=True)]
        got = bp.RangeProof.scan_batch(gens, pc, one, shared, coms, n, keys)
        assert got[:3] == want[:3] and got[3] == [bytes(16)] * nb
        assert bp.RangeProof.scan_batch(gens, pc, one, [], [], n, keys) == (b"", [], [], [], [])
        bad = proofs[1].to_bytes()
        bad = bad[:192] + tw.L.to_bytes(32, "little") + bad[224:]
        with pytest.raises(bp.FormatError):
            bp.RangeProof.scan_batch(gens, pc, mk(), [proofs[0], bad] + proofs[2:], coms, n, keys)
        with pytest.raises(bp.FormatError):
            bp.RangeProof.scan_batch(gens, pc, mk(), [p.to_bytes()[:-64] for p in proofs], coms, n, keys)
        for k in ([], [bytes(31)], b"\x01" * 33):
            with pytest.raises(ValueError):
                bp.RangeProof.scan_batch(gens, pc, mk(), proofs, coms, n, k)
    finally:
        gens.ctx.close()


def test_cpp_client_scans_under_several_keys(tmp_path):
    """include/bulletproofs.hpp: RangeProof::scan_batch"""
    exe, csrc = str(tmp_path / "range_proof_scan_test"), os.path.join(ROOT, "bulletproofs_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "range_proof_scan_test.cpp"),
                           "-L", csrc, "-lbpgpu", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout
