"""The seeded party steps of the multi-party aggregation protocol without a GPU: the step-1 and step-2 lane bodies of csrc/mpc_party.h
over seeds and first-draw indices (mpc_from_seed) against the same bodies over pre-expanded bytes (mpc_from_bytes), compiled for the
host in tests/mpc_seed_harness.  The bytes are the keystream of oracle/py/chacha_rng.py: block first_draw + d of the row's seed is
draw d.  The same harness runs once more as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import hashlib
import os
import random
import subprocess

import pytest

import chacha_rng as CR

HERE = os.path.dirname(os.path.abspath(__file__))
HARNESS = os.path.join(HERE, "mpc_seed_harness", "harness.cpp")
L = CR.L
FIRSTS = [0, 7, 2**32 - 3]   # the last: the 2n + 2 draws of one party straddle the carry into the counter's high word
OUTPUTS = ("state1", "rows_v", "rows_as", "state2", "rows_t", "status2")


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("msh") / "libmsh.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, HARNESS])
    lib = C.CDLL(so)
    u8p, u64p = C.c_char_p, C.POINTER(C.c_uint64)
    lib.msh_party.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), u64p, u8p, u8p, u64p, u8p, C.c_uint32, u8p, u64p] + [u8p] * 6
    return lib


def keystream(seed32, first, ndraws):
    return b"".join(CR.chacha20_block(seed32, first + d) for d in range(ndraws))


def _rows(n, nrows, tag, firsts):
    """nrows parties: positions over 0..3 in shuffled (non-sorted) order, distinct seeds, first draws cycling through `firsts`; poly commit
    either carried on (first + 2n + 2) or at a position of its own"""
    rnd = random.Random(tag)
    h = lambda what, r, k: hashlib.shake_256(b"%s-%s-%d" % (tag.encode(), what, r)).digest(k)
    rows = []
    for r in range(nrows):
        f1 = firsts[r % len(firsts)]
        f2 = f1 + 2 * n + 2 if r % 2 else firsts[(r // 2) % len(firsts)] + 2 * n
        rows.append(dict(pos=rnd.randrange(4), v=int.from_bytes(h(b"v", r, 8), "little"), bl=h(b"b", r, 32), seed=h(b"s", r, 32), f1=f1, f2=f2,
                         chal=h(b"y", r, 31) + b"\x00" + h(b"z", r, 31) + b"\x00"))
    return rows


def _run(H, n, rows, seeded, npos=4):
    nr, row = len(rows), 2 * n + 2
    w1, w2 = H.msh_state_words(n, 1), H.msh_state_words(n, 2)
    bufs = [C.create_string_buffer(k * nr) for k in (4 * w1, 64, 64 * row, 4 * w2, 128, 1)]
    cat = lambda k: b"".join(q[k] for q in rows)
    u64 = lambda k: (C.c_uint64 * nr)(*[q[k] for q in rows])
    if seeded:
        rng1, b1, rng2, b2 = cat("seed"), u64("f1"), None, u64("f2")
        assert len(rng1) == 32 * nr and C.sizeof(b1) == 8 * nr                     # exact sizes: 32 and 8 bytes per row
    else:
        rng1, b1, b2 = b"".join(keystream(q["seed"], q["f1"], row) for q in rows), None, None
        rng2 = b"".join(keystream(q["seed"], q["f2"], 2) for q in rows)
    ns = H.msh_party(1 if seeded else 0, n, nr, npos, (C.c_uint32 * nr)(*[q["pos"] for q in rows]), u64("v"), cat("bl"), rng1, b1, cat("chal"), 0, rng2, b2, *bufs)
    assert ns > 0 and ns % 64 == 0, ns                                            # (-2: a padding slot was written to)
    return ns, dict(zip(OUTPUTS, (b.raw for b in bufs)))


def _scalar(block64):
    return (int.from_bytes(block64, "little") % L).to_bytes(32, "little")


@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("n", [8, 64])
def test_seeded_bodies_equal_the_unseeded_bodies_on_the_keystream(H, n, first):
    """all state words and scalar rows, one first draw for every row; and state1 holds the scalars of the keystream blocks themselves"""
    rows = _rows(n, 5, "parity-%d-%d" % (n, first), [first])
    if first == 2**32 - 3:   # draws 0..2 have a high counter word of 0, the others of 1: a 32-bit counter would repeat blocks 0, 1, ...
        ks = keystream(rows[0]["seed"], first, 2 * n + 2)
        assert ks[64 * 3:64 * 4] == CR.chacha20_block(rows[0]["seed"], 2**32) != CR.chacha20_block(rows[0]["seed"], 0)
    _, want = _run(H, n, rows, False)
    _, got = _run(H, n, rows, True)
    for k in OUTPUTS:
        assert got[k] == want[k], k
    assert got["status2"] == bytes(len(rows))
    w1 = 4 * H.msh_state_words(n, 1)
    for r, q in enumerate(rows):
        st = got["state1"][w1 * r:w1 * (r + 1)]
        ks = keystream(q["seed"], first, 2 * n + 2)
        assert st[64:64 + 32 * (2 * n + 2)] == b"".join(_scalar(ks[64 * d:64 * d + 64]) for d in range(2 * n + 2)), r   # a_blinding, s_blinding, s_L, s_R
        w2 = 4 * H.msh_state_words(n, 2)
        t12 = keystream(q["seed"], q["f2"], 2)
        assert got["state2"][w2 * r + 32 * 5:w2 * r + 32 * 7] == _scalar(t12[:64]) + _scalar(t12[64:]), r                  # t_1_blinding, t_2_blinding


@pytest.mark.parametrize("n", [8, 64])
def test_padding_slots_and_rows_in_non_sorted_position_order(H, n):
    """70 rows over four positions: two or more wavefronts, every position's run padded, the row-to-slot map not the identity.  The expected
    bytes are computed ROW BY ROW (a call of one row has the identity map): what a row gets follows the caller's row, not its slot."""
    rows = _rows(n, 70, "shuffled-%d" % n, FIRSTS)
    pos = [q["pos"] for q in rows]
    assert pos != sorted(pos) and set(pos) == {0, 1, 2, 3}
    ns, got = _run(H, n, rows, True)
    assert ns >= 256 and ns > len(rows)                                           # four padded runs
    _, want = _run(H, n, rows, False)
    for k in OUTPUTS:
        assert got[k] == want[k], k
    sizes = {k: len(got[k]) // len(rows) for k in OUTPUTS}
    for r in (0, 1, 37, 69):
        _, alone = _run(H, n, [rows[r]], False)
        for k in OUTPUTS:
            assert got[k][sizes[k] * r:sizes[k] * (r + 1)] == alone[k], (k, r)


def test_a_rejected_row_draws_nothing_and_leaves_zeros(H):
    n = 8
    rows = _rows(n, 6, "reject", FIRSTS)
    rows[2]["chal"] = L.to_bytes(32, "little") + rows[2]["chal"][32:]            # y = l: not canonical
    _, want = _run(H, n, rows, False)
    _, got = _run(H, n, rows, True)
    for k in OUTPUTS:
        assert got[k] == want[k], k
    w2 = 4 * H.msh_state_words(n, 2)
    assert got["status2"] == bytes([0, 0, 3, 0, 0, 0]) and got["state2"][2 * w2:3 * w2] == bytes(w2) and got["rows_t"][256:384] == bytes(128)


def test_stand_alone_harness_under_the_sanitizers(tmp_path):
    """the same source with its own main, -fsanitize=address,undefined, every buffer at its exact size; a child process, nothing preloaded"""
    exe = str(tmp_path / "msh_sanitized")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DMSH_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-static-libubsan", "-o", exe, HARNESS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    print(r.stderr[:4000])
    assert r.returncode == 0 and "mpc seed harness ok" in r.stdout


# ---- the Python typestates ------------------------------------------------------------------------------------------------------
class _FakeCtx:
    def __init__(self):
        self.calls = []

    def mpc_party_bit_commit(self, n, idx, vals, bl, rng=None, rng_seed32=None, first_draw=None):
        self.calls.append(("bit", rng, rng_seed32, first_draw))
        return bytes(96), bytearray(b"\x11" * 64)

    def mpc_party_poly_commit(self, n, st, ch, rng=None, rng_seed32=None, first_draw=None):
        self.calls.append(("poly", rng, rng_seed32, first_draw))
        return bytes(64), bytearray(b"\x22" * 64), bytes(1)


class _FakeGens:
    gens_capacity, party_capacity = 64, 4

    def __init__(self):
        self.ctx = _FakeCtx()


def test_typestates_pass_seed_and_first_draw_on_and_refuse_both_sources():
    import bulletproofs_amd.range_proof_mpc as M
    gens, s = _FakeGens(), bytes(range(32))
    p1, _ = M.Party.new(gens, None, 5, bytes(32), 8).assign_position_with_rng(1, rng_seed32=s, first_draw=18)
    p1.apply_challenge_with_rng(M.BitChallenge(bytes(64)), rng_seed32=s)
    assert gens.ctx.calls == [("bit", None, s, [18]), ("poly", None, s, None)]
    p0 = M.Party.new(gens, None, 5, bytes(32), 8)
    with pytest.raises(ValueError):
        p0.assign_position_with_rng(0, bytes(64 * 18), rng_seed32=s)
    with pytest.raises(ValueError):
        p0.assign_position_with_rng(0, rng_seed32=s[:31])
    q1, _ = p0.assign_position_with_rng(0, rng_seed32=s)                          # the refused calls did not consume the state
    with pytest.raises(ValueError):
        q1.apply_challenge_with_rng(M.BitChallenge(bytes(64)), bytes(128), rng_seed32=s)
    q1.apply_challenge_with_rng(M.BitChallenge(bytes(64)), bytes(128))
    assert gens.ctx.calls[-1] == ("poly", bytes(128), None, None)
