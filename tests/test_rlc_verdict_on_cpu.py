"""The verdict rule of the combined checks without a GPU: rlc_comb.h's rlc_verdict_thread (the one verdict body of the R1CS, linear and
mixed range-proof checks) and r1cs_rlc.h's r1_rlc_sum_thread in front of it, compiled for the host (tests/r1cs_rlc_harness) and driven
lane by lane.  The rule: a proof's front-end code wins; a proof marked as decided already is left alone; else OK when R decoded and is the
identity; else undecided; the 33 batch bytes are 0 / 1 and compress(R), or zeros where R did not decode."""
import ctypes as C
import os
import subprocess

import pytest

import bp_twin as T

HERE = os.path.dirname(os.path.abspath(__file__))
OK, UNDECIDED, DONE = 0, 5, 0xffffffff
UNTOUCHED = 0xaa
N = 130                                            # lanes 0, 63, 64, 65 and a third wavefront's
IDENTITY = bytes(32)


def _pt(k):
    return T.pt_mul(k, T.BASEPOINT)


ENC = {k: T.compress(_pt(k)) for k in (1, 2, 3, 5)}
ENC_NEG3 = T.compress(T.pt_neg(_pt(3)))
NOT_A_POINT = b"\xff" * 32                         # non-canonical and negative: no decoder takes it


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rlcverdict") / "libr1rlc.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "r1cs_rlc_harness", "harness.cpp")])
    return C.CDLL(so)


def _words(b):
    return (C.c_uint32 * (len(b) // 4))(*[int.from_bytes(b[4 * i:4 * i + 4], "little") for i in range(len(b) // 4)])


def _verdicts(harness, gstatus, enc, status_byte):
    """every lane of the verdict launch -> (the verdict bytes, prefilled with UNTOUCHED; the 33 batch bytes)"""
    n = len(gstatus)
    verdict = (C.c_uint8 * n)(*([UNTOUCHED] * n))
    batch = (C.c_uint8 * 33)(*([UNTOUCHED] * 33))
    harness.rlc_comb_verdict_lanes(n, (C.c_uint32 * n)(*gstatus), _words(enc), (C.c_uint8 * 1)(status_byte), verdict, batch)
    return list(verdict), bytes(batch)


def _sum(harness, parts, part_status):
    """the sum launch's one lane -> (compress(R), its status byte)"""
    res = (C.c_uint32 * 8)(*([0xdeadbeef] * 8))
    rst = (C.c_uint8 * 1)(UNTOUCHED)
    harness.r1cs_rlc_sum_lane(len(parts), _words(b"".join(parts)), (C.c_uint8 * len(parts))(*part_status), res, rst)
    return b"".join(int(w).to_bytes(4, "little") for w in res), rst[0]


def _gstatus():
    """front-end codes at lanes 0, 63, 64 and 129, a group decided already at 1, 65 and 128, the rest for the combination to decide"""
    g = [0] * N
    g[0], g[63], g[64], g[129] = 2, 1, 4, 3
    g[1] = g[65] = g[128] = DONE
    return g


def _expect(gstatus, undecided_or_ok):
    return [UNTOUCHED if st == DONE else (st if st else undecided_or_ok) for st in gstatus]


def test_identity_and_decoded_is_ok_codes_kept_sentinel_untouched(harness):
    g = _gstatus()
    verdict, batch = _verdicts(harness, g, IDENTITY, 0)
    assert verdict == _expect(g, OK)
    assert batch == bytes(33)


def test_lane_0_writes_the_batch_bytes_whatever_its_own_status(harness):
    for st0 in (0, 2, DONE):
        verdict, batch = _verdicts(harness, [st0, 0], ENC[5], 0)
        assert verdict == [UNTOUCHED if st0 == DONE else (st0 or UNDECIDED), UNDECIDED]
        assert batch == b"\x01" + ENC[5]


def test_nonzero_r_is_undecided_with_its_encoding(harness):
    g = _gstatus()
    verdict, batch = _verdicts(harness, g, ENC[2], 0)
    assert verdict == _expect(g, UNDECIDED)
    assert batch[0] == 1 and batch[1:] == ENC[2]
    # one non-zero word anywhere is enough
    for w in range(8):
        enc = bytes(4 * w) + b"\x00\x00\x00\x80" + bytes(28 - 4 * w)
        verdict, batch = _verdicts(harness, [0], enc, 0)
        assert verdict == [UNDECIDED] and batch == b"\x01" + enc


@pytest.mark.parametrize("enc", [IDENTITY, ENC[1]], ids=["zero-words", "some-words"])
@pytest.mark.parametrize("status_byte", [1, 0x80])
def test_undecoded_msm_is_undecided_with_zero_bytes(harness, enc, status_byte):
    """a multiscalar multiplication that dropped a point it could not decode may well leave the identity: never OK"""
    g = _gstatus()
    verdict, batch = _verdicts(harness, g, enc, status_byte)
    assert verdict == _expect(g, UNDECIDED)
    assert batch == b"\x01" + bytes(32)


def test_sum_of_one_combination_is_its_msm_as_it_is(harness):
    assert _sum(harness, [IDENTITY], [0]) == (IDENTITY, 0)
    assert _sum(harness, [ENC[3]], [0]) == (ENC[3], 0)
    assert _sum(harness, [NOT_A_POINT], [0]) == (NOT_A_POINT, 0)           # (no decompression: the MSM's own output)
    for st in (1, 0x80):
        enc, rst = _sum(harness, [IDENTITY], [st])
        assert enc == IDENTITY and rst != 0
        assert _verdicts(harness, [0, 2], enc, rst) == ([UNDECIDED, 2], b"\x01" + bytes(32))


def test_sum_of_three_combinations(harness):
    # 1 + 2 - 3 = 0: every proof of the call passes
    enc, rst = _sum(harness, [ENC[1], ENC[2], ENC_NEG3], [0, 0, 0])
    assert (enc, rst) == (IDENTITY, 0)
    assert _verdicts(harness, [0, 4, 0], enc, rst) == ([OK, 4, OK], bytes(33))
    # 1 + 2 + 2 = 5
    enc, rst = _sum(harness, [ENC[1], ENC[2], ENC[2]], [0, 0, 0])
    assert (enc, rst) == (ENC[5], 0)
    assert _verdicts(harness, [0, 4, 0], enc, rst) == ([UNDECIDED, 4, UNDECIDED], b"\x01" + ENC[5])


@pytest.mark.parametrize("where", [0, 1, 2])
@pytest.mark.parametrize("how", ["status", "encoding"])
def test_sum_with_one_undecoded_part_is_undecided_even_where_the_rest_cancels(harness, where, how):
    """the part is left out of the sum -- what remains is the identity here -- and the call stays undecided, its 32 bytes zero"""
    parts, status = [ENC[3], ENC_NEG3], [0, 0]
    parts.insert(where, ENC[2] if how == "status" else NOT_A_POINT)
    status.insert(where, 1 if how == "status" else 0)
    enc, rst = _sum(harness, parts, status)
    assert enc == IDENTITY and rst != 0
    assert _verdicts(harness, [0, 1, DONE], enc, rst) == ([UNDECIDED, 1, UNTOUCHED], b"\x01" + bytes(32))
