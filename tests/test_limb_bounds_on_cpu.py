"""The three limb arithmetics at the corners of their documented contracts, on the host build of the device headers
(tests/cpu_harness, with BP_FE_CHECK): fe25519.h's field limbs, horner_wave.h's one-limb-per-lane wavefront arithmetic
(lockstep emulation of wavevec.h) and sc25519.h's Montgomery limbs, plus the point formulas that feed them.  Inputs are
raw limb vectors -- every limb at its maximum, alternating maxima, single maxima, carry runs (all 0xffff, p .. p + 18,
2^255 - 1, 2^256 - 1), 2^k +- 1 and seeded random vectors inside the bounds -- not canonical encodings, so the lazy ranges are
reached.  Each result is compared with Python big ints mod p or mod l, and each output with the bound its source states
(limb_corpus.py holds the corpora and the references; test_gpu_limb_bounds.py runs the same calls on the device)."""
import hashlib

import pytest

import bp_twin as T
import harness_lib
import limb_corpus as LC
import point_corpus as PC


@pytest.fixture(scope="module")
def B():
    return LC.Backend(harness_lib.lib(), "h_")


def test_field_primitives_at_limb_bounds(B):
    LC.check_fe(B)


def test_hw_limbs_to_fe_on_its_whole_domain(B):
    """16 limbs <= 2^17: 2^257 - 1 carries out of limb 15 twice (the fold of 38 must run twice) and is 75 mod p."""
    out, ok = B.limbs_to_fe([[0xffff] * 15 + [0x1ffff]])
    assert LC.fev(out[0]) % LC.P == 75 and ok[0]
    LC.check_limbs_to_fe(B)


def test_scalar_montgomery_primitives_at_limb_bounds(B):
    LC.check_sc(B)


def test_point_formulas_at_limb_bounds(B):
    LC.check_ge(B)


def test_wavefront_field_arithmetic_at_limb_bounds(B):
    LC.check_hw(B)


def decode_encodings():
    """The encodings of test_group_ops_and_ristretto_codec: 24 points, the five fixed edge strings, 200 random byte strings;
    then point_corpus.py's members: every rejection class alone, the valid ends of the range, p + k, the roots of -1."""
    pts = [T.from_uniform_bytes(hashlib.shake_256(b"p%d" % i).digest(64)) for i in range(24)]
    enc = [T.compress(p) for p in pts]
    P = T.P
    enc += [bytes([1]) + bytes(31), P.to_bytes(32, "little"), (P + 2).to_bytes(32, "little"), b"\xff" * 32, (2).to_bytes(32, "little")]
    for i in range(200):
        e = hashlib.shake_256(b"e%d" % i).digest(32)
        enc.append(bytes([e[0] & 0xfe]) + e[1:31] + bytes([e[31] & 0x7f]))
    return enc + PC.ALL_ENC


def test_wavefront_drivers_host_copies(B):
    LC.check_drivers(B, decode_encodings())
