"""Values and blindings shared by tests/test_pedersen_on_cpu.py and tests/test_gpu_pedersen.py, and the oracle's answer to a row."""
import hashlib

L_ORDER = 2**252 + 27742317777372353535851937790883648493
OK, BAD_SCALAR = 0, 2                                  # BPGPU_MSM_OK / BPGPU_MSM_BAD_SCALAR
OPENS, VERIFICATION_ERROR, FORMAT_ERROR = 0, 1, 2      # BPGPU_VERDICT_*
WINDOWS = (4, 5, 7, 8, 11, 13, 16, 20)                 # window sizes whose boundaries the u64 values straddle (20: gens_create(8, 1)'s own choice)


def u64_values(windows=WINDOWS):
    """the fixed patterns, then 2^(W k) - 1 and 2^(W k) for every k with W k <= 64 (2^64 itself is a scalar value only)"""
    vals = [0, 1, 2**63, 2**64 - 1, 0x8080808080808080, 0x7f7f7f7f7f7f7f7f, 0x0100000000000000]
    for W in windows:
        for k in range(1, 64 // W + 1):
            for v in (2**(W * k) - 1, 2**(W * k)):
                if v < 2**64 and v not in vals:
                    vals.append(v)
    return vals


SCALAR_ONLY_VALUES = [2**64, 2**252, L_ORDER - 1]
REJECTED_SCALARS = [L_ORDER, 2**256 - 1]


def random_scalars(tag, count):
    return [int.from_bytes(hashlib.shake_256(b"pedersen-%s-%d" % (tag, i)).digest(64), "little") % L_ORDER for i in range(count)]


def blindings():
    return [0, 1, L_ORDER - 1] + random_scalars(b"blinding", 5)


def rows(windows=WINDOWS):
    """(value, blinding) pairs, all canonical: every value against a cycling blinding, every blinding against the fixed patterns;
    (0, 0) first.  Values below 2^64 only."""
    vals, bls = u64_values(windows), blindings()
    out = [(v, bls[i % len(bls)]) for i, v in enumerate(vals)]
    out += [(v, b) for b in bls for v in vals[:7] if (v, b) not in out]
    assert out[0] == (0, 0)
    return out


def le32(x):
    return x.to_bytes(32, "little")


def expect(oracle, B, Bb, value, blinding):
    """oracle.msm([v, r], [B, B_blinding]) -> 32 bytes"""
    st, out = oracle.msm(le32(value) + le32(blinding), B + Bb)
    assert st == 0
    return out


def flip_bit(b, bit):
    x = bytearray(b)
    x[bit // 8] ^= 1 << (bit % 8)
    return bytes(x)
