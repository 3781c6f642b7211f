"""Rows of commitments shared by tests/test_pedersen_sum_on_cpu.py and tests/test_gpu_pedersen_sum.py, and the oracle's answer to a row.

Points are hashed valid encodings (point_corpus.valid_points), values and blindings come from pedersen_cases.  The row lengths are
chosen for workgroups of BLOCK = 64 terms and a finish lane that adds at most SERIAL_MAX = 128 partials (PSUM_BLOCK / PSUM_SERIAL_MAX of
csrc/pedersen_sum.h; the CPU test asserts that the header still says so)."""
import functools
import hashlib

import pedersen_cases as pc
import point_corpus as corpus

BLOCK, SERIAL_MAX = 64, 128
OK, BAD_POINT, BAD_SCALAR = 0, 1, 2                    # BPGPU_MSM_*
BALANCED, VERIFICATION_ERROR, FORMAT_ERROR = 0, 1, 2   # BPGPU_VERDICT_*
L = pc.L_ORDER

# rows that cross a workgroup boundary, rows of a workgroup's length, empty rows between full ones, a row across eleven workgroups
PATTERN = [0, 1, 2, 63, 1, 64, 0, 65, 255, 3, 256, 257, 700, 0]
# PATTERN's own offsets never put a row's first term in lane 63 nor a 64-term row on a workgroup's first lane (its offsets mod 64 are
# 0 .. 7), so these rows follow it, behind a 61-term row that ends the 27th workgroup: a row in (lane 63, lane 0 of the next), a row
# that is exactly one workgroup, another behind an empty row, a 127-term row that ends in lane 62, and (lane 63, lane 0) again
EDGES = [63, 2, 63, 64, 0, 64, 127, 2]
ROWS = PATTERN + [61] + EDGES
LONG_ROW = 2 * BLOCK * BLOCK + 1                        # 8 193 terms: 129 partials, one more than a finish lane may add -> a reduce pass
SIGN_MODES = ("zeros", "ones", "alternating", None)
POOL = 257                                              # distinct hashed points; term t of a batch is point (97 t) mod 257


def offsets(lengths):
    off = [0]
    for n in lengths:
        off.append(off[-1] + n)
    return off


def boundaries(lengths, block=BLOCK):
    """what the pattern is there for, as facts about it: (rows that span a workgroup boundary with their first term in the last lane
    of a workgroup or their last term in the first lane of one, rows that are exactly one workgroup, the most workgroups a row touches)"""
    off = offsets(lengths)
    edge = [r for r, n in enumerate(lengths) if n and off[r] // block != (off[r + 1] - 1) // block and (off[r] % block == block - 1 or (off[r + 1] - 1) % block == 0)]
    whole = [r for r, n in enumerate(lengths) if n == block and off[r] % block == 0]
    most = max(((off[r + 1] - 1) // block - off[r] // block + 1) for r, n in enumerate(lengths) if n)
    return edge, whole, most


@functools.lru_cache(maxsize=None)
def pool():
    return corpus.valid_points(POOL, b"pedersen-sum")


def points(total, shift=0):
    p = pool()
    return [p[(97 * (t + shift)) % POOL] for t in range(total)]


def signs(mode, total):
    """one byte per term, or None (every term added)"""
    if mode is None:
        return None
    if mode == "zeros":
        return bytes(total)
    if mode == "ones":
        return bytes([1]) * total
    if mode == "alternating":
        return bytes((t + t // 7) & 1 for t in range(total))
    raise ValueError(mode)


def scalars(nrows):
    """(values below 2^64, blindings) for nrows rows: the (value, blinding) matrix of pedersen_cases, cycled from its second row on"""
    rows = pc.rows()
    pick = [rows[1 + i % (len(rows) - 1)] for i in range(nrows)]
    return [v for v, _ in pick], [r for _, r in pick]


def pack(values, value_bytes):
    return b"".join(v.to_bytes(value_bytes, "little") for v in values)


ONE, MINUS_ONE = pc.le32(1), pc.le32(L - 1)


def expect_row(oracle, B, Bb, pts, sg, value=None, blinding=None):
    """oracle.msm over (+-1, C_i) ..., (value, B), (blinding, B_blinding) -> (status, 32 bytes); a row without any term is the identity"""
    sc = b"".join(MINUS_ONE if (sg and sg[i]) else ONE for i in range(len(pts)))
    pp = b"".join(pts)
    if value is not None:
        sc, pp = sc + pc.le32(value), pp + B
    if blinding is not None:
        sc, pp = sc + pc.le32(blinding), pp + Bb
    if not sc:
        return 0, bytes(32)
    return oracle.msm(sc, pp)


def expect_rows(oracle, B, Bb, off, pts, sg, values=None, blindings=None):
    out = []
    for r in range(len(off) - 1):
        st, e = expect_row(oracle, B, Bb, pts[off[r]:off[r + 1]], sg[off[r]:off[r + 1]] if sg else None,
                           None if values is None else values[r], None if blindings is None else blindings[r])
        assert st == 0
        out.append(e)
    return out


def msm_route(off, pts, sg, values, blindings, B, Bb):
    """the same rows as arguments of msm_batch: (n_terms, scalars, points) -- contract (a)"""
    n_terms, sc, pp = [], [], []
    for r in range(len(off) - 1):
        a, b = off[r], off[r + 1]
        sc += [MINUS_ONE if (sg and sg[t]) else ONE for t in range(a, b)] + [pc.le32(values[r]), pc.le32(blindings[r])]
        pp += pts[a:b] + [B, Bb]
        n_terms.append(b - a + 2)
    return n_terms, b"".join(sc), b"".join(pp)


def balanced_rows(oracle, B, Bb, lengths):
    """rows built as sums of commitments to (v_i, r_i): (offsets, points, values = sum v_i < 2^64, blindings = sum r_i mod l).
    The v_i are the matrix's values cut to 56 bits, so that a row of up to 256 of them stays a u64."""
    rows = pc.rows()
    off = offsets(lengths)
    pts, values, blindings = [], [], []
    memo = {}
    k = 1
    for n in lengths:
        assert n <= 256
        v_sum = r_sum = 0
        for _ in range(n):
            v, r = rows[k % len(rows)]
            v &= 2**56 - 1
            k += 1
            if (v, r) not in memo:
                memo[(v, r)] = pc.expect(oracle, B, Bb, v, r)
            pts.append(memo[(v, r)])
            v_sum, r_sum = v_sum + v, (r_sum + r) % L
        values.append(v_sum)
        blindings.append(r_sum)
    return off, pts, values, blindings


def reject_rows(nterms=5):
    """One row per member of point_corpus.REJECT_ENC, the member alone among nterms - 1 valid terms at a position that moves with its
    index, and a fully valid row in front of every member's row and behind the last: (lengths, points, flags), flags[r] = row r holds
    a member."""
    p = pool()
    lengths, pts, flags = [], [], []
    for i, e in enumerate(corpus.REJECT_ENC):
        lengths.append(nterms)
        pts += [p[(11 * i + j) % POOL] for j in range(nterms)]
        flags.append(False)
        row = [p[(13 * i + j + 3) % POOL] for j in range(nterms)]
        row[i % nterms] = e
        lengths.append(nterms)
        pts += row
        flags.append(True)
    lengths.append(nterms)
    pts += [p[j] for j in range(nterms)]
    flags.append(False)
    return lengths, pts, flags


def random_lengths(seed, nrows, longest):
    """seeded row lengths with a good share of empty and short rows"""
    h = hashlib.shake_256(b"psum-lengths-%d" % seed).digest(4 * nrows)
    out = []
    for i in range(nrows):
        x = int.from_bytes(h[4 * i:4 * i + 4], "little")
        kind = x & 7
        out.append(0 if kind == 0 else (1 + (x >> 3) % 4 if kind < 5 else (x >> 3) % (longest + 1)))
    return out
