"""Test twin of the R1CS witness check: the residual Prover::eval(lc_q) of every constraint of a recorded
bulletproofs_amd.r1cs.Prover in pure Python, from Prover.descriptor() and r1cs_prover_twin.eval_witness; the gadget cases whose
unsatisfied sets are known; the case file of tests/r1cs_check_harness.  TEST INFRASTRUCTURE ONLY."""
import os
import struct
import subprocess

import r1cs_prover_twin as P
import r1cs_twin as R

L = R.L
HARNESS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "r1cs_check_harness", "harness.cpp")
CHALLENGE = 0x1234567 * 2**200 + 99          # the one fixed challenge the table below was worked out with


def residuals(rec, challenges):
    """[Prover::eval(lc_q) mod l] over the constraints of a recorded Prover, for the given phase-2 challenge values"""
    from bulletproofs_amd import r1cs
    aL, aR, aO = P.eval_witness(rec, challenges)
    out = []
    for terms in rec.descriptor()[5]:
        acc = 0
        for (kind, idx), ch, pw, k in terms:
            val = {r1cs.KIND_L: aL, r1cs.KIND_R: aR, r1cs.KIND_O: aO, r1cs.KIND_V: rec.v}.get(kind)
            x = 1 if kind == r1cs.KIND_ONE else val[idx]
            acc += k * (pow(challenges[ch], pw, L) if ch is not None else 1) * x
        out.append(acc % L)
    return out


def unsatisfied(rec, challenges):
    return [q for q, r in enumerate(residuals(rec, challenges)) if r]


def report(rec, challenges):
    """(first or None, count, map bytes) as the library reports them"""
    bad = unsatisfied(rec, challenges)
    Q = len(rec.descriptor()[5])
    mp = bytearray((Q + 7) // 8)
    for q in bad:
        mp[q // 8] |= 1 << (q % 8)
    return (bad[0] if bad else None), len(bad), bytes(mp)


# ---- the gadget cases: (name, values, gadget(cs, vars), Q, n_challenges, unsatisfied) -------------------------------------
def _shuffle(k):
    return lambda cs, v: R.shuffle_gadget(cs, v[:k], v[k:])


def _example(cs, v):
    R.example_gadget(cs, v[0], v[1], v[2], v[3], v[4], 9)


def _range8(bits_of):
    return lambda cs, v: R.range_gadget(cs, v[0], bits_of, 8)


CASES = [
    ("shuffle3_perm", [1, 2, 3, 3, 1, 2], _shuffle(3), 9, 1, []),
    ("shuffle3_bad", [1, 2, 3, 3, 1, 4], _shuffle(3), 9, 1, [8]),
    ("shuffle1_bad", [1, 2], _shuffle(1), 1, 0, [0]),
    ("example_ok", [3, 4, 6, 1, 40], _example, 3, 0, []),
    ("example_bad", [3, 4, 6, 1, 41], _example, 3, 0, [2]),
    ("range8_ok", [0xa5], _range8(0xa5), 17, 0, []),
    ("range8_bad", [0x1a5], _range8(0xa5), 17, 0, [16]),
]


def record(case, locate=False, st0=bytes(208)):
    from bulletproofs_amd import r1cs
    _, vals, gadget, _, _, _ = case
    cs = r1cs.Prover(st0, locate=locate) if locate else r1cs.Prover(st0)
    xs = [cs.commit(v, 1000 + j) for j, v in enumerate(vals)]
    gadget(cs, xs)
    cs._finish()
    return cs


def long_row_prover(lengths, broken=None, st0=bytes(208)):
    """One constraint per length, every prover of the same lengths the same gadget: the row's last term is a committed variable W_r of
    its own (w_r = 0), before it cancelling pairs c V_0 - c V_1 (v_0 == v_1) and, for an even length, one ONE term of coefficient
    zero.  broken: that row's w_r is off by one, so the row -- and no other -- fails.  A row of length 0 has no term."""
    from bulletproofs_amd import r1cs
    cs = r1cs.Prover(st0)
    x0, x1 = cs.commit(77, 7), cs.commit(77, 8)
    ws = [cs.commit(1 if r == broken else 0, 9 + r) for r in range(len(lengths))]
    for r, ln in enumerate(lengths):
        lc = r1cs.LinearCombination()
        if ln:
            for t in range((ln - 1) // 2):
                lc = lc + x0 * (t + 1) - x1 * (t + 1)
            if (ln - 1) % 2:
                lc = lc + r1cs.ONE() * 0
            lc = lc + ws[r]
        assert len(lc.terms) == ln
        cs.constrain(lc)
    return cs


# ---- the harness ----------------------------------------------------------------------------------------------------------------
def _u32s(xs):
    return struct.pack("<%dI" % len(xs), *xs)


def _pad(b):
    return b + bytes(-len(b) % 4)


def _terms(rows):
    from bulletproofs_amd import r1cs
    row, kind, index, chal, power, coeff = [0], [], [], [], [], []
    for terms in rows:
        for (k_, i_), ch, pw, cf in terms:
            kind.append(k_)
            index.append(i_)
            chal.append(r1cs.NO_CHALLENGE if ch is None else ch)
            power.append(0 if ch is None else pw)
            coeff.append((cf % L).to_bytes(32, "little"))
        row.append(len(kind))
    return row, _pad(bytes(kind)) + _u32s(index) + _u32s(chal) + _u32s(power) + b"".join(coeff), len(kind)


def case_file(provers, challenges, want_map=True):
    """the harness's input: the constraints as Circuit() hands them to bpgpu_r1cs_circuit_create, the witness program as Witness()
    hands it to bpgpu_r1cs_witness_create, then the batch; challenges: nbatch lists of ints"""
    rec = provers[0]
    m, n1, n2, _, labels, cons = rec.descriptor()
    crow, cterms, nct = _terms(cons)
    wrow, wterms, nwt = _terms(rec.rows)
    ins = [p.inputs() for p in provers]
    hdr = [m, n1, n2, len(labels), len(cons), nct, len(rec.free), len(rec.rows), nwt, len(provers), 1 if want_map else 0]
    return (b"R1C1" + _u32s(hdr) + _u32s(crow) + cterms + _u32s(rec.src_left) + _u32s(rec.src_right) + _u32s(wrow) + wterms +
            b"".join(i[0] for i in ins) + b"".join(i[2] for i in ins) + b"".join((c % L).to_bytes(32, "little") for row in challenges for c in row))


def parse_output(raw, nbatch):
    """{chunk, mapw, units, longs, slots, slice, status, first, count, maps (bytes per proof)}"""
    chunk, mapw, units, longs, slots, per = struct.unpack_from("<6I", raw, 0)
    off = 24
    out = {"chunk": chunk, "mapw": mapw, "units": units, "longs": longs, "slots": slots, "slice": per}
    for key in ("status", "first", "count"):
        out[key] = list(struct.unpack_from("<%dI" % nbatch, raw, off))
        off += 4 * nbatch
    out["maps"] = [raw[off + 4 * mapw * b:off + 4 * mapw * (b + 1)] for b in range(nbatch)]
    assert off + 4 * mapw * nbatch == len(raw)
    return out


def build_harness(dirname, sanitized=False):
    """the harness as a shared library (path), or as a stand-alone sanitized executable (path; None without a sanitizer runtime)"""
    if not sanitized:
        so = os.path.join(str(dirname), "libr1ch.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, HARNESS])
        return so
    exe = os.path.join(str(dirname), "harness")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DR1CH_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, HARNESS],
                       capture_output=True, text=True)
    return exe if r.returncode == 0 else None
