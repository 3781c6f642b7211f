#!/usr/bin/env python3
"""Rates of the multi-party aggregation entry points (bpgpu_mpc_*) on one context, host pointers:
  parties/s  for steps 1-3 (bit commit, poly commit, proof share), each step and the three together
  sessions/s for steps 4-6 (bit challenge, poly challenge, assemble with the dealer's verification)
at (n, m) = (64, 1), (64, 16), (32, 4), beside bpgpu_rangeproof_prove_batch on the same shape and count, and
  position  : the bit commitments of P parties all at position 0 against all at position 3 of a (64, 4) table set, interleaved --
              the same 2n + 2 terms and table sizes, so the two should agree within the run-to-run spread
The parties draw their randomness from the OS CSPRNG; every session's proof is verified by the dealer step itself (status 0).
  --seeded  : the two party steps that draw, both ways on the same rows, interleaved -- unseeded with the caller's pre-expanded bytes
              (64 (2n + 2) and 128 per party) and with rng = NULL (the host expands them), seeded with 32 + 8 bytes per party and with
              rng32 = NULL -- at n = 64 and n = 8; the seeded outputs are checked against the unseeded ones on the same keystream first
    python tools/mpc_rate.py [--iters N] [--only position|rates] [--seeded]"""
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

import bulletproofs_amd as bp  # noqa: E402

LABEL = b"mpc rate"


def timed(f):
    t = time.perf_counter()
    r = f()
    return time.perf_counter() - t, r


def one_shape(n, m, ns, iters):
    ctx = bp.Context(0)
    ctx.gens_create(n, m)
    npar = ns * m
    vals = [int.from_bytes(hashlib.shake_256(b"v%d" % i).digest(8), "little") % (1 << n) for i in range(npar)]
    bl = b"".join(hashlib.shake_256(b"b%d" % i).digest(31) + b"\x00" for i in range(npar))
    idx = [r % m for r in range(npar)]
    rep = lambda a, w: b"".join(a[w * p:w * p + w] * m for p in range(ns))
    t = {k: [] for k in ("bit_commit", "poly_commit", "proof_share", "bit_challenge", "poly_challenge", "assemble", "prove_batch")}
    for it in range(iters + 1):
        d1, (bc, st1) = timed(lambda: ctx.mpc_party_bit_commit(n, idx, vals, bl))
        d4, (ch, _, ts, s4) = timed(lambda: ctx.mpc_dealer_bit_challenge(n, m, bc, LABEL))
        d2, (pc, st2, s2) = timed(lambda: ctx.mpc_party_poly_commit(n, st1, rep(ch, 64)))
        d5, (x, _, ts, s5) = timed(lambda: ctx.mpc_dealer_poly_challenge(m, pc, ts))
        d3, (sh, s3) = timed(lambda: ctx.mpc_party_proof_share(n, st2, rep(x, 32)))
        chal = b"".join(ch[64 * p:64 * p + 64] + x[32 * p:32 * p + 32] for p in range(ns))
        d6, (proofs, bad, s6, _) = timed(lambda: ctx.mpc_dealer_assemble(n, m, sh, bc, pc, chal, ts, LABEL))
        assert s2 == s3 == bytes(npar) and s4 == s5 == s6 == bytes(ns) and bad == bytes(npar)   # s6 = 0: the dealer verified every proof
        d7, _ = timed(lambda: ctx.rangeproof_prove_batch(n, m, vals, bl, label=LABEL))
        if it:
            for k, d in zip(t, (d1, d2, d3, d4, d5, d6, d7)):
                t[k].append(d)
    med = {k: statistics.median(v) for k, v in t.items()}
    party, dealer = med["bit_commit"] + med["poly_commit"] + med["proof_share"], med["bit_challenge"] + med["poly_challenge"] + med["assemble"]
    out = {"n": n, "m": m, "sessions": ns, "parties": npar, "iters": iters, "parties_per_s": round(npar / party), "sessions_per_s": round(ns / dealer),
           "prove_batch_proofs_per_s": round(ns / med["prove_batch"])}
    out.update({k + "_ms": round(v * 1e3, 2) for k, v in med.items()})
    print(json.dumps(out), flush=True)
    ctx.close()


def position(iters, npar=1024):
    n = 64
    ctx = bp.Context(0)
    ctx.gens_create(64, 4)
    vals = [int.from_bytes(hashlib.shake_256(b"v%d" % i).digest(8), "little") for i in range(npar)]
    bl = bytes(32 * npar)
    t = {0: [], 3: []}
    for it in range(iters + 1):
        for j in (0, 3):
            d, _ = timed(lambda: ctx.mpc_party_bit_commit(n, [j] * npar, vals, bl))
            if it:
                t[j].append(d)
    med = {j: statistics.median(v) for j, v in t.items()}
    spread = {j: (max(v) - min(v)) / med[j] for j, v in t.items()}
    print(json.dumps({"position": True, "n": n, "table_set": [64, 4], "parties": npar, "iters": iters, "position0_ms": round(med[0] * 1e3, 3),
                      "position3_ms": round(med[3] * 1e3, 3), "position3_over_position0": round(med[3] / med[0], 4),
                      "spread_position0": round(spread[0], 4), "spread_position3": round(spread[3], 4)}), flush=True)
    ctx.close()


def seeded(n, npar, iters):
    sys.path.insert(0, os.path.join(ROOT, "oracle", "py"))
    from chacha_rng import chacha20_block
    ctx = bp.Context(0)
    ctx.gens_create(64, 4)
    vals = [int.from_bytes(hashlib.shake_256(b"v%d" % i).digest(8), "little") % (1 << n) for i in range(npar)]
    bl = b"".join(hashlib.shake_256(b"b%d" % i).digest(31) + b"\x00" for i in range(npar))
    idx = [(r * 7 + r // 5) % 4 for r in range(npar)]
    seeds = hashlib.shake_256(b"seeds%d" % n).digest(32 * npar)
    chal = b"".join(hashlib.shake_256(b"c%d/%d" % (i, q)).digest(31) + b"\x00" for i in range(npar) for q in range(2))
    nd = 2 * n + 2
    # parity on the head of the batch (the keystream in Python is slow), then the timing on bytes of the same size
    k = 8
    ks1 = b"".join(chacha20_block(seeds[32 * r:32 * r + 32], d) for r in range(k) for d in range(nd))
    ks2 = b"".join(chacha20_block(seeds[32 * r:32 * r + 32], nd + d) for r in range(k) for d in range(2))
    bc_u, st_u = ctx.mpc_party_bit_commit(n, idx[:k], vals[:k], bl[:32 * k], ks1)
    bc_s, st_s = ctx.mpc_party_bit_commit(n, idx[:k], vals[:k], bl[:32 * k], rng_seed32=seeds[:32 * k])
    pc_u, st2_u, _ = ctx.mpc_party_poly_commit(n, st_u, chal[:64 * k], ks2)
    pc_s, st2_s, _ = ctx.mpc_party_poly_commit(n, st_s, chal[:64 * k], rng_seed32=seeds[:32 * k])
    assert (bc_u, st_u, pc_u, st2_u) == (bc_s, st_s, pc_s, st2_s), "seeded and unseeded outputs differ"
    rng1, rng2 = hashlib.shake_256(b"r1").digest(64 * nd * npar), hashlib.shake_256(b"r2").digest(128 * npar)
    _, st1 = ctx.mpc_party_bit_commit(n, idx, vals, bl, rng1)
    forms = {"bit_unseeded_bytes": lambda: ctx.mpc_party_bit_commit(n, idx, vals, bl, rng1),
             "bit_unseeded_null": lambda: ctx.mpc_party_bit_commit(n, idx, vals, bl),
             "bit_seeded": lambda: ctx.mpc_party_bit_commit(n, idx, vals, bl, rng_seed32=seeds),
             "bit_seeded_null": lambda: ctx.mpc_party_bit_commit(n, idx, vals, bl, first_draw=[0] * npar),
             "poly_unseeded_bytes": lambda: ctx.mpc_party_poly_commit(n, st1, chal, rng2),
             "poly_unseeded_null": lambda: ctx.mpc_party_poly_commit(n, st1, chal),
             "poly_seeded": lambda: ctx.mpc_party_poly_commit(n, st1, chal, rng_seed32=seeds),
             "poly_seeded_null": lambda: ctx.mpc_party_poly_commit(n, st1, chal, first_draw=[nd] * npar)}
    t = {k_: [] for k_ in forms}
    for it in range(iters + 2):
        for k_, f in forms.items():          # interleaved: drift hits every form alike
            d, _ = timed(f)
            if it >= 2:
                t[k_].append(d)
    med = {k_: statistics.median(v) for k_, v in t.items()}
    out = {"seeded": True, "n": n, "table_set": [64, 4], "parties": npar, "iters": iters, "rng_bytes_per_party_unseeded": [64 * nd, 128],
           "rng_bytes_per_party_seeded": [40, 40]}
    out.update({k_ + "_ms": round(v * 1e3, 3) for k_, v in med.items()})
    out.update({k_ + "_spread": round((max(v) - min(v)) / med[k_], 4) for k_, v in t.items()})
    for step in ("bit", "poly"):
        out[step + "_seeded_over_unseeded_bytes"] = round(med[step + "_seeded"] / med[step + "_unseeded_bytes"], 4)
        out[step + "_seeded_null_over_unseeded_null"] = round(med[step + "_seeded_null"] / med[step + "_unseeded_null"], 4)
    print(json.dumps(out), flush=True)
    ctx.close()


def main():
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 5
    if "--seeded" in sys.argv:
        for n, npar in ((64, 1024), (8, 1024)):
            seeded(n, npar, max(iters, 9))
        return
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    if only in (None, "position"):
        position(max(iters, 7))
    if only in (None, "rates"):
        for n, m, ns in ((64, 1, 1024), (64, 16, 64), (32, 4, 256)):
            one_shape(n, m, ns, iters)


if __name__ == "__main__":
    main()
