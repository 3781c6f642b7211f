#!/usr/bin/env python3
"""The batch-combined check over range proofs of MIXED shapes (bpgpu_rangeproof_verify_rlc_mixed) against the same proofs sent as one
bpgpu_rangeproof_verify_rlc call per shape, on:
  block       : 1 024 proofs at n = 64 with m drawn from {1, 2, 4, 8, 16}, weighted 8 : 4 : 2 : 1 : 1 (a block of confidential
                transactions: aggregated proofs of different output counts side by side)
  one_shape   : 4 096 proofs of (64, 1) alone through both entry points -- on one shape the mixed path should cost what the one-shape
                path costs
Proofs are made on the GPU (bpgpu_rangeproof_prove_batch).  The two forms run interleaved, blocking calls, the same rng64 / weights64
bytes each time; every verdict is checked.  One JSON line per workload: median and spread (min .. max) per form.
--transcripts shared | per-proof: the same workloads on the CALLERS' OWN transcripts instead -- three forms interleaved in one run:
  mixed_label : bpgpu_rangeproof_verify_rlc_mixed on proofs made from the label (the form above)
  mixed_ts    : bpgpu_rangeproof_verify_rlc_mixed_ts on proofs made on pre-bound states -- one state per group (shared), or one per proof
                with 32 different histories per group at differing STROBE positions (per-proof: the byte-wise replay)
  batch_ts    : bpgpu_rangeproof_verify_batch_ts group by group on the inputs of mixed_ts (the per-proof path)
    python tools/rlc_mixed_rate.py [--iters N] [--only block|one_shape] [--path both|per_shape|mixed] [--transcripts label|shared|per-proof]"""
import hashlib
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bulletproofs_amd as bp  # noqa: E402

LABEL = b"rlc-mixed-rate"


def make(ctx, n, m, count):
    """count (n, m) proofs made on the GPU: the group (n, m, proofs, proof_len, commitments, label)"""
    rnd = random.Random(n * 1000 + m)
    proofs, coms = b"", b""
    for s0 in range(0, count, 256):
        nb = min(256, count - s0)
        vals = [rnd.getrandbits(n) for _ in range(nb * m)]
        bl = b"".join(hashlib.shake_256(b"rate-bl-%d-%d-%d" % (n, m, s0 * m + i)).digest(31) + b"\x00" for i in range(nb * m))
        pr, cm = ctx.rangeproof_prove_batch(n, m, vals, bl, label=LABEL)
        proofs += pr
        coms += cm
    return (n, m, proofs, len(proofs) // count, coms, LABEL)


def bound_state(i):
    """a transcript the application has bound already: protocol label, session id, an earlier challenge, then a message whose length
    moves the STROBE position with i"""
    t = bp.Transcript(b"payment-protocol v3")
    t.append_message(b"session", hashlib.shake_256(b"rate-sess%d" % i).digest(40))
    t.challenge_bytes(b"binding", 16)
    t.append_message(b"amount-commitment-context", hashlib.shake_256(b"rate-ctx%d" % i).digest((13 * i + 5) % 166))
    return t.state


def make_ts(ctx, n, m, count, per_proof):
    """count (n, m) proofs made on the GPU on pre-bound states: the group (n, m, proofs, proof_len, commitments, states).  per_proof: proof
    i starts from history i % 32 of the group (proofs of one history are proved together, then dealt back to their places)"""
    rnd = random.Random(n * 1000 + m + 7)
    nst = min(32, count) if per_proof else 1
    states = [bound_state(1000 * m + j) for j in range(nst)]
    pl = 32 * (9 + 2 * ((n * m).bit_length() - 1))
    proofs, coms = [None] * count, [None] * count
    for j in range(nst):
        idx = list(range(j, count, nst))
        for s0 in range(0, len(idx), 256):
            part = idx[s0:s0 + 256]
            vals = [rnd.getrandbits(n) for _ in range(len(part) * m)]
            bl = b"".join(hashlib.shake_256(b"rate-tb-%d-%d-%d-%d" % (n, m, j, s0 * m + i)).digest(31) + b"\x00" for i in range(len(part) * m))
            pr, cm = ctx.rangeproof_prove_batch(n, m, vals, bl, transcript=states[j])
            for q, i in enumerate(part):
                proofs[i], coms[i] = pr[pl * q:pl * (q + 1)], cm[32 * m * q:32 * m * (q + 1)]
    return (n, m, b"".join(proofs), pl, b"".join(coms), b"".join(states[i % nst] for i in range(count)) if per_proof else states[0])


def run_ts(ctx, name, groups, groups_ts, iters, mode):
    """the three forms of --transcripts shared | per-proof, interleaved"""
    counts = [len(g[2]) // g[3] for g in groups]
    total = sum(counts)
    rng = hashlib.shake_256(b"rate-rng-" + name.encode()).digest(64 * total)
    w = hashlib.shake_256(b"rate-w-" + name.encode()).digest(64 * total)

    def mixed_label():
        v, ok, _ = ctx.rangeproof_verify_rlc_mixed(groups, rng, w)
        assert ok
        return v

    def mixed_ts():
        v, ok, _ = ctx.rangeproof_verify_rlc_mixed_ts(groups_ts, rng, w)
        assert ok
        return v

    def batch_ts():
        v, off = b"", 0
        for (n, m, proofs, plen, coms, states), nb in zip(groups_ts, counts):
            v += ctx.rangeproof_verify_batch_ts(n, m, proofs, plen, coms, states, rng[64 * off:64 * (off + nb)])
            off += nb
        return v

    forms = [("mixed_label", mixed_label), ("mixed_ts", mixed_ts), ("batch_ts", batch_ts)]
    ts = {k: [] for k, _ in forms}
    for k, fn in forms:                      # warm-up: tables, scripts, buffers
        assert fn() == bytes(total), k
    for _ in range(iters):
        for k, fn in forms:
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    out = {"workload": name, "transcripts": mode, "proofs": total, "shapes": [[g[0], g[1], c] for g, c in zip(groups, counts)], "iters": iters}
    for k, _ in forms:
        med = statistics.median(ts[k])
        out[k + "_ms"] = {"median": round(med * 1e3, 3), "min": round(min(ts[k]) * 1e3, 3), "max": round(max(ts[k]) * 1e3, 3)}
        out[k + "_proofs_per_s"] = round(total / med, 1)
    out["mixed_ts_over_mixed_label"] = round(statistics.median(ts["mixed_ts"]) / statistics.median(ts["mixed_label"]), 3)
    out["batch_ts_over_mixed_ts"] = round(statistics.median(ts["batch_ts"]) / statistics.median(ts["mixed_ts"]), 3)
    out["GPU_MAX_HW_QUEUES"] = os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP default 4)")
    print(json.dumps(out), flush=True)


def run(ctx, name, groups, iters, path):
    counts = [len(g[2]) // g[3] for g in groups]
    total = sum(counts)
    rng = hashlib.shake_256(b"rate-rng-" + name.encode()).digest(64 * total)
    w = hashlib.shake_256(b"rate-w-" + name.encode()).digest(64 * total)

    def per_shape():
        v, off = b"", 0
        for (n, m, proofs, plen, coms, label), nb in zip(groups, counts):
            vg, ok, _ = ctx.rangeproof_verify_rlc(n, m, proofs, plen, coms, label, rng[64 * off:64 * (off + nb)], w[64 * off:64 * (off + nb)])
            assert ok
            v += vg
            off += nb
        return v

    def mixed():
        v, ok, _ = ctx.rangeproof_verify_rlc_mixed(groups, rng, w)
        assert ok
        return v

    forms = [f for f in (("per_shape", per_shape), ("mixed", mixed)) if path in ("both", f[0])]
    ts = {k: [] for k, _ in forms}
    for k, fn in forms:                      # warm-up: tables, scripts, buffers
        assert fn() == bytes(total), k
    for _ in range(iters):                   # interleaved: both forms see the same clocks and the same neighbours
        for k, fn in forms:
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    out = {"workload": name, "proofs": total, "shapes": [[g[0], g[1], c] for g, c in zip(groups, counts)], "iters": iters}
    for k, _ in forms:
        med = statistics.median(ts[k])
        out[k + "_ms"] = {"median": round(med * 1e3, 3), "min": round(min(ts[k]) * 1e3, 3), "max": round(max(ts[k]) * 1e3, 3)}
        out[k + "_proofs_per_s"] = round(total / med, 1)
    if len(forms) == 2:
        out["per_shape_over_mixed"] = round(statistics.median(ts["per_shape"]) / statistics.median(ts["mixed"]), 3)
    out["GPU_MAX_HW_QUEUES"] = os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP default 4)")
    print(json.dumps(out), flush=True)


def main():
    arg = lambda key, default: sys.argv[sys.argv.index(key) + 1] if key in sys.argv else default
    iters, only, path, mode = int(arg("--iters", "10")), arg("--only", None), arg("--path", "both"), arg("--transcripts", "label")
    if mode not in ("label", "shared", "per-proof"):
        sys.exit("--transcripts label|shared|per-proof")
    ctx = bp.Context(0)
    ctx.gens_create(64, 16)

    def go(name, shapes):
        groups = [make(ctx, n, m, c) for n, m, c in shapes]
        if mode == "label":
            run(ctx, name, groups, iters, path)
        else:
            run_ts(ctx, name, groups, [make_ts(ctx, n, m, c, mode == "per-proof") for n, m, c in shapes], iters, mode)

    if only in (None, "block"):
        rnd = random.Random(1024)
        draws = rnd.choices([1, 2, 4, 8, 16], weights=[8, 4, 2, 1, 1], k=1024)
        go("block", [(64, m, draws.count(m)) for m in (1, 2, 4, 8, 16) if draws.count(m)])
    if only in (None, "one_shape"):
        go("one_shape", [(64, 1, 4096)])
    ctx.close()


if __name__ == "__main__":
    main()
