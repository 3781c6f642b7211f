#!/usr/bin/env python3
"""The batch-combined check over range proofs of MIXED shapes (bpgpu_rangeproof_verify_rlc_mixed) against the same proofs sent as one
bpgpu_rangeproof_verify_rlc call per shape, on:
  block       : 1 024 proofs at n = 64 with m drawn from {1, 2, 4, 8, 16}, weighted 8 : 4 : 2 : 1 : 1 (a block of confidential
                transactions: aggregated proofs of different output counts side by side)
  one_shape   : 4 096 proofs of (64, 1) alone through both entry points -- on one shape the mixed path should cost what the one-shape
                path costs
Proofs are made on the GPU (bpgpu_rangeproof_prove_batch).  The two forms run interleaved, blocking calls, the same rng64 / weights64
bytes each time; every verdict is checked.  One JSON line per workload: median and spread (min .. max) per form.
    python tools/rlc_mixed_rate.py [--iters N] [--only block|one_shape] [--path both|per_shape|mixed]"""
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
    iters, only, path = int(arg("--iters", "10")), arg("--only", None), arg("--path", "both")
    ctx = bp.Context(0)
    ctx.gens_create(64, 16)
    if only in (None, "block"):
        rnd = random.Random(1024)
        draws = rnd.choices([1, 2, 4, 8, 16], weights=[8, 4, 2, 1, 1], k=1024)
        run(ctx, "block", [make(ctx, 64, m, draws.count(m)) for m in (1, 2, 4, 8, 16) if draws.count(m)], iters, path)
    if only in (None, "one_shape"):
        run(ctx, "one_shape", [make(ctx, 64, 1, 4096)], iters, path)
    ctx.close()


if __name__ == "__main__":
    main()
