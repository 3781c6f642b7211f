#!/usr/bin/env python3
"""Batch-combined R1CS verification (bpgpu_r1cs_verify_rlc) against the per-proof path (bpgpu_r1cs_verify_batch_ts), on:
  shuffle64   : 64 k = 1024 shuffles (padded_n = 2048, 2 081 points per proof)
  shuffle1024 : 1 024 of them (about 2.1 M proof-specific terms in one combination)
  mixed       : 256 proofs of 7 gadgets (shuffles k = 2, 8, 32, 128; range gadgets n = 8, 64; the example gadget); the per-proof path is
                one bpgpu_r1cs_verify_batch_ts call per gadget
Proofs are made on the GPU (bpgpu_r1cs_prove_batch) from a few recorded witnesses per gadget, tiled with distinct rng bytes.  Every
verdict is checked; both paths get the same rng32 bytes, the combined one the same weights64 each time.
    python tools/r1cs_rlc_rate.py [--iters N] [--only shuffle64|shuffle1024|mixed] [--path both|per_proof|combined]
                                  [--save FILE | --load FILE]   (make the proofs once; verify them in a separate, e.g. profiled, run)"""
import hashlib
import json
import os
import pickle
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "oracle", "py"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import bulletproofs_amd as bp  # noqa: E402
from bulletproofs_amd import r1cs  # noqa: E402
import r1cs_twin as R  # noqa: E402

DISTINCT = 4


def timed(fn, iters):
    fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def _scalars(tag, n):
    return [int.from_bytes(hashlib.shake_256(tag + b"%d" % i).digest(64), "little") % R.L for i in range(n)]


def _shuffle_vals(k, seed):
    rnd = random.Random(seed)
    inp = [rnd.getrandbits(64) for _ in range(k)]
    out = inp[:]
    rnd.shuffle(out)
    return inp + out


# name -> (values of one witness, the gadget given the values (None on the verifier side))
def _gadget(name):
    kind, arg = name.split(":")
    arg = int(arg)
    if kind == "shuffle":
        return (lambda s: _shuffle_vals(arg, s)), (lambda vals: lambda cs, v: R.shuffle_gadget(cs, v[:arg], v[arg:]))
    if kind == "range":
        return (lambda s: [random.Random(s).getrandbits(arg)]), (lambda vals: lambda cs, v: R.range_gadget(cs, v[0], vals[0] if vals else None, arg))
    return (lambda s: [3, 4, 6, 1, 40]), (lambda vals: lambda cs, v: R.example_gadget(cs, v[0], v[1], v[2], v[3], v[4], 9))


def make(ctx, name, count):
    """count proofs of one gadget made on the GPU: (name, proofs, commitments, transcript state)"""
    vals_of, gadget_of = _gadget(name)
    st0 = R.transcript_state(R.T.Transcript(b"rlc-rate-" + name.encode()))
    provers = []
    for b in range(DISTINCT):
        vals = vals_of(100 + b)
        cs = r1cs.Prover(st0)
        xs = [cs.commit(v, x) for v, x in zip(vals, _scalars(b"rate-bl-%s-%d-" % (name.encode(), b), len(vals)))]
        gadget_of(vals)(cs, xs)
        provers.append(cs)
    ins = [p.inputs() for p in provers]
    proofs, coms = [], b""
    for s0 in range(0, count, 64):
        nb = min(64, count - s0)
        sel = [ins[(s0 + i) % DISTINCT] for i in range(nb)]
        rng = hashlib.shake_256(b"rate-prove-%s-%d" % (name.encode(), s0)).digest(32 * nb)
        pr, cm, status = provers[0].witness().prove_batch(ctx, provers[0].circuit(), nb, b"".join(i[0] for i in sel), b"".join(i[1] for i in sel),
                                                         b"".join(i[2] for i in sel), st0, rng)
        assert status == bytes(nb), name
        proofs += pr
        coms += cm
    return name, proofs, coms, st0


def group(name, proofs, coms, st0):
    """the verifier's own recording of the gadget (the same constraints as the prover's): (circuit, proofs, commitments, transcript)"""
    vals_of, gadget_of = _gadget(name)
    cs = r1cs.Verifier(st0)
    vs = [cs.commit(bytes(32)) for _ in range(len(vals_of(0)))]
    gadget_of(None)(cs, vs)
    return cs.circuit(), proofs, coms, st0


def run(ctx, name, groups, iters, path):
    n = sum(len(g[1]) for g in groups)
    rng = hashlib.shake_256(b"rate-rng-" + name.encode()).digest(32 * n)
    w = hashlib.shake_256(b"rate-w-" + name.encode()).digest(64 * n)

    def per_proof():
        v, off = b"", 0
        for circ, proofs, coms, st0 in groups:
            v += circ.verify_batch(ctx, proofs, coms, st0, rng32=rng[32 * off:32 * (off + len(proofs))])
            off += len(proofs)
        return v

    def combined():
        return r1cs.verify_batch_combined(ctx, groups, rng32=rng, weights64=w, want_batch=True)

    if path != "combined":
        assert per_proof() == bytes(n)
    if path != "per_proof":
        v, batch = combined()
        assert v == bytes(n) and batch == bytes(33)
    t_p = timed(per_proof, iters) if path != "combined" else float("nan")
    t_c = timed(combined, iters) if path != "per_proof" else float("nan")
    print(json.dumps({"workload": name, "proofs": n, "gadgets": len(groups), "per_proof_calls_per_s": round(1 / t_p, 2),
                      "combined_calls_per_s": round(1 / t_c, 2), "per_proof_ms": round(t_p * 1e3, 3), "combined_ms": round(t_c * 1e3, 3),
                      "per_proof_proofs_per_s": round(n / t_p, 1), "combined_proofs_per_s": round(n / t_c, 1), "speedup": round(t_p / t_c, 3),
                      "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP default 4)")}),
          flush=True)


def main():
    arg = lambda key, default: sys.argv[sys.argv.index(key) + 1] if key in sys.argv else default
    iters, only, path = int(arg("--iters", "10")), arg("--only", None), arg("--path", "both")
    save, load = arg("--save", None), arg("--load", None)   # (proofs made once, then a profiled run that verifies only)
    ctx = bp.Context(0)
    ctx.gens_create(2048, 1)
    if load:
        with open(load, "rb") as f:
            made = pickle.load(f)
    else:
        made = {}
        if only in (None, "shuffle64", "shuffle1024"):
            made["big"] = [make(ctx, "shuffle:1024", 1024)]
        if only in (None, "mixed"):
            mix = [("shuffle:2", 48), ("shuffle:8", 48), ("shuffle:32", 40), ("shuffle:128", 24), ("range:8", 40), ("range:64", 32), ("example:0", 24)]
            made["mixed"] = [make(ctx, nm, cnt) for nm, cnt in mix]
        if save:
            with open(save, "wb") as f:
                pickle.dump(made, f)
            ctx.close()
            return
    if "big" in made:
        big = group(*made["big"][0])
        if only in (None, "shuffle64"):
            run(ctx, "shuffle64", [(big[0], big[1][:64], big[2][:64 * 2048 * 32], big[3])], iters, path)
        if only in (None, "shuffle1024"):
            run(ctx, "shuffle1024", [big], max(2, iters // 4), path)
    if "mixed" in made and only in (None, "mixed"):
        run(ctx, "mixed", [group(*m) for m in made["mixed"]], iters, path)
    ctx.close()


if __name__ == "__main__":
    main()
