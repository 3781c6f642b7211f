#!/usr/bin/env python3
"""What the R1CS witness check costs, on shuffle gadgets of k = 64 and k = 1 024 in batches of 64 and 1 024:
  prove   : bpgpu_r1cs_prove_batch (the baseline, unchanged)
  checked : bpgpu_r1cs_prove_batch_checked on the same all-satisfied inputs (byte-identical proofs: asserted)
  check   : bpgpu_r1cs_witness_check alone on the same values, free inputs and one challenge per proof
  verify  : bpgpu_r1cs_verify_batch_ts of the proofs made (prove + verify is the round trip a gadget test pays without the check)
One process, one context; the calls alternate, 10 each after one warm-up each, host clock around the call; medians.  Inputs are
a few recorded provers tiled over the batch.  Writes profiles/r1cs_check_rate.json and prints one JSON line per shape.
    python tools/r1cs_check_rate.py [--iters N] [--only K,NB]"""
import hashlib
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "oracle", "py"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

import bulletproofs_amd as bp  # noqa: E402
from bulletproofs_amd import r1cs  # noqa: E402
import r1cs_twin as R  # noqa: E402

DISTINCT = 4


def shuffle_prover(st0, k, i):
    rnd = random.Random(1000 * k + i)
    inp = [rnd.getrandbits(64) for _ in range(k)]
    out = inp[:]
    rnd.shuffle(out)
    bl = hashlib.shake_256(b"check-rate-bl%d/%d" % (k, i)).digest(64 * 2 * k)
    cs = r1cs.Prover(st0)
    xs = [cs.commit(v, int.from_bytes(bl[64 * j:64 * j + 64], "little")) for j, v in enumerate(inp + out)]
    R.shuffle_gadget(cs, xs[:k], xs[k:])
    return cs


def measure(ctx, k, nb, iters):
    st0 = R.transcript_state(R.T.Transcript(b"ShuffleCheckRate"))
    provers = [shuffle_prover(st0, k, i) for i in range(DISTINCT)]
    ins = [p.inputs() for p in provers]
    tile = lambda j: b"".join(ins[b % DISTINCT][j] for b in range(nb))
    v, vb, fr = tile(0), tile(1), tile(2)
    circuit, w = provers[0].circuit(), provers[0].witness()
    rng32 = hashlib.shake_256(b"check-rate-rng%d/%d" % (k, nb)).digest(32 * nb)
    chal = b"".join((int.from_bytes(hashlib.shake_256(b"check-rate-ch%d" % b).digest(64), "little") % r1cs.L_ORDER).to_bytes(32, "little")
                    for b in range(nb * circuit.n_challenges))
    ver = r1cs.Verifier(st0)
    vs = [ver.commit(bytes(32)) for _ in range(2 * k)]
    R.shuffle_gadget(ver, vs[:k], vs[k:])
    vcirc = ver.circuit()
    keep = {}

    def prove():
        keep["prove"] = w.prove_batch(ctx, circuit, nb, v, vb, fr, st0, rng32)

    def checked():
        keep["checked"] = w.prove_batch(ctx, circuit, nb, v, vb, fr, st0, rng32, check=True)

    def check():
        keep["check"] = w.check_batch(ctx, circuit, nb, v, fr, chal)

    def verify():
        keep["verify"] = vcirc.verify_batch(ctx, keep["prove"][0], keep["prove"][1], st0, rng32=None)

    calls = [("prove", prove), ("checked", checked), ("check", check), ("verify", verify)]
    times = {name: [] for name, _ in calls}
    for it in range(iters + 1):                 # (round 0 warms up: buffers, the circuit's row form)
        for name, fn in calls:
            t0 = time.perf_counter()
            fn()
            if it:
                times[name].append(time.perf_counter() - t0)
    assert keep["prove"][2] == bytes(nb) and keep["checked"][:3] == keep["prove"][:3] and keep["checked"][3] == [r1cs.SATISFIED] * nb
    assert keep["check"] == ([r1cs.SATISFIED] * nb, bytes(nb)) and keep["verify"] == bytes(nb)
    med = {name: statistics.median(ts) * 1e3 for name, ts in times.items()}
    return {"gadget": "shuffle", "k": k, "padded_n": circuit.padded_n, "constraints": circuit.n_constraints, "batch": nb, "iters": iters,
            "prove_ms": round(med["prove"], 3), "prove_checked_ms": round(med["checked"], 3), "witness_check_ms": round(med["check"], 3),
            "verify_ms": round(med["verify"], 3), "checked_over_prove": round(med["checked"] / med["prove"], 4),
            "check_over_prove_plus_verify": round(med["check"] / (med["prove"] + med["verify"]), 4)}


def main():
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 10
    shapes = [(64, 64), (64, 1024), (1024, 64), (1024, 1024)]
    if "--only" in sys.argv:
        shapes = [tuple(int(x) for x in sys.argv[sys.argv.index("--only") + 1].split(","))]
    ctx = bp.Context(0)
    ctx.gens_create(2048, 1)
    rows = []
    for k, nb in shapes:
        rows.append(measure(ctx, k, nb, iters))
        print(json.dumps(rows[-1]), flush=True)
    ctx.close()
    if "--only" not in sys.argv:
        with open(os.path.join(ROOT, "profiles", "r1cs_check_rate.json"), "w") as f:
            json.dump({"tool": "tools/r1cs_check_rate.py", "device": "MI355X", "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
