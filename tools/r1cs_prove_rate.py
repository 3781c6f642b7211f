#!/usr/bin/env python3
"""R1CS proving rate on the k = 1024 shuffle (padded_n = 2048, 2 048 commitments per proof): bpgpu_r1cs_prove_batch on
  batch : 64 proofs per call
  one   : one proof per call
The gadget is recorded once per proof (bulletproofs_amd.r1cs.Prover); every proof made is checked Ok by bpgpu_r1cs_verify_batch_ts.
    python tools/r1cs_prove_rate.py [--iters N]"""
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

K, NB = 1024, 64


def shuffle_prover(st0, i):
    rnd = random.Random(i)
    inp = [rnd.getrandbits(64) for _ in range(K)]
    out = inp[:]
    rnd.shuffle(out)
    bl = hashlib.shake_256(b"rate-bl%d" % i).digest(64 * 2 * K)
    cs = r1cs.Prover(st0)
    xs = [cs.commit(v, int.from_bytes(bl[64 * j:64 * j + 64], "little")) for j, v in enumerate(inp + out)]
    R.shuffle_gadget(cs, xs[:K], xs[K:])
    return cs


def main():
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 5
    st0 = R.transcript_state(R.T.Transcript(b"ShuffleProofRate"))
    provers = [shuffle_prover(st0, i) for i in range(NB)]
    ins = [p.inputs() for p in provers]
    v, vb, fr = (b"".join(x[j] for x in ins) for j in range(3))
    circuit, w = provers[0].circuit(), provers[0].witness()
    ctx = bp.Context(0)
    ctx.gens_create(2 * K, 1)
    ver = r1cs.Verifier(st0)
    vs = [ver.commit(bytes(32)) for _ in range(2 * K)]
    R.shuffle_gadget(ver, vs[:K], vs[K:])
    vcirc = ver.circuit()
    made = {"batch": [], "one": []}

    def run(nb, key):
        ti = time.perf_counter()
        proofs, coms, status = w.prove_batch(ctx, circuit, nb, v[:64 * K * nb], vb[:64 * K * nb], fr[:len(fr) // NB * nb], st0, None)
        dt = time.perf_counter() - ti
        assert status == bytes(nb), status
        made[key].append((proofs, coms))
        return dt

    t_batch = statistics.median([run(NB, "batch") for _ in range(iters + 1)][1:])
    t_one = statistics.median([run(1, "one") for _ in range(iters + 1)][1:])
    nver = 0
    for key in ("batch", "one"):
        for proofs, coms in made[key]:
            verdict = vcirc.verify_batch(ctx, proofs, coms, st0, rng32=None)
            assert verdict == bytes(len(proofs)), (key, verdict)
            nver += len(proofs)
    print(json.dumps({"k": K, "padded_n": circuit.padded_n, "batch": NB, "iters": iters,
                      "r1cs_prove_batch_proofs_per_s": round(NB / t_batch, 2), "r1cs_prove_batch_ms": round(t_batch * 1e3, 2),
                      "r1cs_prove_one_ms": round(t_one * 1e3, 2), "proofs_verified_ok": nver}))
    ctx.close()


if __name__ == "__main__":
    main()
