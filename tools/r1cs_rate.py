#!/usr/bin/env python3
"""R1CS verification rate on the k = 1024 shuffle (padded_n = 2048, 2 048 commitments, a 6 179-term mega-check per proof):
  batch : bpgpu_r1cs_verify_batch_ts on 64 proofs per call, against bpgpu_msm_batch_shared on 64 mega-checks of the same shape
  one   : one proof per call, against one 6 179-term shared-generator MSM
Proofs come from the test twin (tests/r1cs_twin.py, liboracle.so): 8 distinct proofs tiled to the batch.  Every verdict is checked.
    python tools/r1cs_rate.py [--iters N]"""
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
import pyoracle  # noqa: E402
import r1cs_twin as R  # noqa: E402

K, NB, DISTINCT = 1024, 64, 8


def timed(fn, iters):
    fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 20
    g = pyoracle.Gens(2 * K, 1).export()
    proofs, coms = [], []
    st0 = None
    for i in range(DISTINCT):
        rnd = random.Random(i)
        inp = [rnd.getrandbits(64) for _ in range(K)]
        out = inp[:]
        rnd.shuffle(out)
        pf, Vs, st0 = R.prove_shuffle(g, 2 * K, b"ShuffleProofTest", inp, out, b"rate-%d" % i)
        proofs.append(pf.to_bytes())
        coms.append(b"".join(Vs))
    cs = r1cs.Verifier(st0)
    vs = [cs.commit(bytes(32)) for _ in range(2 * K)]
    R.shuffle_gadget(cs, vs[:K], vs[K:])
    circuit = cs.circuit()
    ctx = bp.Context(0)
    ctx.gens_create(2 * K, 1)
    bp_ = [proofs[i % DISTINCT] for i in range(NB)]
    bc = b"".join(coms[i % DISTINCT] for i in range(NB))
    rng = hashlib.shake_256(b"rate").digest(32 * NB)
    v = circuit.verify_batch(ctx, bp_, bc, st0, rng32=rng)
    assert v == bytes(NB), v
    t_batch = timed(lambda: circuit.verify_batch(ctx, bp_, bc, st0, rng32=rng), iters)
    t_one = timed(lambda: circuit.verify_batch(ctx, bp_[:1], bc[:64 * K], st0, rng32=rng[:32]), iters)
    # the same mega-check shape through the shared-generator MSM alone (scalars: random; points: the proofs' own)
    n_u = circuit.n_unique
    sh = hashlib.shake_256(b"rate-scalars").digest((2 * 2 * K + 2 + n_u) * 32 * NB)
    sc = lambda off, cnt: b"".join((int.from_bytes(sh[32 * (off + j):32 * (off + j) + 32], "little") % R.L).to_bytes(32, "little") for j in range(cnt))
    gen_sc = sc(0, (4 * K + 2) * NB)
    u_sc = sc((4 * K + 2) * NB, n_u * NB)
    pts = []
    for i in range(NB):
        p = bp_[i]
        d = R.parse(p)
        pts.append(b"".join([d["A_I1"], d["A_O1"], d["S1"], d["A_I2"], d["A_O2"], d["S2"]]) + coms[i % DISTINCT] +
                   b"".join(d[x] for x in ("T_1", "T_3", "T_4", "T_5", "T_6")) + b"".join(d["L"]) + b"".join(d["R"]))
    u_pt = b"".join(pts)
    m_batch = timed(lambda: ctx.msm_batch_shared(2 * K, 1, NB, n_u, gen_sc, u_sc, u_pt), iters)
    m_one = timed(lambda: ctx.msm_batch_shared(2 * K, 1, 1, n_u, gen_sc[:(4 * K + 2) * 32], u_sc[:n_u * 32], u_pt[:n_u * 32]), iters)
    print(json.dumps({"k": K, "padded_n": circuit.padded_n, "terms": 4 * K + 2 + n_u, "batch": NB,
                      "r1cs_batch_proofs_per_s": round(NB / t_batch, 1), "msm_shared_batch_per_s": round(NB / m_batch, 1),
                      "batch_ratio": round(m_batch / t_batch, 3),
                      "r1cs_one_ms": round(t_one * 1e3, 3), "msm_shared_one_ms": round(m_one * 1e3, 3),
                      "one_overhead_ms": round((t_one - m_one) * 1e3, 3)}))
    ctx.close()


if __name__ == "__main__":
    main()
