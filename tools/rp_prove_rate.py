#!/usr/bin/env python3
"""Range-proof proving rate, on one context, of the five ways a caller can get nbatch proofs of one shape:
  1 buffer      : bpgpu_rangeproof_prove_batch with a pre-drawn rng buffer (64 bytes per random scalar)
  2 buffer_null : the same with rng = NULL (the library draws every scalar's bytes on the calling thread and uploads them)
  3 seeded      : bpgpu_rangeproof_prove_batch_ts, rng32 given, one shared transcript
  4 seeded_null : bpgpu_rangeproof_prove_batch_ts, rng32 = NULL, one transcript per proof
  5 singles     : nbatch calls of bpgpu_rangeproof_prove_batch with nbatch = 1 -- what a caller with one transcript per proof had to do
                  (taken up to 256 proofs)
Shapes: (64, 1) x {1, 64, 1024, 4096} and (64, 16) x 256.  Every form is warmed up at every shape, then the forms are timed in turn,
round after round (so drift of a shared host hits all of them alike); a sample is as many calls as fill SAMPLE_S seconds, each call
ending in the library's own stream synchronise, and a form's figure is the median over the rounds.  One proof batch of forms 3 and 4
per shape is verified by bpgpu_rangeproof_verify_batch_ts.
    python tools/rp_prove_rate.py [--rounds N] [--out FILE]"""
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
from bulletproofs_amd._lib import transcript_append_message, transcript_new  # noqa: E402

SHAPES = [(64, 1, 1), (64, 1, 64), (64, 1, 1024), (64, 1, 4096), (64, 16, 256)]
FORMS = ["buffer", "buffer_null", "seeded", "seeded_null", "singles"]
SAMPLE_S, MAX_CALLS, SINGLES_MAX = 0.25, 200, 256
BOUND = 0.95   # form 3 against form 1 at 1024 x (64, 1): the run-to-run spread of this box class (README)


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 7
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "rp_prove_rate.json")
    ctx = bp.Context(0)
    ctx.gens_create(64, 16)
    start = transcript_append_message(transcript_new(b"payment-protocol v3"), b"session", b"rate")
    rows = []
    for n, m, nb in SHAPES:
        per = 64 * (m * (2 * n + 2) + 2 * m)
        vals = [int.from_bytes(hashlib.shake_256(b"rate-v%d" % i).digest(8), "little") for i in range(nb * m)]
        bl = b"".join(hashlib.shake_256(b"rate-b%d" % i).digest(31) + b"\x00" for i in range(nb * m))
        rng = hashlib.shake_256(b"rate-rng").digest(per * nb)
        seeds = hashlib.shake_256(b"rate-seeds").digest(32 * nb)
        states = [transcript_append_message(start, b"proof", i.to_bytes(4, "little")) for i in range(nb)]
        all_states = b"".join(states)

        def singles():
            for i in range(nb):
                ctx.rangeproof_prove_batch(n, m, vals[m * i:m * (i + 1)], bl[32 * m * i:32 * m * (i + 1)], transcript=states[i], rng=rng[per * i:per * (i + 1)])
        calls = {
            "buffer": lambda: ctx.rangeproof_prove_batch(n, m, vals, bl, transcript=start, rng=rng),
            "buffer_null": lambda: ctx.rangeproof_prove_batch(n, m, vals, bl, transcript=start, rng=None),
            "seeded": lambda: ctx.rangeproof_prove_batch_ts(n, m, vals, bl, start, seeds),
            "seeded_null": lambda: ctx.rangeproof_prove_batch_ts(n, m, vals, bl, all_states, None),
        }
        if nb <= SINGLES_MAX:
            calls["singles"] = singles
        # the new forms make proofs the verifier accepts on the same transcripts (and form 3 the bytes of form 1 on another draw source:
        # tests/test_gpu_prover_seeded.py)
        pr, cm = calls["seeded"]()
        pl = len(pr) // nb
        assert bytes(ctx.rangeproof_verify_batch_ts(n, m, pr, pl, cm, start)) == bytes(nb)
        pr, cm = calls["seeded_null"]()
        assert bytes(ctx.rangeproof_verify_batch_ts(n, m, pr, pl, cm, all_states)) == bytes(nb)
        reps = {}
        for f, fn in calls.items():   # warm-up: twice, the second one sizes the samples
            fn()
            t0 = time.perf_counter()
            fn()
            reps[f] = max(1, min(MAX_CALLS, int(SAMPLE_S / max(time.perf_counter() - t0, 1e-6))))
        samples = {f: [] for f in calls}
        for _ in range(rounds):
            for f, fn in calls.items():
                t0 = time.perf_counter()
                for _ in range(reps[f]):
                    fn()
                samples[f].append((time.perf_counter() - t0) / reps[f])
        row = {"n": n, "m": m, "nbatch": nb, "rounds": rounds, "calls_per_sample": reps}
        for f in calls:
            t = statistics.median(samples[f])
            row[f] = {"ms_per_batch": round(t * 1e3, 4), "proofs_per_s": round(nb / t, 1), "min_ms": round(min(samples[f]) * 1e3, 4),
                      "max_ms": round(max(samples[f]) * 1e3, 4)}
        rate = lambda f: row[f]["proofs_per_s"]
        row["ratio_3_over_1"] = round(rate("seeded") / rate("buffer"), 4)
        row["ratio_3_over_2"] = round(rate("seeded") / rate("buffer_null"), 4)
        if "singles" in calls:
            row["ratio_4_over_5"] = round(rate("seeded_null") / rate("singles"), 4)
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    key = next(r for r in rows if (r["n"], r["m"], r["nbatch"]) == (64, 1, 1024))
    result = {"forms": FORMS, "shapes": rows, "bound_form3_over_form1_at_1024x64x1": BOUND, "measured_form3_over_form1_at_1024x64x1": key["ratio_3_over_1"],
              "bound_met": key["ratio_3_over_1"] >= BOUND}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k != "shapes"}))


if __name__ == "__main__":
    main()
