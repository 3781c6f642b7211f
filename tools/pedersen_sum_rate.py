#!/usr/bin/env python3
"""Rows per second of bpgpu_pedersen_sum_batch / bpgpu_pedersen_balance_batch beside the one route the library offered before, same box,
same process, one context with gens_create(64, 1), host pointers (every call ends in its own device synchronise):
  new_sum     : the signed sum of the row's terms plus value B + blinding B_blinding, compressed
  new_balance : does the signed sum open to (value, blinding)?
  new_sum_ct  : new_sum with prover_constant_time = 1
  old_msm     : bpgpu_msm_batch on the same terms with scalars 1 and l - 1, plus (value, B) and (blinding, B_blinding)
at three shapes: 4 096 rows of 2 added + 2 subtracted terms with a u64 value and a blinding; 64 such rows; one row of 65 536 terms.
The C ABI is called through ctypes on buffers made once, so a sample times the library, not Python's packing.  The forms are
interleaved round by round (drift hits them alike); a sample is K back-to-back calls, K chosen so that it lasts about 50 ms; the figure
is the median of the rounds and `spread` is (max - min) / median.  Before anything is timed new_sum's rows are compared with old_msm's,
and new_balance's verdicts are checked both ways (the timed rows do not balance; the same rows with their own sum subtracted do).
CONDITION (exit status 1 when missed): at the 4 096-row shape new_sum and new_balance are both faster than old_msm by more than the
run-to-run spread of the two medians: median_new * (1 + spread_new) < median_old * (1 - spread_old).
    python tools/pedersen_sum_rate.py [--rounds N] [--out profiles/pedersen_sum_rate.json]"""
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bulletproofs_amd as bp  # noqa: E402

L_ORDER = 2**252 + 27742317777372353535851937790883648493
SHAPES = (("4096x(2+2)", 4096, 4), ("64x(2+2)", 64, 4), ("1x65536", 1, 65536))


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    rounds = arg("--rounds", 9)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "pedersen_sum_rate.json"))
    L = bp.lib()
    ctx, ctx_ct = bp.Context(0), bp.Context(0)
    ctx_ct.set_option("prover_constant_time", 1)
    for c in (ctx, ctx_ct):
        c.gens_create(64, 1)
    _, _, B, Bb = ctx.gens_export()
    chk = lambda rc: ctx._chk(rc)
    # the terms: commitments the library makes itself, 4 096 distinct ones, cycled
    npool = 4096
    raw = hashlib.shake_256(b"pedersen-sum-rate").digest(40 * npool)
    pool_bl = b"".join(raw[8 * npool + 32 * i:8 * npool + 32 * i + 31] + b"\x00" for i in range(npool))     # below 2^248: canonical
    pool, _ = ctx.pedersen_commit_batch(raw[:8 * npool], 8, pool_bl)
    one, minus_one = (1).to_bytes(32, "little"), (L_ORDER - 1).to_bytes(32, "little")

    rows, cond = [], {}
    for name, nb, per in SHAPES:
        total = nb * per
        pts = b"".join(pool[32 * ((7 * t) % npool):32 * ((7 * t) % npool) + 32] for t in range(total))
        sg = bytes(((t % per) >= per // 2) for t in range(total))              # the first half of a row added, the second subtracted
        off = (C.c_uint32 * (nb + 1))(*[per * r for r in range(nb + 1)])
        v8 = hashlib.shake_256(b"pedersen-sum-rate-v").digest(8 * nb)
        bl = b"".join(hashlib.shake_256(b"pedersen-sum-rate-b%d" % r).digest(31) + b"\x00" for r in range(nb))
        out, ref, st = C.create_string_buffer(32 * nb), C.create_string_buffer(32 * nb), C.create_string_buffer(nb)
        # the old route's inputs: the same terms with scalars +-1, then the two base terms
        sc2 = b"".join(b"".join(minus_one if sg[per * r + i] else one for i in range(per)) + v8[8 * r:8 * r + 8] + bytes(24) + bl[32 * r:32 * r + 32] for r in range(nb))
        pt2 = b"".join(pts[32 * per * r:32 * per * (r + 1)] + B + Bb for r in range(nb))
        nt = (C.c_uint32 * nb)(*([per + 2] * nb))
        forms = {
            "new_sum": lambda: L.bpgpu_pedersen_sum_batch(ctx.h, nb, off, pts, sg, v8, 8, bl, out, st),
            "new_balance": lambda: L.bpgpu_pedersen_balance_batch(ctx.h, nb, off, pts, sg, v8, 8, bl, st),
            "new_sum_ct": lambda: L.bpgpu_pedersen_sum_batch(ctx_ct.h, nb, off, pts, sg, v8, 8, bl, out, st),
            "old_msm": lambda: L.bpgpu_msm_batch(ctx.h, nb, nt, sc2, pt2, out, st),
        }
        chk(forms["old_msm"]())
        ref.raw = out.raw
        assert st.raw[:nb] == bytes(nb)
        for fname in ("new_sum", "new_sum_ct"):                                    # same bytes first (and the warm-up)
            chk(forms[fname]())
            assert out.raw == ref.raw and st.raw[:nb] == bytes(nb), (name, fname)
        chk(forms["new_balance"]())
        assert st.raw[:nb] == bytes([1]) * nb                                      # random terms do not open to a random (value, blinding) ...
        # ... and the same terms with the sum of the scalar-free call subtracted open to (0, 0): the verdict the timing is not about
        plain = C.create_string_buffer(32 * nb)
        chk(L.bpgpu_pedersen_sum_batch(ctx.h, nb, off, pts, sg, None, 8, None, plain, st))
        off1 = (C.c_uint32 * (nb + 1))(*[(per + 1) * r for r in range(nb + 1)])
        pts1 = b"".join(pts[32 * per * r:32 * per * (r + 1)] + plain.raw[32 * r:32 * r + 32] for r in range(nb))
        sg1 = b"".join(sg[per * r:per * (r + 1)] + b"\x01" for r in range(nb))
        chk(L.bpgpu_pedersen_balance_batch(ctx.h, nb, off1, pts1, sg1, None, 8, None, st))
        assert st.raw[:nb] == bytes(nb), name
        calls = {}
        for fname, f in forms.items():
            t = time.perf_counter()
            chk(f())
            calls[fname] = max(1, min(400, int(0.05 / max(time.perf_counter() - t, 1e-6))))
        samples = {fname: [] for fname in forms}
        for _ in range(rounds):
            for fname, f in forms.items():
                t = time.perf_counter()
                for _ in range(calls[fname]):
                    rc = f()
                samples[fname].append((time.perf_counter() - t) / calls[fname])
                chk(rc)
        med, spread = {}, {}
        for fname, s in samples.items():
            med[fname] = statistics.median(s)
            spread[fname] = (max(s) - min(s)) / med[fname]
            row = {"shape": name, "rows": nb, "terms_per_row": per, "form": fname, "calls_per_sample": calls[fname], "median_ms": round(med[fname] * 1e3, 4),
                   "spread": round(spread[fname], 4), "rows_per_s": round(nb / med[fname]), "terms_per_s": round(total / med[fname])}
            rows.append(row)
            print(json.dumps(row), flush=True)
        if nb == 4096:
            for fname in ("new_sum", "new_balance"):
                cond[fname] = {"median_ms": round(med[fname] * 1e3, 4), "spread": round(spread[fname], 4), "old_msm_over_new": round(med["old_msm"] / med[fname], 2),
                               "met": med[fname] * (1 + spread[fname]) < med["old_msm"] * (1 - spread["old_msm"])}
            cond["old_msm"] = {"median_ms": round(med["old_msm"] * 1e3, 4), "spread": round(spread["old_msm"], 4)}
    ok = cond["new_sum"]["met"] and cond["new_balance"]["met"]
    res = {"tool": "tools/pedersen_sum_rate.py", "gens": [64, 1], "fixed_window_bits": ctx.get_option("fixed_window_bits"), "rounds": rounds, "rows": rows,
           "condition": {"shape": "4096x(2+2)", **cond, "met": ok}}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["condition"]), flush=True)
    ctx.close()
    ctx_ct.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
