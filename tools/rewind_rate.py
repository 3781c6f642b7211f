#!/usr/bin/env python3
"""Rows per second of bpgpu_rangeproof_rewind_batch beside bpgpu_rangeproof_verify_batch_ts on the same proofs, and proofs per second of
bpgpu_rangeproof_prove_batch_rw beside bpgpu_rangeproof_prove_batch_ts on the same inputs: same box, same process, one context with
gens_create(64, 1), host pointers (every call ends in its own device synchronise), n = 64, one transcript state per row.
  rewind_all_mine  : every row is the wallet's (its own seed): replay, scalars, walk, encode
  rewind_none_mine : no row is (wrong seeds): replay and the test e < 2^192; whole wavefronts skip the walk
  rewind_ct        : every row the wallet's on a second context with prover_constant_time = 1 (every row walks the W = 4 table)
  dev_all_mine / dev_none_mine / dev_ct : the same three through bpgpu_rangeproof_rewind_batch_dev on device-resident buffers, K calls
                     enqueued and ONE synchronise per sample: the launch itself, without the host call's staging (944 bytes per row in,
                     57 out, through the pinned block)
  verify           : bpgpu_rangeproof_verify_batch_ts on the same proofs -- the yardstick: a scan that costs as much as verifying
                     would not be worth a kernel
  prove_rw / prove_ts : the two provers; they differ by one scalar subtraction per proof
at 64, 4 096 and 65 536 rows per call.  The C ABI is called through ctypes on buffers made once; the forms are interleaved round by
round; a sample is K back-to-back calls, K chosen so that it lasts about 50 ms; the figure is the median of the rounds and `spread` is
(max - min) / median.  Before anything is timed the rewinder's outputs are compared with what went into the proofs, and the proofs are
verified.  The provers are timed up to --prove-max rows (their working set grows with n per proof).
CONDITIONS (exit status 1 when one is missed): at every size dev_none_mine is faster than dev_all_mine beyond the two spreads (else the
skip of the walk is not working), and rewind_all_mine is faster than verify beyond the two spreads.  The same comparison of the two
host-pointer forms is recorded beside it.  The provers' medians are
reported with whether they differ by more than the two spreads together.
    python tools/rewind_rate.py [--rounds N] [--sizes 64,4096,65536] [--prove-max 4096] [--out profiles/rewind_rate.json]"""
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
import torch  # noqa: E402

TS, N = 208, 64
PL = 32 * (9 + 2 * 6)


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    rounds = arg("--rounds", 9)
    sizes = [int(x) for x in arg("--sizes", "64,4096,65536").split(",")]
    prove_max = arg("--prove-max", 4096)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "rewind_rate.json"))
    L = bp.lib()
    ctx, ctx_ct = bp.Context(0), bp.Context(0)
    ctx_ct.set_option("prover_constant_time", 1)
    for c in (ctx, ctx_ct):
        c.gens_create(64, 1)
    rows, cond = [], {}
    ok = True
    for nb in sizes:
        raw = hashlib.shake_256(b"rewind-rate-%d" % nb).digest(120 * nb)
        vals = [int.from_bytes(raw[8 * i:8 * i + 8], "little") for i in range(nb)]
        bl = b"".join(raw[8 * nb + 32 * i:8 * nb + 32 * i + 31] + b"\x00" for i in range(nb))     # below 2^248: canonical
        seeds, wrong, msgs = raw[40 * nb:72 * nb], raw[72 * nb:104 * nb], raw[104 * nb:120 * nb]
        states, _ = ctx.transcript_batch(nb, [("append_u64", b"session", list(range(nb)))], label=b"rewind rate")
        proofs, coms = b"", b""
        for lo in range(0, nb, prove_max):                                                         # (the prover's working set bounds its batch)
            hi = min(nb, lo + prove_max)
            p, c = ctx.rangeproof_prove_batch_rw(N, 1, vals[lo:hi], bl[32 * lo:32 * hi], states[TS * lo:TS * hi], seeds[32 * lo:32 * hi], msgs[16 * lo:16 * hi])
            proofs, coms = proofs + p, coms + c
        # ---- the same answers first
        for c in (ctx, ctx_ct):
            st, v, m, g = c.rangeproof_rewind_batch(N, proofs, PL, coms, states, seeds)
            assert st == bytes(nb) and v == vals and m == msgs and g == bl, nb
            st, v, m, g = c.rangeproof_rewind_batch(N, proofs, PL, coms, states, wrong)
            assert st == bytes([1]) * nb and not any(v) and m == bytes(16 * nb) and g == bytes(32 * nb), nb
        assert bytes(ctx.rangeproof_verify_batch_ts(N, 1, proofs, PL, coms, states)) == bytes(nb)
        rng64 = hashlib.shake_256(b"rewind-rate-rng").digest(64 * nb)
        st_o, v_o, m_o, g_o, vd = C.create_string_buffer(nb), (C.c_uint64 * nb)(), C.create_string_buffer(16 * nb), C.create_string_buffer(32 * nb), C.create_string_buffer(nb)
        npv = min(nb, prove_max)
        va = (C.c_uint64 * npv)(*vals[:npv])
        p_o, c_o = C.create_string_buffer(PL * npv), C.create_string_buffer(32 * npv)
        dev = torch.device("cuda:0")
        up = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)
        d_pr, d_cm, d_ts, d_seed, d_wrong = up(proofs), up(coms), up(states), up(seeds), up(wrong)
        d_st, d_m, d_g = (torch.zeros((k * nb,), dtype=torch.uint8, device=dev) for k in (1, 16, 32))
        d_v = torch.zeros((nb,), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

        def dev_form(c, d_s):
            def enqueue():
                c.rangeproof_rewind_batch_dev(N, nb, d_pr.data_ptr(), PL, d_cm.data_ptr(), d_ts.data_ptr(), TS, d_s.data_ptr(), d_st.data_ptr(), d_v.data_ptr(),
                                              d_m.data_ptr(), d_g.data_ptr())
                return 0
            return enqueue
        dev_forms = {"dev_all_mine": (ctx, dev_form(ctx, d_seed)), "dev_none_mine": (ctx, dev_form(ctx, d_wrong)), "dev_ct": (ctx_ct, dev_form(ctx_ct, d_seed))}
        for c, f in dev_forms.values():
            f()
            c.synchronize()
        assert bytes(d_st.cpu().numpy()) == bytes(nb) and bytes(d_g.cpu().numpy()) == bl      # (the last one enqueued: dev_ct, every row the wallet's)
        forms = {
            "rewind_all_mine": lambda: L.bpgpu_rangeproof_rewind_batch(ctx.h, N, nb, proofs, PL, coms, states, TS, seeds, st_o, v_o, m_o, g_o),
            "rewind_none_mine": lambda: L.bpgpu_rangeproof_rewind_batch(ctx.h, N, nb, proofs, PL, coms, states, TS, wrong, st_o, v_o, m_o, g_o),
            "rewind_ct": lambda: L.bpgpu_rangeproof_rewind_batch(ctx_ct.h, N, nb, proofs, PL, coms, states, TS, seeds, st_o, v_o, m_o, g_o),
            "verify": lambda: L.bpgpu_rangeproof_verify_batch_ts(ctx.h, N, 1, nb, proofs, PL, coms, states, TS, rng64, vd, None, None),
            "prove_rw": lambda: L.bpgpu_rangeproof_prove_batch_rw(ctx.h, N, 1, npv, va, bl, states, TS, seeds, msgs, p_o, c_o, None),
            "prove_ts": lambda: L.bpgpu_rangeproof_prove_batch_ts(ctx.h, N, 1, npv, va, bl, states, TS, seeds, p_o, c_o, None),
        }
        sync = {fname: (lambda: None) for fname in forms}
        for fname, (c, f) in dev_forms.items():
            forms[fname], sync[fname] = f, c.synchronize
        count = {f: (npv if f.startswith("prove") else nb) for f in forms}
        calls = {}
        for fname, f in forms.items():
            ctx._chk(f())                                                                          # (warm-up)
            sync[fname]()
            t = time.perf_counter()
            ctx._chk(f())
            sync[fname]()
            calls[fname] = max(1, min(400, int(0.05 / max(time.perf_counter() - t, 1e-6))))
        samples = {fname: [] for fname in forms}
        for _ in range(rounds):
            for fname, f in forms.items():
                t = time.perf_counter()
                for _ in range(calls[fname]):
                    rc = f()
                sync[fname]()
                samples[fname].append((time.perf_counter() - t) / calls[fname])
                ctx._chk(rc)
        med, spread = {}, {}
        for fname, s in samples.items():
            med[fname] = statistics.median(s)
            spread[fname] = (max(s) - min(s)) / med[fname]
            row = {"rows": count[fname], "call": fname, "calls_per_sample": calls[fname], "median_ms": round(med[fname] * 1e3, 4), "spread": round(spread[fname], 4),
                   "rows_per_s": round(count[fname] / med[fname])}
            rows.append(row)
            print(json.dumps(row), flush=True)
        beyond = lambda a, b: med[a] * (1 + spread[a]) < med[b] * (1 - spread[b])
        cond[str(nb)] = {"none_mine_faster_than_all_mine": beyond("dev_none_mine", "dev_all_mine"),
                         "none_mine_faster_than_all_mine_host_pointers": beyond("rewind_none_mine", "rewind_all_mine"),
                         "dev_all_over_none_mine": round(med["dev_all_mine"] / med["dev_none_mine"], 2), "all_mine_faster_than_verify": beyond("rewind_all_mine", "verify"),
                         "verify_over_all_mine": round(med["verify"] / med["rewind_all_mine"], 2), "verify_over_none_mine": round(med["verify"] / med["rewind_none_mine"], 2),
                         "prove_rw_over_prove_ts": round(med["prove_rw"] / med["prove_ts"], 4),
                         "provers_differ_beyond_spreads": abs(med["prove_rw"] - med["prove_ts"]) > spread["prove_rw"] * med["prove_rw"] + spread["prove_ts"] * med["prove_ts"]}
        ok = ok and cond[str(nb)]["none_mine_faster_than_all_mine"] and cond[str(nb)]["all_mine_faster_than_verify"]
    res = {"tool": "tools/rewind_rate.py", "gens": [64, 1], "n": N, "fixed_window_bits": ctx.get_option("fixed_window_bits"), "rounds": rounds, "prove_max": prove_max,
           "rows": rows, "conditions": {**cond, "met": ok}}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["conditions"]), flush=True)
    ctx.close()
    ctx_ct.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
