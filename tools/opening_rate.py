#!/usr/bin/env python3
"""Proofs per second of bpgpu_opening_create_batch_ts / _verify_batch_ts / _verify_rlc_ts beside the route the library offered before,
same box, same process, one context with gens_create(64, 1), host pointers (every call ends in its own device synchronise):
  new_create   : the proofs of a batch, one launch
  new_verify   : every proof on its own (front end, the shared-generator chain with two points per row, verdicts)
  new_combined : ONE combined check over 2 nbatch points
  old_verify   : bpgpu_transcript_batch running the protocol's script for c, then bpgpu_msm_batch on the four terms per row
                 (s_v, B), (s_r, B_blinding), (l - c, C), (l - 1, R) and the identity test.  Only the two library calls are timed: the
                 host arithmetic between them (l - c, and c v in form 1, per row) is prepared outside the samples, so the figure is a LOWER
                 bound of the old route
  old_create   : bpgpu_pedersen_commit_batch for R = k_v B + k_r B_blinding, then bpgpu_transcript_batch for c; the host's two
                 multiply-adds per row are likewise not timed
at 64, 4 096 and 65 536 proofs per call, in form 1 with the public value 0 (the excess proof) and in form 0, one transcript state per proof.
The C ABI is called through ctypes on buffers made once; the forms are interleaved round by round; a sample is K back-to-back calls, K
chosen so that it lasts about 50 ms; the figure is the median of the rounds and `spread` is (max - min) / median.  Before anything is
timed the old route's verdicts are compared with the new calls' (all valid, and with one proof in 64 spoiled).
CONDITION (exit status 1 when missed): at 4 096 proofs, in both forms, new_combined is faster than old_verify by more than the
run-to-run spread of the two medians: median_new * (1 + spread_new) < median_old * (1 - spread_old).
    python tools/opening_rate.py [--rounds N] [--sizes 64,4096,65536] [--out profiles/opening_rate.json]"""
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
from bulletproofs_amd import _lib  # noqa: E402

L_ORDER = 2**252 + 27742317777372353535851937790883648493
TS = 208


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def le32(x):
    return int(x).to_bytes(32, "little")


def script(ctx, nb, form, coms, vals32, Rs, c_out):
    """the protocol's transcript script as a bpgpu_ts_op array over buffers that stay alive: (array, count, keep)"""
    keep = [C.create_string_buffer(b"openingproof v1", 15), (C.c_uint64 * 1)(form), C.create_string_buffer(coms, len(coms)), C.create_string_buffer(Rs, len(Rs))]
    raw = [(_lib.TS_APPEND, b"dom-sep", C.addressof(keep[0]), 0, 15, None), (_lib.TS_APPEND_U64, b"form", C.addressof(keep[1]), 0, 8, None),
           (_lib.TS_APPEND, b"C", C.addressof(keep[2]), 32, 32, None)]
    if form == 1:
        keep.append(C.create_string_buffer(vals32, len(vals32)))
        raw.append((_lib.TS_APPEND, b"v", C.addressof(keep[-1]), 32, 32, None))
    raw += [(_lib.TS_APPEND, b"R", C.addressof(keep[3]), 32, 32, None), (_lib.TS_CHALLENGE_SCALAR, b"c", C.addressof(c_out), 32, 0, None)]
    arr, keep2 = ctx._ts_ops(raw)
    return arr, len(raw), keep + [keep2]


def main():
    rounds = arg("--rounds", 9)
    sizes = [int(x) for x in arg("--sizes", "64,4096,65536").split(",")]
    out_path = arg("--out", os.path.join(ROOT, "profiles", "opening_rate.json"))
    L = bp.lib()
    ctx = bp.Context(0)
    ctx.gens_create(64, 1)
    _, _, B, Bb = ctx.gens_export()
    chk = lambda rc: ctx._chk(rc)
    rows, cond = [], {}
    for nb in sizes:
        for form in (1, 0):
            pl = 96 if form == 0 else 64
            tag = b"opening-rate-%d-%d" % (nb, form)
            raw = hashlib.shake_256(tag).digest(72 * nb)
            v8 = raw[:8 * nb] if form == 0 else bytes(8 * nb)                                           # form 1: the excess proof, v = 0
            bl = b"".join(raw[8 * nb + 32 * i:8 * nb + 32 * i + 31] + b"\x00" for i in range(nb))     # below 2^248: canonical
            seeds = raw[40 * nb:72 * nb]
            coms, st = ctx.pedersen_commit_batch(v8, 8, bl)
            assert st == bytes(nb)
            # one bound transcript per proof, made on the GPU
            states, _ = ctx.transcript_batch(nb, [("append_u64", b"session", list(range(nb)))], label=b"opening rate")
            proofs, st, ends = ctx.opening_create_batch_ts(form, states, coms, v8, 8, bl, rng32=seeds, want_transcripts=True)
            assert st == bytes(nb)
            spoiled = bytearray(proofs)
            for i in range(0, nb, 64):
                spoiled[pl * i + pl - 7] ^= 4
            spoiled = bytes(spoiled)
            vals_arg = v8 if form == 0 else None                                                        # creation: form 1 without a buffer is v = 0
            # ---- the old route's buffers
            c_out, ts_out = C.create_string_buffer(32 * nb), C.create_string_buffer(TS * nb)
            msm_out, msm_st = C.create_string_buffer(32 * nb), C.create_string_buffer(nb)
            nt = (C.c_uint32 * nb)(*([4] * nb))

            def old_inputs(pr):
                Rs = b"".join(pr[pl * i:pl * i + 32] for i in range(nb))
                arr, nops, keep = script(ctx, nb, form, coms, bytes(32 * nb), Rs, c_out)
                chk(L.bpgpu_transcript_batch(ctx.h, nb, None, 0, states, TS, arr, nops, ts_out))
                sc, pt = [], []
                for i in range(nb):
                    c = int.from_bytes(c_out.raw[32 * i:32 * i + 32], "little")
                    s_v = pr[pl * i + 32:pl * i + 64] if form == 0 else bytes(32)                        # form 1: c v with v = 0
                    sc.append(s_v + pr[pl * i + pl - 32:pl * i + pl] + le32((L_ORDER - c) % L_ORDER) + le32(L_ORDER - 1))
                    pt.append(B + Bb + coms[32 * i:32 * i + 32] + Rs[32 * i:32 * i + 32])
                return (arr, nops, keep), b"".join(sc), b"".join(pt)

            def old_verdicts(pr):
                _, sc, pt = old_inputs(pr)
                chk(L.bpgpu_msm_batch(ctx.h, nb, nt, sc, pt, msm_out, msm_st))
                return bytes(0 if (msm_st.raw[i] == 0 and msm_out.raw[32 * i:32 * i + 32] == bytes(32)) else 1 for i in range(nb)), ts_out.raw
            # ---- the same verdicts and states first
            for pr in (proofs, spoiled):
                want_v, want_t = old_verdicts(pr)
                got = ctx.opening_verify_batch_ts(form, pr, pl, states, coms, None, 8, want_transcripts=True)
                comb = ctx.opening_verify_rlc_ts(form, pr, pl, states, coms, None, 8, want_transcripts=True)
                assert got[0] == comb[0] == want_v and got[1] == comb[3] == want_t == ends, (nb, form)
                assert want_v == (bytes(nb) if pr is proofs else bytes(1 if i % 64 == 0 else 0 for i in range(nb)))
            (arr, nops, keep), sc, pt = old_inputs(proofs)
            # the old creation: R through the commit call (k_v, k_r as value and blinding: 32-byte scalars), then the challenge
            k = hashlib.shake_256(tag + b"k").digest(64 * nb)
            kv = b"".join(k[64 * i:64 * i + 31] + b"\x00" for i in range(nb)) if form == 0 else bytes(32 * nb)
            kr = b"".join(k[64 * i + 32:64 * i + 63] + b"\x00" for i in range(nb))
            r_out, r_st = C.create_string_buffer(32 * nb), C.create_string_buffer(nb)
            r_keep = C.create_string_buffer(32 * nb)
            arr_c, nops_c, keep_c = script(ctx, nb, form, coms, bytes(32 * nb), bytes(32 * nb), c_out)

            def old_create():
                rc = L.bpgpu_pedersen_commit_batch(ctx.h, nb, kv, 32, kr, None, 0, r_out, None, r_st)
                C.memmove(keep_c[3], r_out, 32 * nb)                                                   # R into the script's message buffer
                return rc or L.bpgpu_transcript_batch(ctx.h, nb, None, 0, states, TS, arr_c, nops_c, ts_out)
            p_out, p_st, vd, bo = C.create_string_buffer(pl * nb), C.create_string_buffer(nb), C.create_string_buffer(nb), C.create_string_buffer(33)
            forms = {
                "new_create": lambda: L.bpgpu_opening_create_batch_ts(ctx.h, form, nb, states, TS, seeds, coms, vals_arg, 8, bl, p_out, p_st, ts_out),
                "new_verify": lambda: L.bpgpu_opening_verify_batch_ts(ctx.h, form, nb, proofs, pl, states, TS, coms, None, 8, vd, None, ts_out),
                "new_combined": lambda: L.bpgpu_opening_verify_rlc_ts(ctx.h, form, nb, proofs, pl, states, TS, coms, None, 8, None, vd, bo, ts_out),
                "old_verify": lambda: (L.bpgpu_transcript_batch(ctx.h, nb, None, 0, states, TS, arr, nops, ts_out)
                                       or L.bpgpu_msm_batch(ctx.h, nb, nt, sc, pt, msm_out, msm_st)),
                "old_create": old_create,
            }
            calls = {}
            for fname, f in forms.items():
                chk(f())                                                                                # (warm-up)
                t = time.perf_counter()
                chk(f())
                calls[fname] = max(1, min(400, int(0.05 / max(time.perf_counter() - t, 1e-6))))
            assert p_out.raw == proofs and vd.raw[:nb] == bytes(nb) and bo.raw[0] == 0
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
                row = {"proofs": nb, "form": form, "call": fname, "calls_per_sample": calls[fname], "median_ms": round(med[fname] * 1e3, 4),
                       "spread": round(spread[fname], 4), "proofs_per_s": round(nb / med[fname])}
                rows.append(row)
                print(json.dumps(row), flush=True)
            if nb == 4096:
                cond["form %d" % form] = {"new_combined_ms": round(med["new_combined"] * 1e3, 4), "spread_new": round(spread["new_combined"], 4),
                                          "old_verify_ms": round(med["old_verify"] * 1e3, 4), "spread_old": round(spread["old_verify"], 4),
                                          "old_over_new": round(med["old_verify"] / med["new_combined"], 2),
                                          "met": med["new_combined"] * (1 + spread["new_combined"]) < med["old_verify"] * (1 - spread["old_verify"])}
    ok = bool(cond) and all(v["met"] for v in cond.values())
    res = {"tool": "tools/opening_rate.py", "gens": [64, 1], "fixed_window_bits": ctx.get_option("fixed_window_bits"), "rounds": rounds, "rows": rows,
           "condition": {"proofs": 4096, **cond, "met": ok}}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["condition"]), flush=True)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
