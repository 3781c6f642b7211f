#!/usr/bin/env python3
"""Proofs per second of bpgpu_sigma_create_batch_ts / _verify_batch_ts / _verify_rlc_ts beside the route the library offered before, same
box, same process, one context with gens_create(8, 1), host pointers (every call ends in its own device synchronise), by the method of
tools/opening_rate.py:
  new_create   : the proofs of a batch (the products k P, the walks and encodings, the transcripts)
  new_verify   : every proof on its own (front end, the shared-generator chain with one row per (proof, equation), verdicts)
  new_combined : ONE combined check over nbatch (P + E) points
  old_verify   : bpgpu_transcript_batch running the protocol's script for c, then bpgpu_msm_batch on every equation's terms
                 (s[sec], Base) .., (l - c, slot[lhs]), (l - 1, T_k) and the identity test.  Only the two library calls are timed: the host
                 arithmetic between them (l - c per row) is prepared outside the samples, so the figure is a LOWER bound of the old route
  old_create   : bpgpu_msm_batch for T_k = sum k[sec] Base of every (row, equation), then bpgpu_transcript_batch for c; the host's S
                 multiply-adds per row are likewise not timed
for two relations -- R3, DLEQ: P0 = x B, P1 = x P2; R4, one amount under two value bases: P0 = v B + r1 B_blinding, P1 = v P2 + r2 B_blinding
-- at 64, 4 096 and 65 536 rows per call, one transcript state per row.  The C ABI is called through ctypes on buffers made once; the calls
are interleaved round by round; a sample is K back-to-back calls, K chosen so that it lasts about 50 ms; the figure is the median of the
rounds and `spread` is (max - min) / median.  Before anything is timed the old route's verdicts and end states are compared with the new
calls' (all valid, and with one proof in 64 spoiled), and the created proofs are verified.
CONDITION (exit status 1 when missed), for both relations: new_combined at 65 536 rows against old_verify, and new_create at 4 096 rows
against old_create, each faster by more than the run-to-run spread of the two medians:
median_new * (1 + spread_new) < median_old * (1 - spread_old).
    python tools/sigma_rate.py [--rounds N] [--sizes 64,4096,65536] [--out profiles/sigma_rate.json]"""
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
RELATIONS = {
    "R3": bytes([1, 3, 2, 16, 1, 0, 1, 17, 1, 0, 18]),
    "R4": bytes([3, 3, 2, 16, 2, 0, 1, 1, 0, 17, 2, 0, 18, 2, 0]),
}


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def le32(x):
    return int(x).to_bytes(32, "little")


def equations(desc):
    """[(lhs slot, [(secret, base id)])] of canonical descriptor bytes"""
    at, out = 3, []
    for _ in range(desc[2]):
        lhs, n = desc[at], desc[at + 1]
        out.append((lhs - 16, [(desc[at + 2 + 2 * t], desc[at + 3 + 2 * t]) for t in range(n)]))
        at += 2 + 2 * n
    return out


def main():
    rounds = arg("--rounds", 9)
    sizes = [int(x) for x in arg("--sizes", "64,4096,65536").split(",")]
    out_path = arg("--out", os.path.join(ROOT, "profiles", "sigma_rate.json"))
    L = bp.lib()
    ctx = bp.Context(0)
    ctx.gens_create(8, 1)
    _, _, B, Bb = ctx.gens_export()
    shared = {0: Bb, 1: B}
    chk = lambda rc: ctx._chk(rc)
    rows, cond = [], {}
    for name, desc in RELATIONS.items():
        h, S, P, E, digest = ctx.sigma_relation_create(desc)
        shape, eqs, pl = (S, P, E), equations(desc), 32 * (E + S)
        free = [p for p in range(P) if p not in {lhs for lhs, _ in eqs}]
        for nb in sizes:
            tag = b"sigma-rate-%s-%d" % (name.encode(), nb)
            raw = hashlib.shake_256(tag).digest(32 * nb * (S + len(free) + 1))
            sc31 = lambda i: raw[32 * i:32 * i + 31] + b"\x00"                                        # below 2^248: canonical
            xs = [[sc31(r * S + j) for j in range(S)] for r in range(nb)]
            seeds = raw[32 * nb * (S + len(free)):]
            # the instance: the free slots are multiples of B, the lhs slots follow from the equations in order
            pts = [[None] * P for _ in range(nb)]
            fr, st = ctx.msm_batch([1] * (nb * len(free)), b"".join(sc31(nb * S + r * len(free) + f) for r in range(nb) for f in range(len(free))), B * (nb * len(free)))
            assert st == bytes(nb * len(free))
            for r in range(nb):
                for f, p in enumerate(free):
                    pts[r][p] = fr[32 * (r * len(free) + f):32 * (r * len(free) + f) + 32]
            base = lambda r, b: pts[r][b - 16] if b >= 16 else shared[b]
            for lhs, terms in eqs:
                out, st = ctx.msm_batch([len(terms)] * nb, b"".join(xs[r][s] for r in range(nb) for s, _ in terms), b"".join(base(r, b) for r in range(nb) for _, b in terms))
                assert st == bytes(nb)
                for r in range(nb):
                    pts[r][lhs] = out[32 * r:32 * r + 32]
            points = b"".join(b"".join(row) for row in pts)
            secrets = b"".join(b"".join(row) for row in xs)
            states, _ = ctx.transcript_batch(nb, [("append_u64", b"session", list(range(nb)))], label=b"sigma rate")
            proofs, st, ends = ctx.sigma_create_batch_ts(h, shape, states, points, secrets, rng32=seeds, want_transcripts=True)
            assert st == bytes(nb)
            spoiled = bytearray(proofs)
            for i in range(0, nb, 64):
                spoiled[pl * i + pl - 7] ^= 4
            spoiled = bytes(spoiled)
            # ---- the old route's buffers: the script reads the points and the T_k where they lie
            c_out, ts_out = C.create_string_buffer(32 * nb), C.create_string_buffer(TS * nb)
            nrow = nb * E
            msm_out, msm_st = C.create_string_buffer(32 * nrow), C.create_string_buffer(nrow)
            nt = (C.c_uint32 * nrow)(*[len(terms) + 2 for _ in range(nb) for _, terms in eqs])
            nt_c = (C.c_uint32 * nrow)(*[len(terms) for _ in range(nb) for _, terms in eqs])

            def script(t_buf, t_stride):
                keep = [C.create_string_buffer(b"sigmaproof v1", 13), C.create_string_buffer(digest, 32), C.create_string_buffer(points, len(points)), t_buf]
                ops = [(_lib.TS_APPEND, b"dom-sep", C.addressof(keep[0]), 0, 13, None), (_lib.TS_APPEND, b"stmt", C.addressof(keep[1]), 0, 32, None)]
                ops += [(_lib.TS_APPEND, b"P", C.addressof(keep[2]) + 32 * u, 32 * P, 32, None) for u in range(P)]
                ops += [(_lib.TS_APPEND, b"T", C.addressof(t_buf) + 32 * k, t_stride, 32, None) for k in range(E)]
                ops.append((_lib.TS_CHALLENGE_SCALAR, b"c", C.addressof(c_out), 32, 0, None))
                arr, keep2 = ctx._ts_ops(ops)
                return arr, len(ops), keep + [keep2]

            def old_inputs(pr):
                pbuf = C.create_string_buffer(pr, len(pr))
                arr, nops, keep = script(pbuf, pl)
                chk(L.bpgpu_transcript_batch(ctx.h, nb, None, 0, states, TS, arr, nops, ts_out))
                sc, pt = [], []
                minus_one = le32(L_ORDER - 1)
                for r in range(nb):
                    c = int.from_bytes(c_out.raw[32 * r:32 * r + 32], "little")
                    mc = le32((L_ORDER - c) % L_ORDER)
                    for k, (lhs, terms) in enumerate(eqs):
                        sc.append(b"".join(pr[pl * r + 32 * (E + s):pl * r + 32 * (E + s) + 32] for s, _ in terms) + mc + minus_one)
                        pt.append(b"".join(base(r, b) for _, b in terms) + pts[r][lhs] + pr[pl * r + 32 * k:pl * r + 32 * k + 32])
                return (arr, nops, keep), b"".join(sc), b"".join(pt)

            def old_verdicts(pr):
                _, sc, pt = old_inputs(pr)
                chk(L.bpgpu_msm_batch(ctx.h, nrow, nt, sc, pt, msm_out, msm_st))
                ok = lambda j: msm_st.raw[j] == 0 and msm_out.raw[32 * j:32 * j + 32] == bytes(32)
                return bytes(0 if all(ok(r * E + k) for k in range(E)) else 1 for r in range(nb)), ts_out.raw
            # ---- the same verdicts and states first
            for pr in (proofs, spoiled):
                want_v, want_t = old_verdicts(pr)
                got = ctx.sigma_verify_batch_ts(h, shape, pr, states, points, want_transcripts=True)
                comb = ctx.sigma_verify_rlc_ts(h, shape, pr, states, points, want_transcripts=True)
                assert got[0] == comb[0] == want_v and got[1] == comb[3] == want_t == ends, (name, nb)
                assert want_v == (bytes(nb) if pr is proofs else bytes(1 if i % 64 == 0 else 0 for i in range(nb)))
            (arr, nops, keep), sc, pt = old_inputs(proofs)
            # the old creation: every T_k through the multiscalar multiplication (nonces as scalars), then the challenge
            kraw = hashlib.shake_256(tag + b"k").digest(32 * nb * S)
            ks = [[kraw[32 * (r * S + j):32 * (r * S + j) + 31] + b"\x00" for j in range(S)] for r in range(nb)]
            sc_c = b"".join(ks[r][s] for r in range(nb) for _, terms in eqs for s, _ in terms)
            pt_c = b"".join(base(r, b) for r in range(nb) for _, terms in eqs for _, b in terms)
            t_buf = C.create_string_buffer(32 * nrow)
            arr_c, nops_c, keep_c = script(t_buf, 32 * E)

            def old_create():
                return (L.bpgpu_msm_batch(ctx.h, nrow, nt_c, sc_c, pt_c, t_buf, msm_st)                  # T_k straight into the script's message buffer
                        or L.bpgpu_transcript_batch(ctx.h, nb, None, 0, states, TS, arr_c, nops_c, ts_out))
            p_out, p_st, vd, bo = C.create_string_buffer(pl * nb), C.create_string_buffer(nb), C.create_string_buffer(nb), C.create_string_buffer(33)
            forms = {
                "new_create": lambda: L.bpgpu_sigma_create_batch_ts(ctx.h, h, nb, states, TS, seeds, points, secrets, p_out, p_st, ts_out),
                "new_verify": lambda: L.bpgpu_sigma_verify_batch_ts(ctx.h, h, nb, proofs, pl, states, TS, points, vd, None, ts_out),
                "new_combined": lambda: L.bpgpu_sigma_verify_rlc_ts(ctx.h, h, nb, proofs, pl, states, TS, points, None, vd, bo, ts_out),
                "old_verify": lambda: (L.bpgpu_transcript_batch(ctx.h, nb, None, 0, states, TS, arr, nops, ts_out)
                                       or L.bpgpu_msm_batch(ctx.h, nrow, nt, sc, pt, msm_out, msm_st)),
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
                row = {"relation": name, "rows": nb, "call": fname, "calls_per_sample": calls[fname], "median_ms": round(med[fname] * 1e3, 4),
                       "spread": round(spread[fname], 4), "proofs_per_s": round(nb / med[fname])}
                rows.append(row)
                print(json.dumps(row), flush=True)
            for new, old, at in (("new_combined", "old_verify", 65536), ("new_create", "old_create", 4096)):
                if nb == at:
                    cond["%s %s at %d" % (name, new, at)] = {
                        "new_ms": round(med[new] * 1e3, 4), "spread_new": round(spread[new], 4), "old_ms": round(med[old] * 1e3, 4), "spread_old": round(spread[old], 4),
                        "old_over_new": round(med[old] / med[new], 2), "met": med[new] * (1 + spread[new]) < med[old] * (1 - spread[old])}
        ctx.sigma_relation_destroy(h)
    ok = bool(cond) and all(v["met"] for v in cond.values())
    res = {"tool": "tools/sigma_rate.py", "gens": [8, 1], "fixed_window_bits": ctx.get_option("fixed_window_bits"), "rounds": rounds, "rows": rows,
           "condition": {**cond, "met": ok}}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["condition"]), flush=True)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
