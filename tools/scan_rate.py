#!/usr/bin/env python3
"""Rows per second of bpgpu_rangeproof_scan_batch (nkeys wallet keys, ONE transcript replay per row) beside the path it replaces on the
same proofs: nkeys passes of the seed derivation (bpgpu_transcript_batch[_dev], the script of RangeProof.rewind_seeds) +
bpgpu_rangeproof_rewind_batch[_dev].  n = 64, one state per row; rows 4 096 and 65 536; nkeys 1, 16, 256.
  scan_dev_none / scan_dev_all   : bpgpu_rangeproof_scan_batch_dev on device-resident buffers; no row is the wallet's / every row belongs
                                   to ONE of the keys (the last: every earlier candidate is tested and turned away)
  passes_dev_none / passes_dev_all : nkeys x (bpgpu_transcript_batch_dev + bpgpu_rangeproof_rewind_batch_dev), everything device-resident
  scan_host_* / passes_host_*    : the same through the host-pointer entry points (staging, copy back, the secrets cleared)
  rewind_dev_all                 : bpgpu_rangeproof_rewind_batch_dev alone with ready seeds -- what one key costs when the seeds are at hand
Method of tools/rewind_rate.py: every call is warmed up, then timed in interleaved rounds (one sample of each form per round, K calls
per sample and one synchronise for the _dev forms); the table gives medians and the spread (max - min) / median.  Before anything is
timed the scan's outputs are compared with what went into the proofs and with the passes' first-OK answer.
CONDITION (the tool exits 1 when it is not met): at nkeys = 16 and 256 the scan's _dev time is below the passes' _dev time by more than
the two spreads together, for both kinds of batch.  The ratio at nkeys = 1 against rewind_dev_all is recorded, not gated.
    python tools/scan_rate.py [--rounds N] [--sizes 4096,65536] [--keys 1,16,256] [--prove-max 4096] [--out profiles/scan_rate.json]"""
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
from bulletproofs_amd import _lib  # noqa: E402

TS, N = 208, 64
PL = 32 * (9 + 2 * 6)
LABEL = b"bpgpu rewind seed v1"
NONE = 0xFFFFFFFF


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    rounds = arg("--rounds", 7)
    sizes = [int(x) for x in arg("--sizes", "4096,65536").split(",")]
    nkeys_list = [int(x) for x in arg("--keys", "1,16,256").split(",")]
    prove_max = arg("--prove-max", 4096)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "scan_rate.json"))
    L = bp.lib()
    ctx = bp.Context(0)
    ctx.gens_create(64, 1)
    dev = torch.device("cuda:0")
    up = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)
    kmax = max(nkeys_list)
    all_keys = hashlib.shake_256(b"scan-rate-keys").digest(32 * kmax)
    strangers = hashlib.shake_256(b"scan-rate-strangers").digest(32 * kmax)
    rows, cond = [], {}
    ok = True
    for nb in sizes:
        raw = hashlib.shake_256(b"scan-rate-%d" % nb).digest(56 * nb)
        vals = [int.from_bytes(raw[8 * i:8 * i + 8], "little") for i in range(nb)]
        bl = b"".join(raw[8 * nb + 32 * i:8 * nb + 32 * i + 31] + b"\x00" for i in range(nb))     # below 2^248: canonical
        msgs = raw[40 * nb:56 * nb]
        states, _ = ctx.transcript_batch(nb, [("append_u64", b"session", list(range(nb)))], label=b"scan rate")
        coms = ctx.pedersen_commit_batch(b"".join(v.to_bytes(8, "little") for v in vals), 8, bl)[0]
        com_list = [coms[32 * i:32 * i + 32] for i in range(nb)]
        for nk in nkeys_list:
            keys = all_keys[:32 * nk]
            owner = keys[32 * (nk - 1):]                                                           # every row belongs to the LAST key
            seeds = bp.RangeProof.rewind_seeds(ctx, owner, com_list)
            proofs = b""
            for lo in range(0, nb, prove_max):                                                     # (the prover's working set bounds its batch)
                hi = min(nb, lo + prove_max)
                p, c = ctx.rangeproof_prove_batch_rw(N, 1, vals[lo:hi], bl[32 * lo:32 * hi], states[TS * lo:TS * hi], seeds[32 * lo:32 * hi], msgs[16 * lo:16 * hi])
                assert c == coms[32 * lo:32 * hi]
                proofs += p
            none_keys = strangers[:32 * nk]
            # ---- the same answers first
            st, ki, v, m, g = ctx.rangeproof_scan_batch(N, proofs, PL, coms, states, keys)
            assert st == bytes(nb) and ki == [nk - 1] * nb and v == vals and m == msgs and g == bl, (nb, nk)
            st, ki, v, m, g = ctx.rangeproof_scan_batch(N, proofs, PL, coms, states, none_keys)
            assert st == bytes([1]) * nb and ki == [NONE] * nb and not any(v) and m == bytes(16 * nb) and g == bytes(32 * nb), (nb, nk)
            st, v, m, g = ctx.rangeproof_rewind_batch(N, proofs, PL, coms, states, seeds)
            assert st == bytes(nb) and v == vals and m == msgs and g == bl
            # ---- device-resident buffers
            d_pr, d_cm, d_ts, d_keys, d_none, d_ready = up(proofs), up(coms), up(states), up(keys), up(none_keys), up(seeds)
            d_st, d_m, d_g, d_seed = (torch.zeros((k * nb,), dtype=torch.uint8, device=dev) for k in (1, 16, 32, 32))
            d_v = torch.zeros((nb,), dtype=torch.int64, device=dev)
            d_ki = torch.zeros((nb,), dtype=torch.int32, device=dev)
            d_tso = torch.zeros((TS * nb,), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()

            def scan_dev(d_k):
                return lambda: L.bpgpu_rangeproof_scan_batch_dev(ctx.h, N, nb, d_pr.data_ptr(), PL, d_cm.data_ptr(), d_ts.data_ptr(), TS, d_k.data_ptr(), nk,
                                                                 d_st.data_ptr(), d_ki.data_ptr(), d_v.data_ptr(), d_m.data_ptr(), d_g.data_ptr(), None)

            keep = []

            def passes_dev(d_k):
                scripts = []
                for j in range(nk):
                    arr, kp = ctx._ts_ops([(_lib.TS_APPEND, b"key", d_k.data_ptr() + 32 * j, 0, 32, None), (_lib.TS_APPEND, b"C", d_cm.data_ptr(), 32, 32, None),
                                           (_lib.TS_CHALLENGE, b"seed", d_seed.data_ptr(), 32, 32, None)])
                    keep.append(kp)
                    scripts.append(arr)

                def run():
                    rc = 0
                    for arr in scripts:
                        rc = rc or L.bpgpu_transcript_batch_dev(ctx.h, nb, LABEL, len(LABEL), None, 0, arr, 3, d_tso.data_ptr(), None)
                        rc = rc or L.bpgpu_rangeproof_rewind_batch_dev(ctx.h, N, nb, d_pr.data_ptr(), PL, d_cm.data_ptr(), d_ts.data_ptr(), TS, d_seed.data_ptr(),
                                                                       d_st.data_ptr(), d_v.data_ptr(), d_m.data_ptr(), d_g.data_ptr(), None)
                    return rc
                return run

            st_o, v_o, m_o, g_o = C.create_string_buffer(nb), (C.c_uint64 * nb)(), C.create_string_buffer(16 * nb), C.create_string_buffer(32 * nb)
            ki_o, seed_o, ts_o = (C.c_uint32 * nb)(), C.create_string_buffer(32 * nb), C.create_string_buffer(TS * nb)

            def passes_host(kb):
                scripts = []
                kbuf = C.create_string_buffer(kb, len(kb))
                cbuf = C.create_string_buffer(coms, len(coms))
                keep.extend([kbuf, cbuf])
                for j in range(nk):
                    arr, kp = ctx._ts_ops([(_lib.TS_APPEND, b"key", C.addressof(kbuf) + 32 * j, 0, 32, None), (_lib.TS_APPEND, b"C", C.addressof(cbuf), 32, 32, None),
                                           (_lib.TS_CHALLENGE, b"seed", C.addressof(seed_o), 32, 32, None)])
                    keep.append(kp)
                    scripts.append(arr)

                def run():
                    rc = 0
                    for arr in scripts:
                        rc = rc or L.bpgpu_transcript_batch(ctx.h, nb, LABEL, len(LABEL), None, 0, arr, 3, ts_o)
                        rc = rc or L.bpgpu_rangeproof_rewind_batch(ctx.h, N, nb, proofs, PL, coms, states, TS, seed_o, st_o, v_o, m_o, g_o)
                    return rc
                return run

            forms = {
                "scan_dev_none": scan_dev(d_none), "scan_dev_all": scan_dev(d_keys),
                "passes_dev_none": passes_dev(d_none), "passes_dev_all": passes_dev(d_keys),
                "rewind_dev_all": lambda: L.bpgpu_rangeproof_rewind_batch_dev(ctx.h, N, nb, d_pr.data_ptr(), PL, d_cm.data_ptr(), d_ts.data_ptr(), TS, d_ready.data_ptr(),
                                                                              d_st.data_ptr(), d_v.data_ptr(), d_m.data_ptr(), d_g.data_ptr(), None),
                "scan_host_none": lambda: L.bpgpu_rangeproof_scan_batch(ctx.h, N, nb, proofs, PL, coms, states, TS, none_keys, nk, st_o, ki_o, v_o, m_o, g_o),
                "scan_host_all": lambda: L.bpgpu_rangeproof_scan_batch(ctx.h, N, nb, proofs, PL, coms, states, TS, keys, nk, st_o, ki_o, v_o, m_o, g_o),
                "passes_host_none": passes_host(none_keys), "passes_host_all": passes_host(keys),
            }
            if nb * nk > 65536 * 16:                                                               # (the host passes at 256 keys: minutes of staging, nothing new)
                del forms["passes_host_none"], forms["passes_host_all"]
            sync = {f: (ctx.synchronize if "_dev_" in f else (lambda: None)) for f in forms}
            # the passes leave the LAST key's answer in the buffers: with every row the last key's, that is the scan's answer
            ctx._chk(forms["passes_dev_all"]())
            ctx.synchronize()
            assert bytes(d_st.cpu().numpy()) == bytes(nb) and bytes(d_g.cpu().numpy()) == bl
            ctx._chk(forms["scan_dev_all"]())
            ctx.synchronize()
            assert bytes(d_st.cpu().numpy()) == bytes(nb) and bytes(d_g.cpu().numpy()) == bl and d_ki.cpu().tolist() == [nk - 1] * nb
            calls = {}
            for fname, f in forms.items():
                ctx._chk(f())                                                                      # (warm-up)
                sync[fname]()
                t = time.perf_counter()
                ctx._chk(f())
                sync[fname]()
                calls[fname] = max(1, min(200, int(0.05 / max(time.perf_counter() - t, 1e-6))))
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
                row = {"rows": nb, "nkeys": nk, "call": fname, "calls_per_sample": calls[fname], "median_ms": round(med[fname] * 1e3, 4), "spread": round(spread[fname], 4),
                       "candidates_per_s": round(nb * nk / med[fname])}
                rows.append(row)
                print(json.dumps(row), flush=True)
            beyond = lambda a, b: med[a] * (1 + spread[a]) < med[b] * (1 - spread[b])
            c = {"scan_faster_than_passes_dev_none": beyond("scan_dev_none", "passes_dev_none"), "scan_faster_than_passes_dev_all": beyond("scan_dev_all", "passes_dev_all"),
                 "passes_over_scan_dev_none": round(med["passes_dev_none"] / med["scan_dev_none"], 2),
                 "passes_over_scan_dev_all": round(med["passes_dev_all"] / med["scan_dev_all"], 2),
                 "scan_over_rewind_ready_seeds_dev_all": round(med["scan_dev_all"] / med["rewind_dev_all"], 2)}
            if "passes_host_all" in forms:
                c["passes_over_scan_host_none"] = round(med["passes_host_none"] / med["scan_host_none"], 2)
                c["passes_over_scan_host_all"] = round(med["passes_host_all"] / med["scan_host_all"], 2)
            cond["%d x %d" % (nb, nk)] = c
            if nk > 1:
                ok = ok and c["scan_faster_than_passes_dev_none"] and c["scan_faster_than_passes_dev_all"]
            del keep[:]
    res = {"tool": "tools/scan_rate.py", "gens": [64, 1], "n": N, "fixed_window_bits": ctx.get_option("fixed_window_bits"), "rounds": rounds, "prove_max": prove_max,
           "rows": rows, "conditions": {**cond, "met": ok}}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["conditions"]), flush=True)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
