#!/usr/bin/env python3
"""What one transcript per proof costs: bpgpu_linear_verify_batch_ts and bpgpu_ipp_verify_rlc_ts with transcript_stride = 208 against the
existing shared-state calls they generalise (bpgpu_linear_verify_batch, bpgpu_ipp_verify_rlc with shared_transcript), in one process:
  4 096 proofs  x  n in {64, 1024}  x  generator-table mode (G = F = B = NULL resp. G = H = NULL, gens_m = 1)
The proofs are the reference's test shapes (oracle.linear_test_instance, oracle.ipp_test_instance), one instance tiled over the batch
(one public vector for all in the linear calls); the per-proof form gets the same start state 4 096 times, so both forms do the same
work except for the 208-byte load and the separator per proof.  Every call is blocking -- the host-pointer forms as they are, the
device-pointer forms followed by a stream synchronise -- and timed by a host clock; the forms alternate call by call, the turn starting
one form further each round, --iters (10) calls each; the median, the fastest and the slowest call are recorded, and every verdict is
checked.
    python tools/ipp_linear_ts_rate.py [--iters N] [--n 64,1024] [--nbatch 4096] [--out FILE]
    python tools/ipp_linear_ts_rate.py --baseline-lib PATH/libbpgpu.so ...
        also loads a build of another commit and takes its existing shared-state calls into the same alternation (same box, same
        process): is the existing call slower than it was?"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

TS = 208
LIN_LABEL, IPP_LABEL = b"linearprooftest", b"innerproducttest"


def interleaved(calls, iters):
    """calls: {name: function}; one warm-up round, then `iters` rounds of every call in turn, the turn starting one form further each round
    -> {name: (median, min, max) in ms}"""
    for f in calls.values():
        f()
    times = {name: [] for name in calls}
    order = list(calls.items())
    for r in range(iters):
        for name, f in order[r % len(order):] + order[:r % len(order)]:   # (rotated: no form always runs behind the same other one)
            t0 = time.perf_counter()
            f()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return {name: (round(statistics.median(t), 3), round(min(t), 3), round(max(t), 3)) for name, t in times.items()}


def load_baseline(path):
    """another build of the library with the argtypes of the calls timed here"""
    L = C.CDLL(path)
    vp, sz, u8p, i = C.c_void_p, C.c_size_t, C.c_char_p, C.c_int
    L.bpgpu_ctx_create.argtypes = [i, C.POINTER(vp)]
    L.bpgpu_ctx_destroy.argtypes = [vp]
    L.bpgpu_ctx_destroy.restype = None
    L.bpgpu_gens_create.argtypes = [vp, sz, sz]
    L.bpgpu_linear_verify_batch.argtypes = [vp, sz, sz, u8p, sz, u8p, sz, u8p, u8p, u8p, u8p, u8p, u8p, i, u8p, u8p, u8p]
    L.bpgpu_ipp_verify_rlc.argtypes = [vp, sz, sz, u8p, sz, u8p, sz, u8p, u8p, u8p, u8p, u8p, u8p, u8p, sz, u8p, u8p, u8p]
    L.bpgpu_linear_verify_batch_dev.argtypes = [vp, sz, sz, vp, sz, u8p, sz, u8p, vp, vp, vp, vp, vp, i, vp, vp, vp, vp]
    L.bpgpu_ipp_verify_rlc_dev.argtypes = [vp, sz, sz, vp, sz, u8p, sz, u8p, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp]
    return L


def run_shape(libs, n, nb, iters):
    """libs: [(tag, library, context handle)], the first one this build's.  Returns the two rows (linear, inner product) of the shape."""
    import pyoracle as O
    import torch
    dev = torch.device("cuda", 0)
    to_dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    lin, ipp = O.linear_test_instance(n, b"ts-rate-%d" % n), O.ipp_test_instance(n, IPP_LABEL, b"ts-rate-%d" % n)
    lin_st, ipp_st = O.transcript_new(LIN_LABEL), O.transcript_new(IPP_LABEL)
    lpl, ipl = len(lin["proof"]), len(ipp["proof"])
    lproofs, lC = lin["proof"] * nb, lin["C"] * nb
    iproofs, iGf, iHf, iP, iQ = ipp["proof"] * nb, ipp["Gf"] * nb, ipp["Hf"] * nb, ipp["P"] * nb, ipp["Q"] * nb
    weights = bytes(range(64)) * nb
    lin_states, ipp_states = lin_st * nb, ipp_st * nb
    verdict, bo = C.create_string_buffer(nb), C.create_string_buffer(33)
    d = dict(lp=to_dev(lproofs), lc=to_dev(lC), lb=to_dev(lin["b"]), lt=to_dev(lin_states), ip=to_dev(iproofs), igf=to_dev(iGf), ihf=to_dev(iHf), iP=to_dev(iP),
             iQ=to_dev(iQ), it=to_dev(ipp_states), w=to_dev(weights), v=torch.zeros(nb, dtype=torch.uint8, device=dev), bo=torch.zeros(64, dtype=torch.uint8, device=dev))
    stream = torch.cuda.Stream(device=dev)
    ok = lambda rc: rc == 0 or sys.exit("a call failed: rc = %d" % rc)

    def host_ok():
        assert verdict.raw == bytes(nb), "a proof did not verify"

    def dev_ok():
        stream.synchronize()

    L0, h0 = libs[0][1], libs[0][2]
    lin_calls, ipp_calls, lin_dev, ipp_dev = {}, {}, {}, {}
    lin_calls["ts_stride_208"] = lambda: (ok(L0.bpgpu_linear_verify_batch_ts(h0, n, nb, lproofs, lpl, lin_states, TS, lC, None, None, None, lin["b"], 1, verdict, None, None)),
                                         host_ok())
    ipp_calls["ts_stride_208"] = lambda: (ok(L0.bpgpu_ipp_verify_rlc_ts(h0, n, nb, iproofs, ipl, ipp_states, TS, iGf, iHf, iP, iQ, None, None, 1, weights, verdict, bo, None)),
                                         host_ok())
    lin_dev["ts_stride_208"] = lambda: (ok(L0.bpgpu_linear_verify_batch_ts_dev(h0, n, nb, d["lp"].data_ptr(), lpl, None, d["lt"].data_ptr(), d["lc"].data_ptr(), None, None,
                                                                               None, d["lb"].data_ptr(), 1, d["v"].data_ptr(), None, None, stream.cuda_stream)), dev_ok())
    ipp_dev["ts_stride_208"] = lambda: (ok(L0.bpgpu_ipp_verify_rlc_ts_dev(h0, n, nb, d["ip"].data_ptr(), ipl, None, d["it"].data_ptr(), d["igf"].data_ptr(),
                                                                          d["ihf"].data_ptr(), d["iP"].data_ptr(), d["iQ"].data_ptr(), None, None, 1, d["w"].data_ptr(),
                                                                          d["v"].data_ptr(), d["bo"].data_ptr(), None, stream.cuda_stream)), dev_ok())
    for tag, L, h in libs:
        name = "shared_state" if tag == "this" else "shared_state_" + tag
        lin_calls[name] = lambda L=L, h=h: (ok(L.bpgpu_linear_verify_batch(h, n, nb, lproofs, lpl, None, 0, lin_st, lC, None, None, None, lin["b"], 1, verdict, None, None)),
                                            host_ok())
        ipp_calls[name] = lambda L=L, h=h: (ok(L.bpgpu_ipp_verify_rlc(h, n, nb, iproofs, ipl, None, 0, ipp_st, iGf, iHf, iP, iQ, None, None, 1, weights, verdict, bo)),
                                            host_ok())
        lin_dev[name] = lambda L=L, h=h: (ok(L.bpgpu_linear_verify_batch_dev(h, n, nb, d["lp"].data_ptr(), lpl, None, 0, lin_st, d["lc"].data_ptr(), None, None, None,
                                                                             d["lb"].data_ptr(), 1, d["v"].data_ptr(), None, None, stream.cuda_stream)), dev_ok())
        ipp_dev[name] = lambda L=L, h=h: (ok(L.bpgpu_ipp_verify_rlc_dev(h, n, nb, d["ip"].data_ptr(), ipl, None, 0, ipp_st, d["igf"].data_ptr(), d["ihf"].data_ptr(),
                                                                        d["iP"].data_ptr(), d["iQ"].data_ptr(), None, None, 1, d["w"].data_ptr(), d["v"].data_ptr(),
                                                                        d["bo"].data_ptr(), stream.cuda_stream)), dev_ok())
    rows = []
    for call, form, calls in (("bpgpu_linear_verify_batch[_ts]", "host", lin_calls), ("bpgpu_linear_verify_batch[_ts]_dev", "dev", lin_dev),
                              ("bpgpu_ipp_verify_rlc[_ts]", "host", ipp_calls), ("bpgpu_ipp_verify_rlc[_ts]_dev", "dev", ipp_dev)):
        t = interleaved(calls, iters)
        if form == "dev":
            assert bytes(d["v"].cpu().numpy()) == bytes(nb), "a proof did not verify"
        row = {"call": call, "form": form, "n": n, "nbatch": nb, "bases": "table"}
        for name, (med, lo, hi) in t.items():
            row[name + "_ms"] = {"median": med, "min": lo, "max": hi, "spread_pct": round(100 * (hi - lo) / med, 1)}
        row["ts_over_shared"] = round(t["ts_stride_208"][0] / t["shared_state"][0], 4)
        for tag, _, _ in libs[1:]:
            row["shared_over_" + tag] = round(t["shared_state"][0] / t["shared_state_" + tag][0], 4)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    arg = lambda key, default: sys.argv[sys.argv.index(key) + 1] if key in sys.argv else default
    ints = lambda s: [int(x) for x in s.split(",")]
    iters, out_file, base = int(arg("--iters", "10")), arg("--out", None), arg("--baseline-lib", None)
    ns, nb = ints(arg("--n", "64,1024")), int(arg("--nbatch", "4096"))
    import bulletproofs_amd as bp
    ctx = bp.Context(0)
    ctx.gens_create(max(ns), 1)
    libs = [("this", bp.lib(), ctx.h)]
    if base:
        Lb = load_baseline(base)
        hb = C.c_void_p()
        assert Lb.bpgpu_ctx_create(0, C.byref(hb)) == 0 and Lb.bpgpu_gens_create(hb, max(ns), 1) == 0
        libs.append(("baseline", Lb, hb))
    doc = {"tool": "tools/ipp_linear_ts_rate.py", "iters": iters, "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP default 4)"),
           "baseline_lib": bool(base), "shapes": []}
    for n in ns:
        doc["shapes"] += run_shape(libs, n, nb, iters)
    if base:
        libs[1][1].bpgpu_ctx_destroy(libs[1][2])
    ctx.close()
    if out_file:
        json.dump(doc, open(out_file, "w"), indent=1)


if __name__ == "__main__":
    main()
