#!/usr/bin/env python3
"""Batch-combined InnerProductProof verification (bpgpu_ipp_verify_rlc_dev) against the per-proof path (bpgpu_ipp_verify_batch_dev with
bases_shared = 1, the yardstick: unchanged by the combined entry point), both on the same device-resident valid batch:
  n in {64, 256, 1024}  x  bases in {explicit (the caller's G, H), table (the context's generators)}  x  nbatch in {64, 1024, 4096}
Proofs are the reference's test shape (oracle.ipp_test_instance, whose bases are the context's G(n, 1), H(n, 1)), a few distinct ones per n
tiled over the batch; the per-proof path always gets the encodings (it has no generator-table mode), the combined path the same weights64
each time.  Each call is timed by a host clock around the call and a stream
synchronise, the two paths alternating; every verdict is checked.  One more pair of calls per shape has a single bad proof: what a
caller of the _dev form pays then (the combined call, then the per-proof call it falls back to).
    python tools/ipp_rlc_rate.py [--iters N] [--n 64,256,1024] [--nbatch 64,1024,4096] [--modes explicit,table] [--out FILE]
    python tools/ipp_rlc_rate.py --one N NBATCH MODE [--iters K]      the combined path alone, for a profiled run:
        rocprofv3 --kernel-trace --stats -d DIR/n<N>_nb<NBATCH>_<MODE> -o t --output-format csv -- python tools/ipp_rlc_rate.py --one ...
    python tools/ipp_rlc_rate.py --split DIR --out FILE      the kernel time of the LAST combined call of every trace under DIR
        (k_ipp_vs_front / k_ipp_rlc_uniq / k_ipp_rlc_weigh / the combination's other launches / the multiscalar multiplication), merged
        into FILE"""
import csv
import glob
import hashlib
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

DISTINCT = 4
LABEL = b"innerproducttest"
UNDECIDED = 5


def instances(ns):
    import pyoracle as O
    return {n: [O.ipp_test_instance(n, LABEL, b"ipp-rlc-rate-%d-%d" % (n, j)) for j in range(DISTINCT)] for n in ns}


class Batch:
    """one shape on the device: nbatch proofs tiled from the distinct instances, and the same batch with proof 1 tampered"""

    def __init__(self, insts, n, nbatch, fixed):
        import torch
        dev = torch.device("cuda", 0)
        to_dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
        tile = lambda key: b"".join(insts[j % DISTINCT][key] for j in range(nbatch))
        g0 = insts[0]
        self.n, self.nbatch, self.fixed, self.label, self.pl = n, nbatch, fixed, LABEL, len(g0["proof"])
        proofs = tile("proof")
        bad = bytearray(proofs)
        bad[self.pl * (1 % nbatch) + self.pl - 40] ^= 1                       # a tampered
        self.bad_at = 1 % nbatch
        self.d_proofs, self.d_bad = to_dev(proofs), to_dev(bytes(bad))
        self.d_Gf, self.d_Hf, self.d_P, self.d_Q = (to_dev(tile(k)) for k in ("Gf", "Hf", "P", "Q"))
        self.d_G, self.d_H = to_dev(g0["G"]), to_dev(g0["H"])
        self.d_w = to_dev(hashlib.shake_256(b"ipp-rlc-rate-w").digest(64 * nbatch))
        self.d_v = torch.full((nbatch,), 255, dtype=torch.uint8, device=dev)
        self.d_bo = torch.full((64,), 255, dtype=torch.uint8, device=dev)
        self.stream = torch.cuda.Stream(device=dev)

    def per_proof(self, ctx, L, bad=False):
        pr = (self.d_bad if bad else self.d_proofs).data_ptr()
        rc = L.bpgpu_ipp_verify_batch_dev(ctx.h, self.n, self.nbatch, pr, self.pl, self.label, len(self.label), None, self.d_Gf.data_ptr(),
                                          self.d_Hf.data_ptr(), self.d_P.data_ptr(), self.d_Q.data_ptr(), self.d_G.data_ptr(), self.d_H.data_ptr(), 1,
                                          self.d_v.data_ptr(), None, self.stream.cuda_stream)
        self.stream.synchronize()
        assert rc == 0, L.bpgpu_last_error(ctx.h)

    def combined(self, ctx, L, bad=False):
        pr = (self.d_bad if bad else self.d_proofs).data_ptr()
        g, h = (None, None) if self.fixed else (self.d_G.data_ptr(), self.d_H.data_ptr())
        rc = L.bpgpu_ipp_verify_rlc_dev(ctx.h, self.n, self.nbatch, pr, self.pl, self.label, len(self.label), None, self.d_Gf.data_ptr(),
                                        self.d_Hf.data_ptr(), self.d_P.data_ptr(), self.d_Q.data_ptr(), g, h, 1, self.d_w.data_ptr(), self.d_v.data_ptr(),
                                        self.d_bo.data_ptr(), self.stream.cuda_stream)
        self.stream.synchronize()
        assert rc == 0, L.bpgpu_last_error(ctx.h)

    def verdicts(self):
        return bytes(self.d_v.cpu().numpy()), bytes(self.d_bo.cpu().numpy())[:33]


def timed_pair(fa, fb, iters):
    """medians of two calls, alternating (other work shares the machine)"""
    fa()
    fb()
    ta, tb = [], []
    for _ in range(iters):
        t0 = time.perf_counter()
        fa()
        t1 = time.perf_counter()
        fb()
        t2 = time.perf_counter()
        ta.append(t1 - t0)
        tb.append(t2 - t1)
    return statistics.median(ta), statistics.median(tb)


def context_for(bp, ns, modes):
    """the context, and the largest n its generator tables serve (0: none)"""
    ctx = bp.Context(0)
    cap = 0
    if "table" in modes:
        for want in sorted(set(ns), reverse=True):
            try:
                ctx.gens_create(want, 1)
                cap = want
                break
            except bp.BpgpuError as e:
                print(json.dumps({"gens_create": [want, 1], "refused": str(e)}), flush=True)
    return ctx, cap


def run_shape(ctx, L, insts, n, nbatch, mode, iters):
    b = Batch(insts[n], n, nbatch, mode == "table")
    b.per_proof(ctx, L)
    assert b.verdicts()[0] == bytes(nbatch)
    b.combined(ctx, L)
    assert b.verdicts() == (bytes(nbatch), bytes(33))
    want_bad = bytes(1 if j == b.bad_at else 0 for j in range(nbatch))
    b.per_proof(ctx, L, bad=True)
    assert b.verdicts()[0] == want_bad
    b.combined(ctx, L, bad=True)
    v, bo = b.verdicts()
    assert v == bytes([UNDECIDED]) * nbatch and bo[0] == 1 and bo[1:] != bytes(32)
    t_p, t_c = timed_pair(lambda: b.per_proof(ctx, L), lambda: b.combined(ctx, L), iters)

    def fallback():
        b.combined(ctx, L, bad=True)
        b.per_proof(ctx, L, bad=True)
    t_pb, t_fb = timed_pair(lambda: b.per_proof(ctx, L, bad=True), fallback, max(2, iters // 2))
    return {"n": n, "nbatch": nbatch, "bases": mode, "per_proof_ms": round(t_p * 1e3, 3), "combined_ms": round(t_c * 1e3, 3),
            "per_proof_proofs_per_s": round(nbatch / t_p, 1), "combined_proofs_per_s": round(nbatch / t_c, 1), "speedup": round(t_p / t_c, 3),
            "one_bad_per_proof_ms": round(t_pb * 1e3, 3), "one_bad_combined_then_per_proof_ms": round(t_fb * 1e3, 3)}


def split_of(trace_csv):
    """kernel time (us) of the last combined call in a kernel trace: from its k_ipp_vs_front dispatch to the end of the trace"""
    rows = []
    with open(trace_csv) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0].replace("void ", "")))
    rows.sort()
    last = max(i for i, r in enumerate(rows) if "k_ipp_vs_front" in r[2])
    call = rows[last:]
    out = {"front_us": 0.0, "uniq_us": 0.0, "weigh_us": 0.0, "rho_reduce_verdict_us": 0.0, "msm_us": 0.0, "runtime_fill_copy_us": 0.0}
    for s, e, name in call:
        key = ("front_us" if "k_ipp_vs_front" in name else "uniq_us" if "k_ipp_rlc_uniq" in name else "weigh_us" if "k_ipp_rlc_weigh" in name else
               "rho_reduce_verdict_us" if "k_ipp_rlc_" in name or "k_rlc_comb_" in name else "msm_us" if re.match(r"k_\w+", name) else "runtime_fill_copy_us")
        out[key] += (e - s) / 1e3
    out = {k: round(v, 1) for k, v in out.items()}
    out["launches"] = len(call)
    out["other_kernels"] = sorted({name for _, _, name in call if "k_ipp_" not in name and "k_rlc_comb_" not in name})
    out["span_us"] = round((call[-1][1] - call[0][0]) / 1e3, 1)
    return out


def main():
    arg = lambda key, default: sys.argv[sys.argv.index(key) + 1] if key in sys.argv else default
    ints = lambda s: [int(x) for x in s.split(",")]
    iters, out_file = int(arg("--iters", "10")), arg("--out", None)
    if "--split" in sys.argv:
        doc = json.load(open(out_file)) if out_file and os.path.exists(out_file) else {"shapes": []}
        for d in sorted(glob.glob(os.path.join(arg("--split", "."), "n*_nb*_*"))):
            m = re.match(r"n(\d+)_nb(\d+)_(\w+)$", os.path.basename(d))
            traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
            if not m or not traces:
                continue
            sp = split_of(traces[0])
            key = (int(m.group(1)), int(m.group(2)), m.group(3))
            hit = [s for s in doc["shapes"] if (s["n"], s["nbatch"], s["bases"]) == key]
            if hit:
                hit[0]["combined_kernel_split"] = sp
            else:
                doc["shapes"].append({"n": key[0], "nbatch": key[1], "bases": key[2], "combined_kernel_split": sp})
            print(json.dumps({"shape": key, "combined_kernel_split": sp}), flush=True)
        if out_file:
            json.dump(doc, open(out_file, "w"), indent=1)
        return
    one = None
    if "--one" in sys.argv:
        i = sys.argv.index("--one")
        one = (int(sys.argv[i + 1]), int(sys.argv[i + 2]), sys.argv[i + 3])
    ns, nbs, modes = ints(arg("--n", "64,256,1024")), ints(arg("--nbatch", "64,1024,4096")), arg("--modes", "explicit,table").split(",")
    if one:
        ns, nbs, modes = [one[0]], [one[1]], [one[2]]
    insts = instances(ns)
    import bulletproofs_amd as bp
    L = bp.lib()
    ctx, cap = context_for(bp, ns, modes)
    if one:
        n, nbatch, mode = one
        if mode == "table" and n > cap:
            raise SystemExit("no generator tables for n = %d" % n)
        b = Batch(insts[n], n, nbatch, mode == "table")
        for _ in range(1 + iters):
            b.combined(ctx, L)
        assert b.verdicts() == (bytes(nbatch), bytes(33))
        ctx.close()
        return
    doc = {"tool": "tools/ipp_rlc_rate.py", "iters": iters, "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP default 4)"),
           "table_capacity": cap, "shapes": []}
    for n in ns:
        for mode in modes:
            for nbatch in nbs:
                if mode == "table" and n > cap:
                    row = {"n": n, "nbatch": nbatch, "bases": mode, "not_measured": "gens_create(%d, 1) was refused" % n}
                else:
                    row = run_shape(ctx, L, insts, n, nbatch, mode, iters if n * nbatch < (1 << 20) else max(3, iters // 2))
                doc["shapes"].append(row)
                print(json.dumps(row), flush=True)
    ctx.close()
    if out_file:
        json.dump(doc, open(out_file, "w"), indent=1)


if __name__ == "__main__":
    main()
