#!/usr/bin/env python3
"""Commitments per second of bpgpu_pedersen_commit_batch / bpgpu_pedersen_open_batch beside the two routes the library offered before,
same box, same process, one context with gens_create(64, 1), host pointers (every call ends in its own device synchronise):
  new_given   : u64 values, the caller's blindings            new_seeded : u64 values, blindings drawn on the device from one seed
  new_ct      : new_given with prover_constant_time = 1       new_open   : bpgpu_pedersen_open_batch on the commitments of new_given
  old_msm     : bpgpu_msm_batch, nbatch two-term MSMs (value, B), (blinding, B_blinding) -- what BulletproofGens.commit does per call
  old_shared  : bpgpu_msm_batch_shared(64, 1, nbatch, 0, ...): 130 generator scalars per row, all but two of them zero
at nbatch = 1, 64, 4 096, 262 144 (old_shared stops at 4 096: 262 144 rows would stage 1.09 GB of zeros).
The C ABI is called through ctypes on buffers made once, so a sample times the library, not Python's packing.  The forms are
interleaved round by round (drift hits them alike); a sample is K back-to-back calls, K chosen so that it lasts about 50 ms; the figure
is the median of the rounds and `spread` is (max - min) / median.  Before anything is timed the new call's rows are compared with
old_msm's at 4 096.
CONDITION (exit status 1 when missed): at 4 096 new_given is not slower than the better of old_msm and old_shared by more than 4 %.
    python tools/pedersen_rate.py [--rounds N] [--out profiles/pedersen_rate.json] [--lib path/to/libbpgpu.so]
--lib: a library built with another form of the kernel (-DBP_PED_SECOND_LINE), for a same-box comparison."""
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

from bulletproofs_amd import _lib  # noqa: E402

if "--lib" in sys.argv:
    _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
import bulletproofs_amd as bp  # noqa: E402

SIZES = (1, 64, 4096, 262144)
SHARED_MAX = 4096
TOLERANCE = 0.04      # the run-to-run spread the README records for this box


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    rounds = arg("--rounds", 9)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "pedersen_rate.json"))
    L = bp.lib()
    ctx, ctx_ct = bp.Context(0), bp.Context(0)
    ctx_ct.set_option("prover_constant_time", 1)
    for c in (ctx, ctx_ct):
        c.gens_create(64, 1)
    _, _, B, Bb = ctx.gens_export()
    nmax = max(SIZES)
    raw = hashlib.shake_256(b"pedersen-rate").digest(40 * nmax)
    v8 = raw[:8 * nmax]
    bl = b"".join(raw[8 * nmax + 32 * i:8 * nmax + 32 * i + 31] + b"\x00" for i in range(nmax))     # below 2^248: canonical
    seed = hashlib.shake_256(b"pedersen-rate-seed").digest(32)
    out, blo, st = C.create_string_buffer(32 * nmax), C.create_string_buffer(32 * nmax), C.create_string_buffer(nmax)
    coms = C.create_string_buffer(32 * nmax)
    chk = lambda rc: ctx._chk(rc)

    rows, at4096 = [], {}
    for nb in SIZES:
        # the old routes' inputs for this size
        sc2 = b"".join(v8[8 * i:8 * i + 8] + bytes(24) + bl[32 * i:32 * i + 32] for i in range(nb))
        pt2 = (B + Bb) * nb
        nt = (C.c_uint32 * nb)(*([2] * nb))
        gs = None
        if nb <= SHARED_MAX:
            gs = b"".join(bl[32 * i:32 * i + 32] + v8[8 * i:8 * i + 8] + bytes(24) + bytes(32 * 128) for i in range(nb))
        chk(L.bpgpu_pedersen_commit_batch(ctx.h, nb, v8, 8, bl, None, 0, coms, None, st))
        assert st.raw[:nb] == bytes(nb)
        forms = {
            "new_given": lambda: L.bpgpu_pedersen_commit_batch(ctx.h, nb, v8, 8, bl, None, 0, out, None, st),
            "new_seeded": lambda: L.bpgpu_pedersen_commit_batch(ctx.h, nb, v8, 8, None, seed, 0, out, blo, st),
            "new_ct": lambda: L.bpgpu_pedersen_commit_batch(ctx_ct.h, nb, v8, 8, bl, None, 0, out, None, st),
            "new_open": lambda: L.bpgpu_pedersen_open_batch(ctx.h, nb, coms, v8, 8, bl, st),
            "old_msm": lambda: L.bpgpu_msm_batch(ctx.h, nb, nt, sc2, pt2, out, st),
        }
        if gs is not None:
            forms["old_shared"] = lambda: L.bpgpu_msm_batch_shared(ctx.h, 64, 1, nb, 0, gs, None, None, out, st)
        # same bytes first (and the warm-up of every form at this size)
        for name, f in forms.items():
            chk(f())
            if name in ("new_given", "new_ct", "old_msm", "old_shared"):
                assert out.raw[:32 * nb] == coms.raw[:32 * nb] and st.raw[:nb] == bytes(nb), name
            elif name == "new_open":
                assert st.raw[:nb] == bytes(nb), name
        calls = {}
        for name, f in forms.items():
            t = time.perf_counter()
            chk(f())
            calls[name] = max(1, min(400, int(0.05 / max(time.perf_counter() - t, 1e-6))))
        samples = {name: [] for name in forms}
        for _ in range(rounds):
            for name, f in forms.items():
                t = time.perf_counter()
                for _ in range(calls[name]):
                    rc = f()
                samples[name].append((time.perf_counter() - t) / calls[name])
                chk(rc)
        for name, s in samples.items():
            med = statistics.median(s)
            row = {"nbatch": nb, "form": name, "calls_per_sample": calls[name], "median_ms": round(med * 1e3, 4), "spread": round((max(s) - min(s)) / med, 4),
                   "commitments_per_s": round(nb / med)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            if nb == 4096:
                at4096[name] = nb / med
    best_old = max(at4096["old_msm"], at4096["old_shared"])
    ok = at4096["new_given"] >= (1 - TOLERANCE) * best_old
    res = {"tool": "tools/pedersen_rate.py", "gens": [64, 1], "fixed_window_bits": ctx.get_option("fixed_window_bits"), "rounds": rounds,
           "library": os.path.relpath(_lib.LIB_PATH, ROOT), "rows": rows,
           "condition": {"nbatch": 4096, "new_given_per_s": round(at4096["new_given"]), "best_old_route": "old_msm" if at4096["old_msm"] >= at4096["old_shared"] else "old_shared",
                         "best_old_per_s": round(best_old), "new_over_best_old": round(at4096["new_given"] / best_old, 2), "tolerance": TOLERANCE, "met": ok}}
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
