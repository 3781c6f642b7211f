#!/usr/bin/env python3
"""What it costs to make nbatch bound Merlin states, three ways, for two scripts:
  binding   : Transcript::new("payment-protocol v3") + a 32-byte session id per row (the README binding)
  binding+  : that, one 16-byte challenge, and a 40-byte append per row
  host      : bpgpu_transcript_batch, host pointers in, host states out (staging, kernel, copy back, the staging cleared)
  dev       : bpgpu_transcript_batch_dev on session ids that already sit in device memory, states left there; host clock around the call and
              the synchronise behind it
  loop      : what the library offered before: ONE host thread calling bpgpu_transcript_append_message / _challenge_bytes per row (from C, so
              that no interpreter is timed; Transcript::new computed once and copied, as a careful caller would), then the copy of 208 bytes
              per state to the device (pinned source), timed separately
for nbatch = 1 Ki, 64 Ki and 1 Mi.  One process, one context; the three alternate, 10 calls each after one warm-up each; medians.  The
three ways' states are compared byte for byte at every size.  Writes profiles/transcript_batch_rate.json and prints one JSON line per row.
Measured on one MI355X (profiles/transcript_batch_rate.json): at 64 Ki rows the _dev form takes 0.047 ms (binding) and 0.093 ms (binding+),
the host form 1.10 and 1.47 ms, the loop plus copy 2.40 and 50.0 ms; at 1 Mi rows 0.222 / 0.460 ms, 17.1 / 22.0 ms and 38.5 / 798 ms.
    python tools/transcript_batch_rate.py [--iters N] [--only NB]"""
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bulletproofs_amd as bp  # noqa: E402
from bulletproofs_amd import _lib  # noqa: E402

TS = 208
LOOP_SRC = r"""
#include <cstring>
#include "bpgpu.h"
// the per-row loop of the three host helpers; returns non-zero if one of them fails
extern "C" int loop_rows(size_t nbatch, int plus, const uint8_t *ids, const uint8_t *ctx40, uint8_t *states, uint8_t *chal16) {
    uint8_t st0[BPGPU_TRANSCRIPT_BYTES];
    int bad = bpgpu_transcript_new((const uint8_t *)"payment-protocol v3", 19, st0);
    for (size_t r = 0; r < nbatch; r++) {
        uint8_t *st = states + r * BPGPU_TRANSCRIPT_BYTES;
        memcpy(st, st0, BPGPU_TRANSCRIPT_BYTES);
        bad |= bpgpu_transcript_append_message(st, (const uint8_t *)"session", 7, ids + 32 * r, 32);
        if (plus) {
            bad |= bpgpu_transcript_challenge_bytes(st, (const uint8_t *)"binding", 7, chal16 + 16 * r, 16);
            bad |= bpgpu_transcript_append_message(st, (const uint8_t *)"context", 7, ctx40 + 40 * r, 40);
        }
    }
    return bad;
}
"""


def build_loop(tmp):
    src, so = os.path.join(tmp, "loop.cpp"), os.path.join(tmp, "libloop.so")
    open(src, "w").write(LOOP_SRC)
    csrc = os.path.join(ROOT, "bulletproofs_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), src, "-L", csrc, "-lbpgpu",
                           "-Wl,-rpath," + csrc, "-o", so])
    lib = C.CDLL(so)
    lib.loop_rows.argtypes = [C.c_size_t, C.c_int, C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p]
    return lib


def measure(ctx, loop, nb, plus, iters):
    import torch
    L = ctx._L
    dev = torch.device("cuda:0")
    ids = hashlib.shake_256(b"rate-ids").digest(32 * nb)
    ctx40 = hashlib.shake_256(b"rate-ctx").digest(40 * nb)
    d_ids = torch.frombuffer(bytearray(ids), dtype=torch.uint8).to(dev)
    d_ctx = torch.frombuffer(bytearray(ctx40), dtype=torch.uint8).to(dev)
    d_chal = torch.zeros(16 * nb, dtype=torch.uint8, device=dev)
    d_states = torch.zeros(TS * nb, dtype=torch.uint8, device=dev)
    d_copy = torch.zeros(TS * nb, dtype=torch.uint8, device=dev)
    h_ids, h_ctx, h_chal = C.create_string_buffer(ids, len(ids)), C.create_string_buffer(ctx40, len(ctx40)), C.create_string_buffer(16 * nb)
    h_states = C.create_string_buffer(TS * nb)
    pinned = torch.zeros(TS * nb, dtype=torch.uint8).pin_memory()
    h_chal_loop = C.create_string_buffer(16 * nb)

    def ops(p_ids, p_chal, p_ctx):
        raw = [(_lib.TS_APPEND, b"session", p_ids, 32, 32, None)]
        if plus:
            raw += [(_lib.TS_CHALLENGE, b"binding", p_chal, 16, 16, None), (_lib.TS_APPEND, b"context", p_ctx, 40, 40, None)]
        return ctx._ts_ops(raw)
    host_ops, keep1 = ops(C.addressof(h_ids), C.addressof(h_chal), C.addressof(h_ctx))
    dev_ops, keep2 = ops(d_ids.data_ptr(), d_chal.data_ptr(), d_ctx.data_ptr())
    label = b"payment-protocol v3"
    times = {"host": [], "dev": [], "loop": [], "copy": []}
    torch.cuda.synchronize()
    for it in range(iters + 1):                 # (round 0 warms up: staging buffers, the code object)
        t0 = time.perf_counter()
        rc = L.bpgpu_transcript_batch(ctx.h, nb, label, len(label), None, 0, host_ops, 3 if plus else 1, h_states)
        t1 = time.perf_counter()
        assert rc == 0
        rc = L.bpgpu_transcript_batch_dev(ctx.h, nb, label, len(label), None, 0, dev_ops, 3 if plus else 1, d_states.data_ptr(), None)
        ctx.synchronize()
        t2 = time.perf_counter()
        assert rc == 0
        rc = loop.loop_rows(nb, plus, ids, ctx40, pinned.data_ptr(), C.addressof(h_chal_loop))
        t3 = time.perf_counter()
        assert rc == 0
        d_copy.copy_(pinned, non_blocking=True)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        if it:
            for name, dt in (("host", t1 - t0), ("dev", t2 - t1), ("loop", t3 - t2), ("copy", t4 - t3)):
                times[name].append(dt)
    want = bytes(pinned.numpy())
    assert h_states.raw == want and bytes(d_states.cpu().numpy()) == want and bytes(d_copy.cpu().numpy()) == want
    if plus:
        assert h_chal.raw == h_chal_loop.raw == bytes(d_chal.cpu().numpy())
    med = {name: statistics.median(ts) * 1e3 for name, ts in times.items()}
    row = {"script": "binding+" if plus else "binding", "nbatch": nb, "iters": iters,
           "host_ms": round(med["host"], 3), "dev_ms": round(med["dev"], 3), "loop_ms": round(med["loop"], 3), "copy_ms": round(med["copy"], 3),
           "host_states_per_s": round(nb / med["host"] * 1e3), "dev_states_per_s": round(nb / med["dev"] * 1e3),
           "loop_plus_copy_states_per_s": round(nb / (med["loop"] + med["copy"]) * 1e3),
           "dev_min_ms": round(min(times["dev"]) * 1e3, 3), "dev_max_ms": round(max(times["dev"]) * 1e3, 3)}
    return row


def main():
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 10
    sizes = [int(sys.argv[sys.argv.index("--only") + 1])] if "--only" in sys.argv else [1 << 10, 1 << 16, 1 << 20]
    ctx = bp.Context(0)      # no generators: the transcript batch needs none
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        loop = build_loop(tmp)
        for plus in (0, 1):
            for nb in sizes:
                row = measure(ctx, loop, nb, plus, iters)
                rows.append(row)
                print(json.dumps(row), flush=True)
    ctx.close()
    if "--only" not in sys.argv:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "transcript_batch_rate.json"), "w") as f:
            json.dump({"tool": "tools/transcript_batch_rate.py", "clock": "host clock around the call (dev: and the synchronise behind it), medians", "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
