"""bpgpu_rangeproof_prove_batch_rw / _rewind_batch and their _dev forms at the ABI, without a GPU: the four symbols as include/bpgpu.h
declares them, the status constants, the Rust declarations tools/gen_rust_extern.py derives, the Python bindings' argument lists, the
mirror in bulletproofs.hpp, what the header says rewinding is not, and the argument check that needs no context.  (m != 1, a bad
proof_len and a bad stride are refused before anything is staged, but the refusal carries the context's error text:
tests/test_gpu_rewind.py makes those calls on a real context.)"""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1
NAMES = ["bpgpu_rangeproof_prove_batch_rw", "bpgpu_rangeproof_prove_batch_rw_dev", "bpgpu_rangeproof_rewind_batch", "bpgpu_rangeproof_rewind_batch_dev"]


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    import bulletproofs_amd as bp
    return bp


def _header():
    return open(os.path.join(ROOT, "include", "bpgpu.h")).read()


def test_the_four_symbols_are_exported_and_bound(built):
    from bulletproofs_amd import _lib
    L = built.lib()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_extern as g
    protos = {name: args for name, _, args in g.prototypes(_header())}
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.EXPORTS and name in protos
        assert len(getattr(L, name).argtypes) == len(protos[name].split(",")), name   # the binding takes what the header declares
    # the argument lists are the seeded prover's plus `messages`
    for suffix in ("", "_dev"):
        ts, rw = protos["bpgpu_rangeproof_prove_batch_ts" + suffix].split(","), protos["bpgpu_rangeproof_prove_batch_rw" + suffix].split(",")
        extra = [a for a in rw if a not in ts]
        assert len(rw) == len(ts) + 1 and len(extra) == 1 and "messages" in extra[0]
    for method in ("rangeproof_prove_batch_rw", "rangeproof_prove_batch_rw_dev", "rangeproof_rewind_batch", "rangeproof_rewind_batch_dev"):
        assert callable(getattr(_lib.Context, method))
    assert (_lib.REWIND_OK, _lib.REWIND_NOT_FOUND, _lib.REWIND_FORMAT) == (0, 1, 2)
    h = _header()
    assert "#define BPGPU_REWIND_OK 0" in h and "#define BPGPU_REWIND_NOT_FOUND 1" in h and "#define BPGPU_REWIND_FORMAT 2" in h
    for method in ("rewind_batch", "rewind_single", "rewind_seeds", "prove_batch"):
        assert callable(getattr(built.RangeProof, method))
    import inspect
    sig = inspect.signature(built.RangeProof.prove_batch).parameters
    assert sig["rewind"].default is False and sig["messages"].default is None
    hpp = open(os.path.join(ROOT, "include", "bulletproofs.hpp")).read()
    for needle in ("prove_batch_rewindable(", "rewind_batch(", "rewind_single(", "rewind_seeds(", "bpgpu_rangeproof_prove_batch_rw(", "bpgpu_rangeproof_rewind_batch(",
                   "BPGPU_REWIND_FORMAT", "bpgpu rewind seed v1"):
        assert needle in hpp, needle


def test_the_header_states_the_protocol_and_what_rewinding_is_not():
    h = " ".join(_header().replace("\n *", " ").split())        # (the comment's line breaks and leading stars taken out)
    for phrase in ("m = 1 ONLY", "a_blinding = d_0 - e (mod l)", "e = d_0 + d_1 x - e_blinding (mod l)", "e >= 2^192: BPGPU_REWIND_NOT_FOUND",
                   "gamma = (t_x_blinding - x (d_{2n+2} + x d_{2n+3})) z^-2", "compress(v B + gamma B_blinding) != V: BPGPU_REWIND_NOT_FOUND",
                   "all zero unless its status is BPGPU_REWIND_OK", "It does NOT verify the proof", "A changed e_blinding can change the recovered message",
                   "Whoever holds a seed opens the output", "A SEED MUST NEVER SERVE TWO (COMMITMENT, TRANSCRIPT) PAIRS", "z is public",
                   'Transcript::new(b"bpgpu rewind seed v1")', 't.append_message(b"key", key32)', 't.append_message(b"C", commitment_i)',
                   't.challenge_bytes(b"seed", 32 bytes)', "block 0 replaced by the 32 canonical bytes of (d_0 - e) mod l, zero-extended to 64"):
        assert phrase in h, phrase


def test_calls_without_a_context_are_refused(built):
    L = built.lib()
    b = lambda n: C.create_string_buffer(n)
    ts, pr, cm, seed = b(208), b(480), b(32), b(32)
    va = (C.c_uint64 * 1)(1)
    assert L.bpgpu_rangeproof_prove_batch_rw(None, 8, 1, 1, va, b(32), ts, 0, seed, None, pr, cm, None) == INVALID_ARG
    assert L.bpgpu_rangeproof_prove_batch_rw_dev(None, 8, 1, 1, 256, 512, 768, 0, 1024, None, 1280, 1536, None, None) == INVALID_ARG
    assert L.bpgpu_rangeproof_rewind_batch(None, 8, 1, pr, 480, cm, ts, 0, seed, b(1), va, b(16), b(32)) == INVALID_ARG
    assert L.bpgpu_rangeproof_rewind_batch_dev(None, 8, 1, 256, 480, 512, 768, 0, 1024, 1280, 1536, 1792, 2048, None) == INVALID_ARG
    assert L.bpgpu_rangeproof_rewind_batch(None, 8, 0, None, 480, None, ts, 0, None, None, None, None, None) == INVALID_ARG   # even the empty batch names its context


def test_rust_declarations_are_present():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_extern as g
    protos = {name: (ret, args) for name, ret, args in g.prototypes(_header())}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        decl = g.rust_decl(name, *protos[name])
        assert decl in doc, name
        assert decl.strip().endswith("-> c_int;")
    assert "messages: *const u8" in g.rust_decl(NAMES[0], *protos[NAMES[0]]) and "values_out: *mut u64" in g.rust_decl(NAMES[2], *protos[NAMES[2]])
    assert subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "gen_rust_extern.py"), "--missing"], text=True).strip() == ""
