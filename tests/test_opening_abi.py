"""bpgpu_opening_* at the ABI, without a GPU: the five symbols as include/bpgpu.h declares them, the Rust declarations
tools/gen_rust_extern.py derives, the Python bindings' argument lists, the three contracts in the header, and the argument check that
needs no context.  (A bad form or proof_len is refused before anything is staged, but the refusal carries the context's error text:
tests/test_gpu_opening.py makes those calls on a real context.)"""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1
NAMES = ["bpgpu_opening_create_batch_ts", "bpgpu_opening_verify_batch_ts", "bpgpu_opening_verify_batch_ts_dev", "bpgpu_opening_verify_rlc_ts",
         "bpgpu_opening_verify_rlc_ts_dev"]


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    import bulletproofs_amd as bp
    return bp


def _header():
    return open(os.path.join(ROOT, "include", "bpgpu.h")).read()


def test_the_five_symbols_are_exported_and_bound(built):
    from bulletproofs_amd import _lib
    L = built.lib()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_extern as g
    protos = {name: args for name, _, args in g.prototypes(_header())}
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.EXPORTS and name in protos
        assert len(getattr(L, name).argtypes) == len(protos[name].split(",")), name   # the binding takes what the header declares
    for method in ("opening_create_batch_ts", "opening_verify_batch_ts", "opening_verify_rlc_ts", "opening_verify_batch_ts_dev", "opening_verify_rlc_ts_dev"):
        assert callable(getattr(_lib.Context, method))
    assert (_lib.OPENING_FULL, _lib.OPENING_BLINDING) == (0, 1)
    h = _header()
    assert "#define BPGPU_OPENING_FULL 0" in h and "#define BPGPU_OPENING_BLINDING 1" in h
    from bulletproofs_amd.api import BulletproofGens
    for method in ("create_batch", "verify_batch", "verify_batch_combined", "create", "verify"):
        assert callable(getattr(built.OpeningProof, method))
    assert callable(BulletproofGens.prove_balance) and callable(BulletproofGens.verify_balance_proved)
    hpp = open(os.path.join(ROOT, "include", "bulletproofs.hpp")).read()
    for needle in ("class OpeningProof", "create_batch(", "verify_batch_combined(", "prove_balance(", "verify_balance_proved(", "bpgpu_opening_create_batch_ts(",
                   "bpgpu_opening_verify_batch_ts(", "bpgpu_opening_verify_rlc_ts("):
        assert needle in hpp, needle


def test_the_header_states_the_three_contracts_and_the_seed_rule():
    h = " ".join(_header().replace("\n *", " ").split())        # (the comment's line breaks and leading stars taken out)
    for phrase in ("(a) a row's msm_out equals bpgpu_msm_batch on (s_v, B), (s_r, B_blinding), (l - c, C), (l - 1, R)",
                   "(b) verdict and transcripts_out of an _rlc_ts call ALWAYS equal those of the _verify_batch_ts call",
                   "(c) a proof from bpgpu_opening_create_batch_ts verifies, and the transcripts_out of the two sides are equal",
                   "A SEED MUST NEVER BE USED FOR TWO DIFFERENT STATEMENTS OR TRANSCRIPTS"):
        assert phrase in h, phrase


def test_calls_without_a_context_are_refused(built):
    L = built.lib()
    b = lambda n: C.create_string_buffer(n)
    ts, pr, cm, vd, out = b(208), b(96), b(32), b(1), b(208)
    assert L.bpgpu_opening_create_batch_ts(None, 0, 1, ts, 0, b(32), cm, b(8), 8, b(32), pr, vd, out) == INVALID_ARG
    assert L.bpgpu_opening_verify_batch_ts(None, 0, 1, pr, 96, ts, 0, cm, None, 8, vd, None, None) == INVALID_ARG
    assert L.bpgpu_opening_verify_rlc_ts(None, 1, 1, pr, 64, ts, 0, cm, None, 8, None, vd, None, None) == INVALID_ARG
    assert L.bpgpu_opening_verify_batch_ts_dev(None, 0, 1, 256, 96, ts, None, 512, None, 8, 768, None, None, None) == INVALID_ARG
    assert L.bpgpu_opening_verify_rlc_ts_dev(None, 1, 1, 256, 64, ts, None, 512, None, 8, None, 768, None, None, None) == INVALID_ARG
    assert L.bpgpu_opening_verify_rlc_ts(None, 0, 0, None, 96, ts, 0, None, None, 8, None, None, None, None) == INVALID_ARG   # even the empty batch names its context


def test_rust_declarations_are_present():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_extern as g
    protos = {name: (ret, args) for name, ret, args in g.prototypes(_header())}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        decl = g.rust_decl(name, *protos[name])
        assert decl in doc, name
        assert "form: c_int" in decl and decl.strip().endswith("-> c_int;")
    assert subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "gen_rust_extern.py"), "--missing"], text=True).strip() == ""
