"""bpgpu_sigma_* at the ABI, without a GPU: the symbols as include/bpgpu.h declares them, the Rust declarations tools/gen_rust_extern.py
derives, the Python bindings' argument lists, the protocol lines of the header, the descriptor validator (bpgpu_sigma_descriptor_check:
the validation of bpgpu_sigma_relation_create, host only) on each malformed class, and the argument check that needs no context."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1
NAMES = ["bpgpu_sigma_descriptor_check", "bpgpu_sigma_relation_create", "bpgpu_sigma_relation_destroy", "bpgpu_sigma_relation_shape",
         "bpgpu_sigma_create_batch_ts", "bpgpu_sigma_verify_batch_ts", "bpgpu_sigma_verify_batch_ts_dev", "bpgpu_sigma_verify_rlc_ts",
         "bpgpu_sigma_verify_rlc_ts_dev"]


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    import bulletproofs_amd as bp
    return bp


def _header():
    return open(os.path.join(ROOT, "include", "bpgpu.h")).read()


def test_the_symbols_are_exported_and_bound(built):
    from bulletproofs_amd import _lib
    L = built.lib()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_extern as g
    protos = {name: args for name, _, args in g.prototypes(_header())}
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.EXPORTS and name in protos
        assert len(getattr(L, name).argtypes) == len(protos[name].split(",")), name   # the binding takes what the header declares
    for method in ("sigma_relation_create", "sigma_relation_destroy", "sigma_create_batch_ts", "sigma_verify_batch_ts", "sigma_verify_rlc_ts",
                   "sigma_verify_batch_ts_dev", "sigma_verify_rlc_ts_dev"):
        assert callable(getattr(_lib.Context, method))
    for method in ("secret", "point", "G", "equation", "compile"):
        assert callable(getattr(built.SigmaStatement, method))
    for method in ("create_batch", "verify_batch", "verify_batch_combined", "create", "verify"):
        assert callable(getattr(built.SigmaRelation, method))
    hpp = open(os.path.join(ROOT, "include", "bulletproofs.hpp")).read()
    for needle in ("class SigmaStatement", "class SigmaRelation", "create_batch(", "verify_batch_combined(", "bpgpu_sigma_relation_create(", "bpgpu_sigma_create_batch_ts(",
                   "bpgpu_sigma_verify_batch_ts(", "bpgpu_sigma_verify_rlc_ts(", 'append_message(b"dom-sep", b"sigmaproof v1")', "T_1 | .. | T_E | s_1 | .. | s_S"):
        assert needle in hpp, needle


def test_the_header_states_the_protocol_the_contracts_and_the_seed_rule():
    h = " ".join(_header().replace("\n *", " ").split())        # (the comment's line breaks and leading stars taken out)
    for phrase in ('append_message(b"dom-sep", b"sigmaproof v1"); append_message(b"stmt", digest)',
                   "u8 S, u8 P, u8 E, then per equation u8 lhs, u8 nterms, then nterms x (u8 secret, u8 base)",
                   "proof = T_1 | .. | T_E | s_1 | .. | s_S, 32 (E + S) bytes",
                   "(a) msm_out of (row, equation) equals bpgpu_msm_batch on that equation's terms",
                   "(b) verdict and transcripts_out of an _rlc_ts call ALWAYS equal those of the _verify_batch_ts call",
                   "(c) a created proof verifies and both sides' transcripts_out are equal",
                   "A SEED MUST NEVER SERVE TWO DIFFERENT STATEMENTS OR TRANSCRIPTS",
                   "Public scalar coefficients are out of scope"):
        assert phrase in h, phrase


def test_the_validator_rejects_each_malformed_descriptor_class(built, oracle):
    """the classes of the header: a count out of range, an lhs that is not an instance slot, a secret used in no term, an instance slot
    used nowhere, a G_i beyond the loaded generators; and what a byte string can get wrong besides.  The named relations pass, with the
    twin's digest."""
    import sigma_cases
    import sigma_twin as tw
    L = built.lib()
    chk = lambda desc, cap=8: L.bpgpu_sigma_descriptor_check(bytes(desc), len(desc), cap, None)
    for name, rel in list(sigma_cases.RELATIONS.items()) + [("R3'", sigma_cases.R3_SWAPPED)]:
        desc = tw.descriptor(rel)
        dg = C.create_string_buffer(32)
        assert L.bpgpu_sigma_descriptor_check(desc, len(desc), 8, dg) == 0 and dg.raw == tw.digest(desc), name
    dleq = [1, 3, 2, 16, 1, 0, 1, 17, 1, 0, 18]
    assert chk(dleq) == 0 and chk(dleq, 0) == 0                 # (no G_i: no generator needed)
    bad = {
        "S = 0": [0, 1, 1, 16, 1, 0, 1],
        "S = 9": [9, 1, 1, 16, 1, 0, 1],
        "P = 0": [1, 0, 1, 16, 1, 0, 1],
        "P = 9": [1, 9, 1, 16, 1, 0, 1],
        "E = 0": [1, 1, 0],
        "E = 9": [1, 1, 9] + [16, 1, 0, 1] * 9,
        "no terms": [1, 1, 1, 16, 0],
        "nine terms": [1, 1, 1, 16, 9] + [0, 1] * 9,
        "33 terms in all": [1, 5, 5] + sum(([16 + k, 7] + [0, 1] * 7 for k in range(4)), []) + [20, 5] + [0, 1] * 5,
        "lhs is a shared base": [1, 1, 1, 1, 1, 0, 0],
        "lhs beyond P": [1, 1, 1, 17, 1, 0, 1],
        "secret out of range": [1, 1, 1, 16, 1, 1, 1],
        "secret used in no term": [2, 1, 1, 16, 1, 0, 1],
        "slot used nowhere": [1, 2, 1, 16, 1, 0, 1],
        "slot out of range": [1, 1, 1, 16, 1, 0, 17],
        "base id 10 .. 15": [1, 1, 1, 16, 1, 0, 10],
        "ends early": dleq[:-1],
        "ends late": dleq + [0],
        "header only": [1, 1],
    }
    for why, desc in bad.items():
        assert chk(desc) == INVALID_ARG, why
    use_g3 = [1, 1, 1, 16, 1, 0, 5]
    assert chk(use_g3, 4) == 0 and chk(use_g3, 3) == INVALID_ARG                   # G_3 needs four generators
    assert chk([1, 5, 5] + sum(([16 + k, 7] + [0, 1] * 7 for k in range(4)), []) + [20, 4] + [0, 1] * 4) == 0   # 32 terms exactly
    assert L.bpgpu_sigma_descriptor_check(None, 0, 8, None) == INVALID_ARG


def test_calls_without_a_context_or_relation_are_refused(built):
    L = built.lib()
    b = lambda n: C.create_string_buffer(n)
    ts, pr, pt, vd, out = b(208), b(96), b(96), b(1), b(208)
    h = C.c_void_p()
    assert L.bpgpu_sigma_relation_create(None, bytes([1, 1, 1, 16, 1, 0, 1]), 7, C.byref(h)) == INVALID_ARG and not h.value
    assert L.bpgpu_sigma_relation_shape(None, None, None, None, None) == INVALID_ARG
    L.bpgpu_sigma_relation_destroy(None)
    assert L.bpgpu_sigma_create_batch_ts(None, None, 1, ts, 0, b(32), pt, b(32), pr, vd, out) == INVALID_ARG
    assert L.bpgpu_sigma_verify_batch_ts(None, None, 1, pr, 96, ts, 0, pt, vd, None, None) == INVALID_ARG
    assert L.bpgpu_sigma_verify_rlc_ts(None, None, 1, pr, 96, ts, 0, pt, None, vd, None, None) == INVALID_ARG
    assert L.bpgpu_sigma_verify_batch_ts_dev(None, None, 1, 256, 96, ts, None, 512, 768, None, None, None) == INVALID_ARG
    assert L.bpgpu_sigma_verify_rlc_ts_dev(None, None, 1, 256, 96, ts, None, 512, None, 768, None, None, None) == INVALID_ARG


def test_rust_declarations_are_present():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_extern as g
    protos = {name: (ret, args) for name, ret, args in g.prototypes(_header())}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert g.rust_decl(name, *protos[name]) in doc, name
    assert "pub struct bpgpu_sigma_relation" in doc
    assert subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "gen_rust_extern.py"), "--missing"], text=True).strip() == ""
