"""bpgpu_pedersen_sum_batch / _balance_batch and their _dev forms at the ABI, without a GPU: the four symbols as include/bpgpu.h declares
them, the Rust declarations tools/gen_rust_extern.py derives, the Python bindings' argument lists, and the argument checks that need no
context."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1
NAMES = ["bpgpu_pedersen_sum_batch", "bpgpu_pedersen_balance_batch", "bpgpu_pedersen_sum_batch_dev", "bpgpu_pedersen_balance_batch_dev"]


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
    for method in ("pedersen_sum_batch", "pedersen_balance_batch", "pedersen_sum_batch_dev", "pedersen_balance_batch_dev"):
        assert callable(getattr(_lib.Context, method))
    from bulletproofs_amd.api import BulletproofGens
    assert callable(BulletproofGens.sum_commitments) and callable(BulletproofGens.verify_balance)
    hpp = open(os.path.join(ROOT, "include", "bulletproofs.hpp")).read()
    assert "sum_commitments(" in hpp and "verify_balance(" in hpp and "bpgpu_pedersen_sum_batch(" in hpp and "bpgpu_pedersen_balance_batch(" in hpp


def test_the_header_states_the_three_contracts():
    h = " ".join(_header().replace("\n *", " ").split())        # (the comment's line breaks and leading stars taken out)
    for phrase in ("(a) row r of the sum call equals bpgpu_msm_batch", "(b) a row without terms equals row r of bpgpu_pedersen_commit_batch",
                   "(c) a balance row with exactly one added term has the verdict of bpgpu_pedersen_open_batch"):
        assert phrase in h, phrase


def test_calls_without_a_context_are_refused(built):
    L = built.lib()
    off = (C.c_uint32 * 2)(0, 1)
    pt, out, st = C.create_string_buffer(32), C.create_string_buffer(32), C.create_string_buffer(1)
    assert L.bpgpu_pedersen_sum_batch(None, 1, off, pt, None, None, 8, None, out, st) == INVALID_ARG
    assert L.bpgpu_pedersen_balance_batch(None, 1, off, pt, None, None, 8, None, st) == INVALID_ARG
    assert L.bpgpu_pedersen_sum_batch_dev(None, 1, off, 256, None, None, 8, None, 512, 768, None) == INVALID_ARG
    assert L.bpgpu_pedersen_balance_batch_dev(None, 1, off, 256, None, None, 8, None, 768, None) == INVALID_ARG
    assert L.bpgpu_pedersen_sum_batch(None, 0, None, None, None, None, 8, None, None, None) == INVALID_ARG      # even the empty batch names its context
    assert L.bpgpu_pedersen_balance_batch_dev(None, 0, None, None, None, None, 8, None, None, None) == INVALID_ARG


def test_rust_declarations_are_present():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_extern as g
    protos = {name: (ret, args) for name, ret, args in g.prototypes(_header())}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        decl = g.rust_decl(name, *protos[name])
        assert decl in doc, name
        assert "row_offsets: *const u32" in decl and decl.strip().endswith("-> c_int;")
    host = g.rust_decl(NAMES[0], *protos[NAMES[0]])
    assert host.strip() == ("pub fn bpgpu_pedersen_sum_batch(ctx: *mut bpgpu_ctx, nbatch: usize, row_offsets: *const u32, points: *const u8, signs: *const u8, "
                            "values: *const c_void, value_bytes: usize, blindings: *const u8, out: *mut u8, status_out: *mut u8) -> c_int;")
    assert subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "gen_rust_extern.py"), "--missing"], text=True).strip() == ""
