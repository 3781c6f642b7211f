"""bpgpu_transcript_batch / _dev at the ABI, without a GPU: the symbols and the op struct as include/bpgpu.h declares them, the documented
caps, the Rust declarations tools/gen_rust_extern.py derives, and the argument checks that need no context."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    import bulletproofs_amd as bp
    return bp


def _header():
    return open(os.path.join(ROOT, "include", "bpgpu.h")).read()


def test_symbols_and_constants_match_the_header(built):
    from bulletproofs_amd import _lib
    L = built.lib()
    assert hasattr(L, "bpgpu_transcript_batch") and hasattr(L, "bpgpu_transcript_batch_dev")
    defs = dict(re.findall(r"^#define (BPGPU_TS_[A-Z_0-9]+) (\d+)$", _header(), re.M))
    assert {k: int(v) for k, v in defs.items()} == {
        "BPGPU_TS_APPEND": _lib.TS_APPEND, "BPGPU_TS_APPEND_U64": _lib.TS_APPEND_U64, "BPGPU_TS_CHALLENGE": _lib.TS_CHALLENGE,
        "BPGPU_TS_CHALLENGE_SCALAR": _lib.TS_CHALLENGE_SCALAR, "BPGPU_TS_MAX_OPS": _lib.TS_MAX_OPS, "BPGPU_TS_MAX_LABEL": _lib.TS_MAX_LABEL,
        "BPGPU_TS_MAX_LEN": _lib.TS_MAX_LEN, "BPGPU_TS_MAX_CHALLENGE": _lib.TS_MAX_CHALLENGE}
    # the struct: the fields of the header in its order, laid out as a C compiler lays them out on a 64-bit target
    body = re.search(r"typedef struct bpgpu_ts_op \{(.*?)\} bpgpu_ts_op;", _header(), re.S).group(1)
    assert [d.split()[-1].lstrip("*") for d in body.split(";") if d.strip()] == [f[0] for f in _lib.TsOp._fields_]
    assert C.sizeof(_lib.TsOp) == 56 and _lib.TsOp.data.offset == 24 and _lib.TsOp.lens.offset == 48


def test_calls_without_a_context_are_refused(built):
    from bulletproofs_amd import _lib
    L = built.lib()
    st, out = C.create_string_buffer(_lib.transcript_new(b"x"), 208), C.create_string_buffer(208)
    assert L.bpgpu_transcript_batch(None, 1, None, 0, st, 208, None, 0, out) == INVALID_ARG
    assert L.bpgpu_transcript_batch_dev(None, 1, None, 0, 256, 208, None, 0, 512, None) == INVALID_ARG
    assert L.bpgpu_transcript_batch(None, 0, None, 0, None, 0, None, 0, None) == INVALID_ARG      # even the empty batch names its context


def test_rust_declarations_cover_the_struct_and_both_prototypes():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_extern as g
    struct = "#[repr(C)] pub struct bpgpu_ts_op { pub kind: u32, pub label: *const u8, pub label_len: usize, pub data: *mut c_void, pub stride: usize, pub len: usize, pub lens: *const u32 }"
    assert [g.rust_struct(name, fields) for name, fields in g.structs(_header())] == [struct]
    protos = {name: (ret, args) for name, ret, args in g.prototypes(_header())}
    host, dev = g.rust_decl("bpgpu_transcript_batch", *protos["bpgpu_transcript_batch"]), g.rust_decl("bpgpu_transcript_batch_dev", *protos["bpgpu_transcript_batch_dev"])
    assert host.strip() == ("pub fn bpgpu_transcript_batch(ctx: *mut bpgpu_ctx, nbatch: usize, new_label: *const u8, new_label_len: usize, states_in: *const u8, "
                            "stride_in: usize, ops: *const bpgpu_ts_op, nops: usize, states_out: *mut u8) -> c_int;")
    assert "d_states_in: *const c_void" in dev and dev.strip().endswith("d_states_out: *mut c_void, stream: *mut c_void) -> c_int;")
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert struct in doc and host in doc and dev in doc
    # and the tool's own listing of what INTEGRATION.md lacks stays empty
    assert subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "gen_rust_extern.py"), "--missing"], text=True).strip() == ""
