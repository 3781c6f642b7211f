"""bpgpu_rangeproof_scan_batch and its _dev form at the ABI: the two symbols as include/bpgpu.h declares them, the Rust declarations
tools/gen_rust_extern.py derives, the Python bindings' argument lists, the mirror in bulletproofs.hpp, the consequences the header must
state, and the call without a context.  Every other refusal carries the context's error text and so needs a context: the last test
(marked gpu) makes them on a real one -- nkeys 0 and 1 025, a product over 2^28, a bad proof_len, a bad stride, a malformed state, a
NULL key pointer, a context without generators -- each before anything is staged."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, NO_GENS = -1, -3
NAMES = ["bpgpu_rangeproof_scan_batch", "bpgpu_rangeproof_scan_batch_dev"]


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    import bulletproofs_amd as bp
    return bp


def _header():
    return open(os.path.join(ROOT, "include", "bpgpu.h")).read()


def _protos():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_extern as g
    return g, {name: (ret, args) for name, ret, args in g.prototypes(_header())}


def test_the_two_symbols_are_exported_and_bound(built):
    from bulletproofs_amd import _lib
    L = built.lib()
    _, protos = _protos()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.EXPORTS and name in protos
        assert len(getattr(L, name).argtypes) == len(protos[name][1].split(",")), name   # the binding takes what the header declares
    # the argument lists are the rewinder's with (keys32, nkeys) in the seeds' place and key_index_out behind the status
    for suffix in ("", "_dev"):
        rw, sc = (protos["bpgpu_rangeproof_%s_batch%s" % (k, suffix)][1].split(",") for k in ("rewind", "scan"))
        names = lambda args: [a.split()[-1].lstrip("*") for a in args]
        d = "d_" if suffix else ""
        want = names(rw)
        at = want.index(d + "rng32")
        want[at:at + 1] = [d + "keys32", "nkeys"]
        want.insert(want.index(d + "status_out") + 1, d + "key_index_out")
        assert names(sc) == want, suffix
    vp, sz, u8p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint8)
    host = L.bpgpu_rangeproof_scan_batch.argtypes
    assert host[9] is sz and host[11] is C.POINTER(C.c_uint32) and host[12] is C.POINTER(C.c_uint64)
    assert L.bpgpu_rangeproof_scan_batch_dev.argtypes == [vp, sz, sz, vp, sz, vp, vp, sz, vp, sz, vp, vp, vp, vp, vp, vp]
    for method in ("rangeproof_scan_batch", "rangeproof_scan_batch_dev"):
        assert callable(getattr(_lib.Context, method))
    import inspect
    assert list(inspect.signature(built.RangeProof.scan_batch).parameters) == ["bp_gens", "pc_gens", "transcripts", "proofs", "commitments", "n", "keys"]
    hpp = open(os.path.join(ROOT, "include", "bulletproofs.hpp")).read()
    for needle in ("scan_batch(", "bpgpu_rangeproof_scan_batch(", "keys32, nkeys"):
        assert needle in hpp, needle


def test_the_header_states_the_contract_and_its_consequences():
    h = " ".join(_header().replace("\n *", " ").split())        # (the comment's line breaks and leading stars taken out)
    for phrase in ("j* is the LOWEST j with e_j < 2^192", "key_index_out : nbatch x u32, j* when the status is OK, else 0xFFFFFFFF",
                   "If at most one key of a row passes step 2, row p equals the first BPGPU_REWIND_OK", "nkeys * 2^-61",
                   "A key listed twice reports the lower index", "EVEN IF A HIGHER KEY WOULD OPEN IT", "scanning does NOT verify",
                   "1 <= nkeys <= 1024, nbatch <= 2^26, nbatch * nkeys <= 2^28", "nbatch = 0 is BPGPU_OK", "BPGPU_ERR_NO_GENS",
                   "144 < 166", "ONE Keccak-f", "nothing branches on e or j*", "z's inversion stays the variable-time one",
                   "the _dev form stages nothing, reads nothing back"):
        assert phrase in h, phrase
    assert h.index("WHAT REWINDING IS NOT") < h.index("EVEN IF A HIGHER KEY WOULD OPEN IT")


def test_calls_without_a_context_are_refused(built):
    L = built.lib()
    b = lambda n: C.create_string_buffer(n)
    ts, pr, cm, keys = b(208), b(480), b(32), b(64)
    va, ki = (C.c_uint64 * 1)(), (C.c_uint32 * 1)()
    assert L.bpgpu_rangeproof_scan_batch(None, 8, 1, pr, 480, cm, ts, 0, keys, 2, b(1), ki, va, b(16), b(32)) == INVALID_ARG
    assert L.bpgpu_rangeproof_scan_batch_dev(None, 8, 1, 256, 480, 512, 768, 0, 1024, 2, 1280, 1536, 1792, 2048, 2304, None) == INVALID_ARG
    assert L.bpgpu_rangeproof_scan_batch(None, 8, 0, None, 480, None, ts, 0, keys, 2, None, None, None, None, None) == INVALID_ARG   # even the empty batch names its context


def test_rust_declarations_are_present():
    g, protos = _protos()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        decl = g.rust_decl(name, *protos[name])
        assert decl in doc, name
        assert decl.strip().endswith("-> c_int;")
    d = g.rust_decl(NAMES[0], *protos[NAMES[0]])
    assert "keys32: *const u8" in d and "nkeys: usize" in d and "key_index_out: *mut u32" in d
    assert subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "gen_rust_extern.py"), "--missing"], text=True).strip() == ""


@pytest.mark.gpu
def test_every_refusal_comes_before_anything_is_staged():
    """On a context: each bad argument alone gives BPGPU_ERR_INVALID_ARG from both forms, with every data pointer NULL or a small
    integer -- a call that staged or launched anything would fault on them -- and the outputs untouched; nbatch = 0 is BPGPU_OK; a
    context without generators answers BPGPU_ERR_NO_GENS to a well-formed call."""
    import bulletproofs_amd as bp
    L = bp.lib()
    b = lambda n: C.create_string_buffer(b"\x5a" * n, n)
    ctx = bp.Context(0)
    try:
        ts = bp.Transcript(b"scan abi").state
        pr, cm, keys = bytes(480), bytes(32), bytes(64)
        st, ki, va, mo, go = b(1), (C.c_uint32 * 1)(0x5a5a5a5a), (C.c_uint64 * 1)(0x5a5a), b(16), b(32)
        host = lambda n=8, nb=1, pl=480, stride=0, k=keys, nk=2, t=ts: L.bpgpu_rangeproof_scan_batch(ctx.h, n, nb, pr, pl, cm, t, stride, k, nk, st, ki, va, mo, go)
        dev = lambda n=8, nb=1, pl=480, stride=0, k=1024, nk=2: L.bpgpu_rangeproof_scan_batch_dev(ctx.h, n, nb, 256, pl, 512, 768, stride, k, nk, 1280, 1536, 1792, 2048,
                                                                                                   2304, None)
        for kw in (dict(nk=0), dict(nk=1025), dict(nb=(1 << 28) // 1024 + 1, nk=1024), dict(nb=(1 << 26) + 1, nk=1), dict(nb=(1 << 27), nk=2), dict(pl=512),
                   dict(pl=416), dict(stride=104), dict(n=7), dict(n=64), dict(k=None)):
            assert host(**kw) == INVALID_ARG, kw
            assert dev(**kw) == INVALID_ARG, kw
        bad = ts[:200] + bytes([200]) + ts[201:]
        assert host(t=bad) == INVALID_ARG
        assert host(t=None) == INVALID_ARG
        assert host(nb=0) == 0 and dev(nb=0) == 0
        assert L.bpgpu_rangeproof_scan_batch(ctx.h, 8, 0, None, 480, None, ts, 0, None, 1, None, None, None, None, None) == 0
        assert host(nb=0, nk=0) == INVALID_ARG                     # the limits hold for the empty batch too
        # the largest product is not refused for its size: without generators it gets as far as BPGPU_ERR_NO_GENS
        assert L.bpgpu_rangeproof_scan_batch_dev(ctx.h, 8, (1 << 28) // 1024, 256, 480, 512, 768, 0, 1024, 1024, 1280, 1536, 1792, 2048, 2304, None) == NO_GENS
        assert host() == NO_GENS and dev() == NO_GENS
        assert (st.raw, ki[0], va[0], mo.raw, go.raw) == (b"\x5a", 0x5a5a5a5a, 0x5a5a, b"\x5a" * 16, b"\x5a" * 32)
    finally:
        ctx.close()
