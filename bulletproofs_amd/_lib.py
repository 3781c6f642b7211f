"""ctypes binding of libbpgpu.so (the C ABI declared in include/bpgpu.h).

There is no CPU fallback: if the HIP library is missing or no GPU is usable,
everything here raises.  Nothing under oracle/ is ever imported.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libbpgpu.so")

_lib = None

EXPORTS = [
    "bpgpu_r1cs_circuit_create", "bpgpu_r1cs_circuit_destroy", "bpgpu_r1cs_circuit_shape", "bpgpu_r1cs_verify_batch_ts",
    "bpgpu_r1cs_verify_batch_ts_dev", "bpgpu_pool_r1cs_verify_ts", "bpgpu_r1cs_witness_create", "bpgpu_r1cs_witness_destroy",
    "bpgpu_r1cs_prove_batch", "bpgpu_r1cs_verify_rlc", "bpgpu_pool_r1cs_verify_rlc",
    "bpgpu_r1cs_witness_check", "bpgpu_r1cs_prove_batch_checked",
    "bpgpu_version", "bpgpu_ctx_create", "bpgpu_ctx_destroy", "bpgpu_last_error", "bpgpu_ctx_set_option",
    "bpgpu_ctx_get_option",
    "bpgpu_synchronize", "bpgpu_gens_create", "bpgpu_gens_load", "bpgpu_gens_export",
    "bpgpu_msm_batch", "bpgpu_msm_batch_dev", "bpgpu_msm_batch_shared", "bpgpu_msm_batch_shared_dev",
    "bpgpu_rangeproof_verify_batch", "bpgpu_rangeproof_verify_batch_dev", "bpgpu_ipp_verify_batch",
    "bpgpu_rangeproof_verify_rlc", "bpgpu_rangeproof_verify_rlc_dev",
    "bpgpu_rangeproof_verify_rlc_mixed", "bpgpu_pool_rangeproof_verify_rlc_mixed",
    "bpgpu_rangeproof_verify_rlc_ts", "bpgpu_rangeproof_verify_rlc_ts_dev", "bpgpu_rangeproof_verify_rlc_mixed_ts",
    "bpgpu_pool_rangeproof_verify_rlc_mixed_ts",
    "bpgpu_profile_enable", "bpgpu_profile_reset", "bpgpu_profile_report",
    "bpgpu_transcript_new", "bpgpu_transcript_append_message", "bpgpu_transcript_challenge_bytes",
    "bpgpu_transcript_batch", "bpgpu_transcript_batch_dev",
    "bpgpu_rangeproof_verify_batch_ts", "bpgpu_rangeproof_verify_batch_ts_dev", "bpgpu_ipp_verify_batch_dev",
    "bpgpu_ipp_create_batch", "bpgpu_rangeproof_prove_batch", "bpgpu_rangeproof_verify_batch_submit", "bpgpu_ctx_collect",
    "bpgpu_rangeproof_prove_batch_ts", "bpgpu_rangeproof_prove_batch_ts_dev",
    "bpgpu_linear_verify_batch", "bpgpu_linear_verify_batch_dev", "bpgpu_linear_create_batch",
    "bpgpu_linear_verify_rlc", "bpgpu_linear_verify_rlc_dev", "bpgpu_ipp_verify_rlc", "bpgpu_ipp_verify_rlc_dev",
    "bpgpu_ipp_verify_batch_ts", "bpgpu_ipp_verify_batch_ts_dev", "bpgpu_ipp_verify_rlc_ts", "bpgpu_ipp_verify_rlc_ts_dev",
    "bpgpu_linear_verify_batch_ts", "bpgpu_linear_verify_batch_ts_dev", "bpgpu_linear_verify_rlc_ts", "bpgpu_linear_verify_rlc_ts_dev",
    "bpgpu_ipp_create_batch_ts", "bpgpu_linear_create_batch_ts",
    "bpgpu_rangeproof_audit_shares", "bpgpu_ipp_verification_scalars",
    "bpgpu_pool_create", "bpgpu_pool_destroy", "bpgpu_pool_last_error", "bpgpu_pool_set_option", "bpgpu_pool_get_option",
    "bpgpu_pool_devices", "bpgpu_pool_lanes", "bpgpu_pool_lane", "bpgpu_pool_gens_create", "bpgpu_pool_gens_load",
    "bpgpu_pool_rangeproof_verify", "bpgpu_pool_rangeproof_submit_dev", "bpgpu_pool_flush", "bpgpu_pool_wait",
    "bpgpu_pool_rangeproof_verify_ts", "bpgpu_pool_rangeproof_submit_ts", "bpgpu_pool_ticket_done", "bpgpu_pool_ticket_wait",
    "bpgpu_pool_rangeproof_submit_dev_ex", "bpgpu_pool_ticket_stream_wait", "bpgpu_pool_rangeproof_submit_rlc_dev",
    "bpgpu_gens_add_shape", "bpgpu_pool_gens_add_shape", "bpgpu_pool_gather_dev",
    "bpgpu_pool_msm_batch_shared", "bpgpu_pool_msm_batch_shared_submit", "bpgpu_pool_msm_batch", "bpgpu_pool_ipp_verify", "bpgpu_pool_trace_dump",
    "bpgpu_pool_msm_batch_shared_submit_dev",
    "bpgpu_mpc_state1_bytes", "bpgpu_mpc_state2_bytes", "bpgpu_mpc_party_bit_commit", "bpgpu_mpc_party_poly_commit", "bpgpu_mpc_party_proof_share",
    "bpgpu_mpc_dealer_bit_challenge", "bpgpu_mpc_dealer_poly_challenge", "bpgpu_mpc_dealer_assemble",
    "bpgpu_mpc_party_bit_commit_seeded", "bpgpu_mpc_party_poly_commit_seeded",
    "bpgpu_pedersen_commit_batch", "bpgpu_pedersen_open_batch", "bpgpu_pedersen_commit_batch_dev", "bpgpu_pedersen_open_batch_dev",
    "bpgpu_pedersen_sum_batch", "bpgpu_pedersen_balance_batch", "bpgpu_pedersen_sum_batch_dev", "bpgpu_pedersen_balance_batch_dev",
    "bpgpu_opening_create_batch_ts", "bpgpu_opening_verify_batch_ts", "bpgpu_opening_verify_batch_ts_dev", "bpgpu_opening_verify_rlc_ts",
    "bpgpu_opening_verify_rlc_ts_dev",
    "bpgpu_sigma_descriptor_check", "bpgpu_sigma_relation_create", "bpgpu_sigma_relation_destroy", "bpgpu_sigma_relation_shape",
    "bpgpu_sigma_create_batch_ts", "bpgpu_sigma_verify_batch_ts", "bpgpu_sigma_verify_batch_ts_dev", "bpgpu_sigma_verify_rlc_ts",
    "bpgpu_sigma_verify_rlc_ts_dev",
    "bpgpu_rangeproof_prove_batch_rw", "bpgpu_rangeproof_prove_batch_rw_dev", "bpgpu_rangeproof_rewind_batch", "bpgpu_rangeproof_rewind_batch_dev",
    "bpgpu_rangeproof_scan_batch", "bpgpu_rangeproof_scan_batch_dev",
]

REWIND_OK, REWIND_NOT_FOUND, REWIND_FORMAT = 0, 1, 2   # bpgpu_rangeproof_rewind_batch: the status byte of a row
OPENING_FULL, OPENING_BLINDING = 0, 1   # bpgpu_opening_*: v and r secret (96-byte proofs) / v public, r secret (64-byte proofs)

TRANSCRIPT_BYTES = 208
TS_APPEND, TS_APPEND_U64, TS_CHALLENGE, TS_CHALLENGE_SCALAR = 1, 2, 3, 4       # bpgpu_ts_op.kind
TS_MAX_OPS, TS_MAX_LABEL, TS_MAX_LEN, TS_MAX_CHALLENGE = 32, 255, 65536, 4096


class TsOp(C.Structure):
    """bpgpu_ts_op"""
    _fields_ = [("kind", C.c_uint32), ("label", C.c_void_p), ("label_len", C.c_size_t), ("data", C.c_void_p), ("stride", C.c_size_t),
                ("len", C.c_size_t), ("lens", C.c_void_p)]


class BpgpuError(RuntimeError):
    pass


def lib():
    """Load libbpgpu.so (built by __graft_entry__.build()); raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm wheels bundle their own libamdhip64; if libbpgpu.so pulled in /opt/rocm's copy first, a
    # later `import torch` in the same process would bring up a second HIP runtime and find no GPU.  Loading
    # torch first makes both share one runtime (torch is plumbing here: device buffers, streams, RCCL).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise BpgpuError("libbpgpu.so not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'` -- "
                         "there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, sz, u8p, i = C.c_void_p, C.c_size_t, C.c_char_p, C.c_int
    L.bpgpu_version.restype = i
    L.bpgpu_ctx_create.argtypes = [i, C.POINTER(vp)]
    L.bpgpu_ctx_destroy.argtypes = [vp]
    L.bpgpu_ctx_destroy.restype = None
    L.bpgpu_last_error.argtypes = [vp]
    L.bpgpu_last_error.restype = C.c_char_p
    L.bpgpu_ctx_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    L.bpgpu_ctx_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    L.bpgpu_synchronize.argtypes = [vp]
    missing = [n for n in EXPORTS if not hasattr(L, n)]
    if missing:
        raise BpgpuError("libbpgpu.so lacks symbols declared in include/bpgpu.h: %s" % missing)
    L.bpgpu_gens_create.argtypes = [vp, sz, sz]
    L.bpgpu_gens_load.argtypes = [vp, sz, sz, u8p, u8p, u8p, u8p]
    L.bpgpu_gens_export.argtypes = [vp, u8p, u8p, u8p, u8p]
    L.bpgpu_msm_batch.argtypes = [vp, sz, C.POINTER(C.c_uint32), u8p, u8p, u8p, u8p]
    L.bpgpu_msm_batch_dev.argtypes = [vp, sz, C.POINTER(C.c_uint32), vp, vp, vp, vp, vp]
    L.bpgpu_msm_batch_shared.argtypes = [vp, sz, sz, sz, sz, u8p, u8p, u8p, u8p, u8p]
    L.bpgpu_msm_batch_shared_dev.argtypes = [vp, sz, sz, sz, sz, vp, vp, vp, vp, vp, vp]
    L.bpgpu_rangeproof_verify_batch.argtypes = [vp, sz, sz, sz, u8p, sz, u8p, u8p, sz, u8p, u8p, u8p]
    L.bpgpu_rangeproof_verify_batch_dev.argtypes = [vp, sz, sz, sz, vp, sz, vp, u8p, sz, vp, vp, vp, vp]
    L.bpgpu_rangeproof_verify_rlc.argtypes = [vp, sz, sz, sz, u8p, sz, u8p, u8p, sz, u8p, u8p, u8p, u8p]
    L.bpgpu_rangeproof_verify_rlc_dev.argtypes = [vp, sz, sz, sz, vp, sz, vp, u8p, sz, vp, vp, vp, vp, vp]
    szp = C.POINTER(sz)
    L.bpgpu_rangeproof_verify_rlc_mixed.argtypes = [vp, sz, szp, szp, szp, szp, u8p, u8p, C.POINTER(u8p), szp, u8p, u8p, u8p, u8p]
    L.bpgpu_pool_rangeproof_verify_rlc_mixed.argtypes = L.bpgpu_rangeproof_verify_rlc_mixed.argtypes
    L.bpgpu_rangeproof_verify_rlc_ts.argtypes = [vp, sz, sz, sz, u8p, sz, u8p, u8p, sz, u8p, u8p, u8p, u8p, u8p]
    L.bpgpu_rangeproof_verify_rlc_ts_dev.argtypes = [vp, sz, sz, sz, vp, sz, vp, u8p, vp, vp, vp, vp, vp, vp, vp]
    L.bpgpu_rangeproof_verify_rlc_mixed_ts.argtypes = [vp, sz, szp, szp, szp, szp, u8p, u8p, u8p, szp, u8p, u8p, u8p, u8p, u8p]
    L.bpgpu_pool_rangeproof_verify_rlc_mixed_ts.argtypes = L.bpgpu_rangeproof_verify_rlc_mixed_ts.argtypes
    L.bpgpu_ipp_verify_batch.argtypes = [vp, sz, sz, u8p, sz, u8p, sz, u8p, u8p, u8p, u8p, u8p, u8p, u8p, u8p]
    L.bpgpu_transcript_new.argtypes = [u8p, sz, u8p]
    L.bpgpu_transcript_append_message.argtypes = [u8p, u8p, sz, u8p, sz]
    L.bpgpu_transcript_challenge_bytes.argtypes = [u8p, u8p, sz, u8p, sz]
    L.bpgpu_transcript_batch.argtypes = [vp, sz, u8p, sz, u8p, sz, C.POINTER(TsOp), sz, u8p]
    L.bpgpu_transcript_batch_dev.argtypes = [vp, sz, u8p, sz, vp, sz, C.POINTER(TsOp), sz, vp, vp]
    L.bpgpu_rangeproof_verify_batch_ts.argtypes = [vp, sz, sz, sz, u8p, sz, u8p, u8p, sz, u8p, u8p, u8p, u8p]
    L.bpgpu_rangeproof_verify_batch_ts_dev.argtypes = [vp, sz, sz, sz, vp, sz, vp, u8p, vp, vp, vp, vp, vp, vp]
    L.bpgpu_ipp_verify_batch_dev.argtypes = [vp, sz, sz, vp, sz, u8p, sz, u8p, vp, vp, vp, vp, vp, vp, i, vp, vp, vp]
    L.bpgpu_ipp_create_batch.argtypes = [vp, sz, sz, u8p, sz, u8p, u8p, u8p, u8p, u8p, u8p, i, u8p, u8p, u8p, u8p]
    L.bpgpu_rangeproof_prove_batch.argtypes = [vp, sz, sz, sz, C.POINTER(C.c_uint64), u8p, u8p, sz, u8p, u8p, u8p, u8p, u8p]
    L.bpgpu_rangeproof_prove_batch_ts.argtypes = [vp, sz, sz, sz, C.POINTER(C.c_uint64), u8p, u8p, sz, u8p, u8p, u8p, u8p]
    L.bpgpu_rangeproof_prove_batch_ts_dev.argtypes = [vp, sz, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp, vp]
    L.bpgpu_rangeproof_verify_batch_submit.argtypes =[vp, sz, sz, sz, u8p, sz, u8p, u8p, sz, u8p, u8p, u8p]
    L.bpgpu_ctx_collect.argtypes = [vp]
    L.bpgpu_linear_verify_batch.argtypes = [vp, sz, sz, u8p, sz, u8p, sz, u8p, u8p, u8p, u8p, u8p, u8p, i, u8p, u8p, u8p]
    L.bpgpu_rangeproof_audit_shares.argtypes = [vp, sz, sz, C.POINTER(C.c_uint32), u8p, u8p, u8p, u8p, i, u8p, u8p]
    L.bpgpu_linear_create_batch.argtypes = [vp, sz, sz, u8p, sz, u8p, u8p, u8p, u8p, u8p, u8p, i, u8p, u8p, u8p, u8p, u8p, u8p]
    L.bpgpu_linear_verify_batch_dev.argtypes = [vp, sz, sz, vp, sz, u8p, sz, u8p, vp, vp, vp, vp, vp, i, vp, vp, vp, vp]
    L.bpgpu_linear_verify_rlc.argtypes = [vp, sz, sz, u8p, sz, u8p, sz, u8p, u8p, u8p, u8p, u8p, u8p, i, u8p, u8p, u8p, u8p]
    L.bpgpu_linear_verify_rlc_dev.argtypes = [vp, sz, sz, vp, sz, u8p, sz, u8p, vp, vp, vp, vp, vp, i, vp, vp, vp, vp, vp]
    L.bpgpu_ipp_verify_rlc.argtypes = [vp, sz, sz, u8p, sz, u8p, sz, u8p, u8p, u8p, u8p, u8p, u8p, u8p, sz, u8p, u8p, u8p]
    L.bpgpu_ipp_verify_rlc_dev.argtypes = [vp, sz, sz, vp, sz, u8p, sz, u8p, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp]
    L.bpgpu_ipp_verify_batch_ts.argtypes = [vp, sz, sz, u8p, sz, u8p, sz, u8p, u8p, u8p, u8p, u8p, u8p, i, u8p, u8p, u8p]
    L.bpgpu_ipp_verify_batch_ts_dev.argtypes = [vp, sz, sz, vp, sz, u8p, vp, vp, vp, vp, vp, vp, vp, i, vp, vp, vp, vp]
    L.bpgpu_ipp_verify_rlc_ts.argtypes = [vp, sz, sz, u8p, sz, u8p, sz, u8p, u8p, u8p, u8p, u8p, u8p, sz, u8p, u8p, u8p, u8p]
    L.bpgpu_ipp_verify_rlc_ts_dev.argtypes = [vp, sz, sz, vp, sz, u8p, vp, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp]
    L.bpgpu_linear_verify_batch_ts.argtypes = [vp, sz, sz, u8p, sz, u8p, sz, u8p, u8p, u8p, u8p, u8p, i, u8p, u8p, u8p]
    L.bpgpu_linear_verify_batch_ts_dev.argtypes = [vp, sz, sz, vp, sz, u8p, vp, vp, vp, vp, vp, vp, i, vp, vp, vp, vp]
    L.bpgpu_linear_verify_rlc_ts.argtypes = [vp, sz, sz, u8p, sz, u8p, sz, u8p, u8p, u8p, u8p, u8p, i, u8p, u8p, u8p, u8p]
    L.bpgpu_linear_verify_rlc_ts_dev.argtypes = [vp, sz, sz, vp, sz, u8p, vp, vp, vp, vp, vp, vp, i, vp, vp, vp, vp, vp]
    L.bpgpu_ipp_create_batch_ts.argtypes = [vp, sz, sz, u8p, sz, u8p, u8p, u8p, u8p, u8p, i, u8p, u8p, u8p, u8p, u8p]
    L.bpgpu_linear_create_batch_ts.argtypes = [vp, sz, sz, u8p, sz, u8p, u8p, u8p, u8p, u8p, i, u8p, u8p, u8p, u8p, u8p, u8p]
    L.bpgpu_ipp_verification_scalars.argtypes = [vp, sz, sz, u8p, sz, u8p, sz, u8p, sz, u8p, u8p, u8p, u8p, u8p]
    L.bpgpu_mpc_state1_bytes.argtypes = [sz]
    L.bpgpu_mpc_state1_bytes.restype = sz
    L.bpgpu_mpc_state2_bytes.argtypes = [sz]
    L.bpgpu_mpc_state2_bytes.restype = sz
    L.bpgpu_mpc_party_bit_commit.argtypes = [vp, sz, sz, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), u8p, u8p, u8p, u8p]
    L.bpgpu_mpc_party_poly_commit.argtypes = [vp, sz, sz, u8p, u8p, i, u8p, u8p, u8p, u8p]
    L.bpgpu_mpc_party_proof_share.argtypes = [vp, sz, sz, u8p, u8p, i, u8p, u8p]
    L.bpgpu_mpc_party_bit_commit_seeded.argtypes = [vp, sz, sz, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), u8p, u8p, C.POINTER(C.c_uint64), u8p, u8p]
    L.bpgpu_mpc_party_poly_commit_seeded.argtypes = [vp, sz, sz, u8p, u8p, i, u8p, C.POINTER(C.c_uint64), u8p, u8p, u8p]
    L.bpgpu_mpc_dealer_bit_challenge.argtypes = [vp, sz, sz, sz, u8p, u8p, sz, u8p, sz, u8p, u8p, u8p, u8p]
    L.bpgpu_mpc_dealer_poly_challenge.argtypes = [vp, sz, sz, u8p, u8p, u8p, u8p, u8p]
    L.bpgpu_mpc_dealer_assemble.argtypes = [vp, sz, sz, sz, u8p, u8p, u8p, u8p, u8p, u8p, sz, u8p, sz, u8p, i, u8p, u8p, u8p]
    L.bpgpu_pedersen_commit_batch.argtypes = [vp, sz, u8p, sz, u8p, u8p, C.c_uint64, u8p, u8p, u8p]
    L.bpgpu_pedersen_open_batch.argtypes = [vp, sz, u8p, u8p, sz, u8p, u8p]
    L.bpgpu_pedersen_commit_batch_dev.argtypes = [vp, sz, vp, sz, vp, vp, C.c_uint64, vp, vp, vp, vp]
    L.bpgpu_pedersen_open_batch_dev.argtypes = [vp, sz, vp, vp, sz, vp, vp, vp]
    u32p = C.POINTER(C.c_uint32)
    L.bpgpu_pedersen_sum_batch.argtypes = [vp, sz, u32p, u8p, u8p, u8p, sz, u8p, u8p, u8p]
    L.bpgpu_pedersen_balance_batch.argtypes = [vp, sz, u32p, u8p, u8p, u8p, sz, u8p, u8p]
    L.bpgpu_pedersen_sum_batch_dev.argtypes = [vp, sz, u32p, vp, vp, vp, sz, vp, vp, vp, vp]
    L.bpgpu_pedersen_balance_batch_dev.argtypes = [vp, sz, u32p, vp, vp, vp, sz, vp, vp, vp]
    L.bpgpu_opening_create_batch_ts.argtypes = [vp, i, sz, u8p, sz, u8p, u8p, u8p, sz, u8p, u8p, u8p, u8p]
    L.bpgpu_opening_verify_batch_ts.argtypes = [vp, i, sz, u8p, sz, u8p, sz, u8p, u8p, sz, u8p, u8p, u8p]
    L.bpgpu_opening_verify_batch_ts_dev.argtypes = [vp, i, sz, vp, sz, u8p, vp, vp, vp, sz, vp, vp, vp, vp]
    L.bpgpu_opening_verify_rlc_ts.argtypes = [vp, i, sz, u8p, sz, u8p, sz, u8p, u8p, sz, u8p, u8p, u8p, u8p]
    L.bpgpu_opening_verify_rlc_ts_dev.argtypes = [vp, i, sz, vp, sz, u8p, vp, vp, vp, sz, vp, vp, vp, vp, vp]
    L.bpgpu_sigma_descriptor_check.argtypes = [u8p, sz, sz, u8p]
    L.bpgpu_sigma_relation_create.argtypes = [vp, u8p, sz, C.POINTER(vp)]
    L.bpgpu_sigma_relation_destroy.argtypes = [vp]
    L.bpgpu_sigma_relation_destroy.restype = None
    L.bpgpu_sigma_relation_shape.argtypes = [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), u8p]
    L.bpgpu_sigma_create_batch_ts.argtypes = [vp, vp, sz, u8p, sz, u8p, u8p, u8p, u8p, u8p, u8p]
    L.bpgpu_sigma_verify_batch_ts.argtypes = [vp, vp, sz, u8p, sz, u8p, sz, u8p, u8p, u8p, u8p]
    L.bpgpu_sigma_verify_batch_ts_dev.argtypes = [vp, vp, sz, vp, sz, u8p, vp, vp, vp, vp, vp, vp]
    L.bpgpu_sigma_verify_rlc_ts.argtypes = [vp, vp, sz, u8p, sz, u8p, sz, u8p, u8p, u8p, u8p, u8p]
    L.bpgpu_sigma_verify_rlc_ts_dev.argtypes = [vp, vp, sz, vp, sz, u8p, vp, vp, vp, vp, vp, vp, vp]
    L.bpgpu_rangeproof_prove_batch_rw.argtypes = [vp, sz, sz, sz, C.POINTER(C.c_uint64), u8p, u8p, sz, u8p, u8p, u8p, u8p, u8p]
    L.bpgpu_rangeproof_prove_batch_rw_dev.argtypes = [vp, sz, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp]
    L.bpgpu_rangeproof_rewind_batch.argtypes = [vp, sz, sz, u8p, sz, u8p, u8p, sz, u8p, u8p, C.POINTER(C.c_uint64), u8p, u8p]
    L.bpgpu_rangeproof_rewind_batch_dev.argtypes = [vp, sz, sz, vp, sz, vp, vp, sz, vp, vp, vp, vp, vp, vp]
    L.bpgpu_rangeproof_scan_batch.argtypes = [vp, sz, sz, u8p, sz, u8p, u8p, sz, u8p, sz, u8p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), u8p, u8p]
    L.bpgpu_rangeproof_scan_batch_dev.argtypes = [vp, sz, sz, vp, sz, vp, vp, sz, vp, sz, vp, vp, vp, vp, vp, vp]
    L.bpgpu_pool_create.argtypes = [C.POINTER(C.c_int), i, i, C.POINTER(vp)]
    L.bpgpu_pool_destroy.argtypes = [vp]
    L.bpgpu_pool_destroy.restype = None
    L.bpgpu_pool_last_error.argtypes = [vp]
    L.bpgpu_pool_last_error.restype = C.c_char_p
    L.bpgpu_pool_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    L.bpgpu_pool_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    L.bpgpu_pool_devices.argtypes = [vp]
    L.bpgpu_pool_lanes.argtypes = [vp]
    L.bpgpu_pool_lane.argtypes = [vp, i, i]
    L.bpgpu_pool_lane.restype = vp
    L.bpgpu_pool_gens_create.argtypes = [vp, sz, sz]
    L.bpgpu_gens_add_shape.argtypes = [vp, sz, sz]
    L.bpgpu_pool_gens_add_shape.argtypes = [vp, sz, sz]
    L.bpgpu_pool_gens_load.argtypes = [vp, sz, sz, u8p, u8p, u8p, u8p]
    L.bpgpu_pool_rangeproof_verify.argtypes = [vp, sz, sz, sz, u8p, sz, u8p, u8p, sz, u8p, u8p, u8p]
    L.bpgpu_pool_rangeproof_submit_dev.argtypes = [vp, i, sz, sz, sz, vp, sz, vp, u8p, sz, vp, vp, vp]
    L.bpgpu_pool_rangeproof_verify_ts.argtypes = [vp, sz, sz, sz, u8p, sz, u8p, u8p, sz, u8p, u8p, u8p, u8p]
    L.bpgpu_pool_rangeproof_submit_ts.argtypes = [vp, sz, sz, sz, u8p, sz, u8p, u8p, sz, u8p, u8p, u8p, u8p, C.POINTER(vp)]
    L.bpgpu_pool_rangeproof_submit_dev_ex.argtypes = [vp, i, sz, sz, sz, vp, sz, vp, u8p, sz, vp, vp, vp, vp, i, C.POINTER(vp)]
    L.bpgpu_pool_ticket_stream_wait.argtypes = [vp, vp, vp]
    L.bpgpu_pool_gather_dev.argtypes = [vp, i, C.POINTER(vp), C.POINTER(sz), vp, vp]
    L.bpgpu_pool_rangeproof_submit_rlc_dev.argtypes = [vp, i, sz, sz, sz, vp, sz, vp, u8p, sz, vp, vp, vp, vp, i, C.POINTER(vp)]
    L.bpgpu_pool_msm_batch_shared.argtypes = [vp, sz, sz, sz, sz, u8p, u8p, u8p, u8p, u8p]
    L.bpgpu_pool_msm_batch_shared_submit.argtypes = [vp, sz, sz, sz, sz, u8p, u8p, u8p, u8p, u8p, C.POINTER(vp)]
    L.bpgpu_pool_msm_batch.argtypes = [vp, sz, C.POINTER(C.c_uint32), u8p, u8p, u8p, u8p]
    L.bpgpu_pool_ipp_verify.argtypes = [vp, sz, sz, u8p, sz, u8p, sz, u8p, u8p, u8p, u8p, u8p, u8p, u8p, u8p]
    L.bpgpu_pool_msm_batch_shared_submit_dev.argtypes = [vp, i, sz, sz, sz, sz, vp, vp, vp, vp, vp, vp, i, C.POINTER(vp)]
    L.bpgpu_pool_trace_dump.argtypes = [vp, C.c_char_p]
    L.bpgpu_pool_ticket_done.argtypes = [vp, vp]
    L.bpgpu_pool_ticket_wait.argtypes = [vp, vp]
    L.bpgpu_pool_flush.argtypes = [vp]
    L.bpgpu_pool_wait.argtypes = [vp]
    L.bpgpu_profile_enable.argtypes = [vp, i]
    L.bpgpu_profile_reset.argtypes = [vp]
    L.bpgpu_profile_report.argtypes = [vp, C.c_char_p, sz]
    _lib = L
    return L


def transcript_new(label):
    """merlin::Transcript::new(label) as its 208-byte state (host-side helper of the library; needs no GPU)."""
    st = C.create_string_buffer(TRANSCRIPT_BYTES)
    if lib().bpgpu_transcript_new(label, len(label), st) != 0:
        raise BpgpuError("bpgpu_transcript_new failed")
    return st.raw


def transcript_append_message(state, label, msg):
    st = C.create_string_buffer(bytes(state), TRANSCRIPT_BYTES)
    if lib().bpgpu_transcript_append_message(st, label, len(label), msg, len(msg)) != 0:
        raise BpgpuError("bpgpu_transcript_append_message failed (malformed state?)")
    return st.raw


def transcript_challenge_bytes(state, label, n):
    st = C.create_string_buffer(bytes(state), TRANSCRIPT_BYTES)
    out = C.create_string_buffer(max(n, 1))
    if lib().bpgpu_transcript_challenge_bytes(st, label, len(label), out, n) != 0:
        raise BpgpuError("bpgpu_transcript_challenge_bytes failed (malformed state?)")
    return st.raw, out.raw[:n]


ERR_NAMES = {0: "OK", -1: "INVALID_ARG", -2: "HIP", -3: "NO_GENS", -4: "NO_DEVICE", -5: "BAD_GENERATOR", -6: "HW_QUEUES"}


def _rlc_mixed_call(fn, handle, groups, rng64, weights64):
    """bpgpu_[pool_]rangeproof_verify_rlc_mixed: groups = [(n, m, proofs, proof_len, commitments, label)]"""
    ng = len(groups)
    sz = C.c_size_t
    nbs = []
    for n, m, proofs, proof_len, commitments, label in groups:
        nb = len(proofs) // proof_len if proof_len else 0
        assert len(proofs) == nb * proof_len and len(commitments) == 32 * m * nb
        nbs.append(nb)
    total = sum(nbs)
    assert rng64 is None or len(rng64) == 64 * total
    assert weights64 is None or len(weights64) == 64 * total
    arr = lambda vals: (sz * max(ng, 1))(*vals)
    labels = (C.c_char_p * max(ng, 1))(*[bytes(g[5]) for g in groups])
    verdict = C.create_string_buffer(max(total, 1))
    bo = C.create_string_buffer(33)
    rc = fn(handle, ng, arr([g[0] for g in groups]), arr([g[1] for g in groups]), arr(nbs), arr([g[3] for g in groups]),
            b"".join(bytes(g[2]) for g in groups), b"".join(bytes(g[4]) for g in groups), labels, arr([len(g[5]) for g in groups]),
            rng64, weights64, verdict, bo)
    return rc, verdict.raw[:total], bo.raw[0] == 0, bo.raw[1:33]


def _rlc_mixed_ts_call(fn, handle, groups, rng64, weights64, want_transcripts):
    """bpgpu_[pool_]rangeproof_verify_rlc_mixed_ts: groups = [(n, m, proofs, proof_len, commitments, states)], states = ONE 208-byte state
    for the group or one per proof"""
    ng = len(groups)
    sz = C.c_size_t
    nbs, strides = [], []
    for n, m, proofs, proof_len, commitments, states in groups:
        nb = len(proofs) // proof_len if proof_len else 0
        assert len(proofs) == nb * proof_len and len(commitments) == 32 * m * nb
        assert len(states) in (TRANSCRIPT_BYTES, TRANSCRIPT_BYTES * nb)
        nbs.append(nb)
        strides.append(0 if (len(states) == TRANSCRIPT_BYTES and nb != 1) else TRANSCRIPT_BYTES)
    total = sum(nbs)
    assert rng64 is None or len(rng64) == 64 * total
    assert weights64 is None or len(weights64) == 64 * total
    arr = lambda vals: (sz * max(ng, 1))(*vals)
    verdict = C.create_string_buffer(max(total, 1))
    bo = C.create_string_buffer(33)
    tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(total, 1)) if want_transcripts else None
    rc = fn(handle, ng, arr([g[0] for g in groups]), arr([g[1] for g in groups]), arr(nbs), arr([g[3] for g in groups]),
            b"".join(bytes(g[2]) for g in groups), b"".join(bytes(g[4]) for g in groups), b"".join(bytes(g[5]) for g in groups) or bytes(1), arr(strides),
            rng64, weights64, verdict, bo, tso)
    out = (verdict.raw[:total], bo.raw[0] == 0, bo.raw[1:33])
    return rc, (out + (tso.raw[:TRANSCRIPT_BYTES * total],) if want_transcripts else out)


class Context:
    """Owns one bpgpu_ctx (one GPU)."""

    def __init__(self, device=0, fixed_window_bits=None, fixed_splits=None, fixed_table_max_bytes=None, horner_lanes=None):
        self._L = lib()
        h = C.c_void_p()
        rc = self._L.bpgpu_ctx_create(device, C.byref(h))
        if rc != 0:
            raise BpgpuError("bpgpu_ctx_create(device=%d) failed: %s (no CPU fallback)" % (device, ERR_NAMES.get(rc, rc)))
        self.h = h
        if fixed_window_bits is not None:
            self.set_option("fixed_window_bits", fixed_window_bits)
        if fixed_splits is not None:
            self.set_option("fixed_splits", fixed_splits)
        if fixed_table_max_bytes is not None:
            self.set_option("fixed_table_max_bytes", fixed_table_max_bytes)
        if horner_lanes is not None:
            self.set_option("horner_lanes", horner_lanes)

    def close(self):
        if getattr(self, "h", None):
            self._L.bpgpu_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise BpgpuError("%s: %s" % (ERR_NAMES.get(rc, rc), self._L.bpgpu_last_error(self.h).decode()))

    def set_option(self, key, value):
        self._chk(self._L.bpgpu_ctx_set_option(self.h, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_int64(0)
        self._chk(self._L.bpgpu_ctx_get_option(self.h, key.encode(), C.byref(v)))
        return v.value

    def synchronize(self):
        self._chk(self._L.bpgpu_synchronize(self.h))

    # ---- generators ----
    def gens_create(self, gens_capacity, party_capacity):
        self._chk(self._L.bpgpu_gens_create(self.h, gens_capacity, party_capacity))
        self.gens_capacity, self.party_capacity = gens_capacity, party_capacity

    def gens_add_shape(self, n2, m2):
        """a second, larger-window table for the smaller shape (n2, m2) (bpgpu_gens_add_shape)"""
        self._chk(self._L.bpgpu_gens_add_shape(self.h, n2, m2))

    def gens_load(self, gens_capacity, party_capacity, G, H, B, B_blinding):
        assert len(G) == len(H) == 32 * gens_capacity * party_capacity
        self._chk(self._L.bpgpu_gens_load(self.h, gens_capacity, party_capacity, G, H, B, B_blinding))
        self.gens_capacity, self.party_capacity = gens_capacity, party_capacity

    def gens_export(self):
        tot = self.gens_capacity * self.party_capacity
        G, H = C.create_string_buffer(32 * tot), C.create_string_buffer(32 * tot)
        B, Bb = C.create_string_buffer(32), C.create_string_buffer(32)
        self._chk(self._L.bpgpu_gens_export(self.h, G, H, B, Bb))
        return G.raw, H.raw, B.raw, Bb.raw

    # ---- MSM ----
    def msm_batch(self, n_terms, scalars, points):
        nb = len(n_terms)
        tot = sum(n_terms)
        assert len(scalars) == len(points) == 32 * tot
        nt = (C.c_uint32 * max(nb, 1))(*n_terms)
        out, st = C.create_string_buffer(32 * max(nb, 1)), C.create_string_buffer(max(nb, 1))
        self._chk(self._L.bpgpu_msm_batch(self.h, nb, nt, scalars, points, out, st))
        return out.raw[:32 * nb], st.raw[:nb]

    def msm_batch_shared(self, n, m, nbatch, n_unique, gen_scalars, uniq_scalars, uniq_points):
        assert len(gen_scalars) == 32 * (2 * n * m + 2) * nbatch
        assert len(uniq_scalars) == len(uniq_points) == 32 * n_unique * nbatch
        out, st = C.create_string_buffer(32 * max(nbatch, 1)), C.create_string_buffer(max(nbatch, 1))
        self._chk(self._L.bpgpu_msm_batch_shared(self.h, n, m, nbatch, n_unique, gen_scalars, uniq_scalars, uniq_points, out, st))
        return out.raw[:32 * nbatch], st.raw[:nbatch]

    # ---- range proofs ----
    def rangeproof_verify_batch(self, n, m, proofs, proof_len, commitments, label, rng64=None, want_msm=False):
        nb = len(proofs) // proof_len if proof_len else 0
        assert len(proofs) == nb * proof_len and len(commitments) == 32 * m * nb
        assert rng64 is None or len(rng64) == 64 * nb
        verdict = C.create_string_buffer(max(nb, 1))
        msm = C.create_string_buffer(32 * max(nb, 1)) if want_msm else None
        self._chk(self._L.bpgpu_rangeproof_verify_batch(self.h, n, m, nb, proofs, proof_len, commitments, label, len(label),
                                                        rng64, verdict, msm))
        return (verdict.raw[:nb], msm.raw[:32 * nb]) if want_msm else verdict.raw[:nb]

    def rangeproof_verify_batch_submit(self, n, m, proofs, proof_len, commitments, label, rng64=None):
        """Asynchronous bpgpu_rangeproof_verify_batch: returns at once; collect() returns the verdict bytes."""
        nb = len(proofs) // proof_len if proof_len else 0
        assert len(proofs) == nb * proof_len and len(commitments) == 32 * m * nb
        self._pending = (C.create_string_buffer(max(nb, 1)), nb)
        self._chk(self._L.bpgpu_rangeproof_verify_batch_submit(self.h, n, m, nb, proofs, proof_len, commitments, label, len(label), rng64,
                                                               self._pending[0], None))

    def collect(self):
        self._chk(self._L.bpgpu_ctx_collect(self.h))
        buf, nb = self._pending
        self._pending = None
        return buf.raw[:nb]

    def rangeproof_verify_batch_ts(self, n, m, proofs, proof_len, commitments, transcripts, rng64=None, want_msm=False,
                                   want_transcripts=False):
        """bpgpu_rangeproof_verify_batch_ts: `transcripts` is ONE 208-byte state shared by the batch, or nbatch of them.
        Returns verdict bytes [, msm encodings] [, advanced states]."""
        nb = len(proofs) // proof_len if proof_len else 0
        assert len(proofs) == nb * proof_len and len(commitments) == 32 * m * nb
        assert len(transcripts) in (TRANSCRIPT_BYTES, TRANSCRIPT_BYTES * nb)
        stride = 0 if (len(transcripts) == TRANSCRIPT_BYTES and nb != 1) else TRANSCRIPT_BYTES
        verdict = C.create_string_buffer(max(nb, 1))
        msm = C.create_string_buffer(32 * max(nb, 1)) if want_msm else None
        tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_rangeproof_verify_batch_ts(self.h, n, m, nb, proofs, proof_len, commitments, transcripts, stride,
                                                           rng64, verdict, msm, tso))
        out = [verdict.raw[:nb]]
        if want_msm:
            out.append(msm.raw[:32 * nb])
        if want_transcripts:
            out.append(tso.raw[:TRANSCRIPT_BYTES * nb])
        return out[0] if len(out) == 1 else tuple(out)

    def rangeproof_verify_rlc(self, n, m, proofs, proof_len, commitments, label, rng64=None, weights64=None):
        """Batch-combined verification (include/bpgpu.h): returns (verdict bytes, batch_ok, 32-byte encoding of the
        combined point).  On a failing combination the verdicts come from the per-proof path (automatic fallback)."""
        nb = len(proofs) // proof_len if proof_len else 0
        assert len(proofs) == nb * proof_len and len(commitments) == 32 * m * nb
        assert rng64 is None or len(rng64) == 64 * nb
        assert weights64 is None or len(weights64) == 64 * nb
        verdict = C.create_string_buffer(max(nb, 1))
        bo = C.create_string_buffer(33)
        self._chk(self._L.bpgpu_rangeproof_verify_rlc(self.h, n, m, nb, proofs, proof_len, commitments, label, len(label),
                                                      rng64, weights64, verdict, bo))
        return verdict.raw[:nb], bo.raw[0] == 0, bo.raw[1:33]

    def rangeproof_verify_rlc_mixed(self, groups, rng64=None, weights64=None):
        """Batch-combined verification of proofs of mixed shapes in ONE check (bpgpu_rangeproof_verify_rlc_mixed): groups is a list of
        (n, m, proofs, proof_len, commitments, label); rng64 / weights64: 64 bytes per proof in call order.  Returns (verdict bytes in
        call order, batch_ok, 32-byte encoding of the combined point), as rangeproof_verify_rlc."""
        rc, verdict, ok, enc = _rlc_mixed_call(self._L.bpgpu_rangeproof_verify_rlc_mixed, self.h, groups, rng64, weights64)
        self._chk(rc)
        return verdict, ok, enc

    def rangeproof_verify_rlc_ts(self, n, m, proofs, proof_len, commitments, transcripts, rng64=None, weights64=None, want_transcripts=False):
        """rangeproof_verify_rlc on the callers' own transcripts (bpgpu_rangeproof_verify_rlc_ts): `transcripts` is ONE 208-byte state
        shared by the batch, or nbatch of them (at any STROBE positions).  Returns (verdict bytes, batch_ok, 32-byte encoding of the
        combined point[, advanced states])."""
        nb = len(proofs) // proof_len if proof_len else 0
        assert len(proofs) == nb * proof_len and len(commitments) == 32 * m * nb
        assert len(transcripts) in (TRANSCRIPT_BYTES, TRANSCRIPT_BYTES * nb)
        assert rng64 is None or len(rng64) == 64 * nb
        assert weights64 is None or len(weights64) == 64 * nb
        stride = 0 if (len(transcripts) == TRANSCRIPT_BYTES and nb != 1) else TRANSCRIPT_BYTES
        verdict = C.create_string_buffer(max(nb, 1))
        bo = C.create_string_buffer(33)
        tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_rangeproof_verify_rlc_ts(self.h, n, m, nb, proofs, proof_len, commitments, transcripts, stride, rng64, weights64,
                                                         verdict, bo, tso))
        out = (verdict.raw[:nb], bo.raw[0] == 0, bo.raw[1:33])
        return out + (tso.raw[:TRANSCRIPT_BYTES * nb],) if want_transcripts else out

    def rangeproof_verify_rlc_mixed_ts(self, groups, rng64=None, weights64=None, want_transcripts=False):
        """rangeproof_verify_rlc_mixed on the callers' own transcripts (bpgpu_rangeproof_verify_rlc_mixed_ts): groups is a list of
        (n, m, proofs, proof_len, commitments, states), states = ONE 208-byte state for the group or one per proof.  Returns (verdict
        bytes in call order, batch_ok, 32-byte encoding of the combined point[, advanced states in call order])."""
        rc, out = _rlc_mixed_ts_call(self._L.bpgpu_rangeproof_verify_rlc_mixed_ts, self.h, groups, rng64, weights64, want_transcripts)
        self._chk(rc)
        return out

    # ---- stand-alone inner-product proofs ----
    def ipp_verify_batch(self, n, proofs, proof_len, label, Gf, Hf, P, Q, G, H, want_msm=False):
        nb = len(proofs) // proof_len if proof_len else 0
        assert len(Gf) == len(Hf) == len(G) == len(H) == 32 * n * nb and len(P) == len(Q) == 32 * nb
        verdict = C.create_string_buffer(max(nb, 1))
        msm = C.create_string_buffer(32 * max(nb, 1)) if want_msm else None
        self._chk(self._L.bpgpu_ipp_verify_batch(self.h, n, nb, proofs, proof_len, label, len(label), Gf, Hf, P, Q, G, H, verdict, msm))
        return (verdict.raw[:nb], msm.raw[:32 * nb]) if want_msm else verdict.raw[:nb]

    def ipp_verify_rlc(self, n, proofs, proof_len, Gf, Hf, P, Q, G, H, label=b"", transcript=None, gens_m=1, weights64=None):
        """Batch-combined InnerProductProof verification (bpgpu_ipp_verify_rlc) of len(P) / 32 proofs.  G, H: n points each, shared by
        the batch, or both None: the context's G(n / gens_m, gens_m), H(n / gens_m, gens_m) through the window tables.  weights64: 64
        bytes per proof or None (drawn by the library).  Returns (verdict bytes, batch_ok, 32-byte encoding of the combined point).  On
        a failing combination the verdicts come from the per-proof path (automatic fallback)."""
        nb = len(P) // 32
        assert len(proofs) == nb * proof_len and len(Gf) == len(Hf) == 32 * n * nb and len(Q) == 32 * nb
        assert G is None or len(G) == 32 * n
        assert H is None or len(H) == 32 * n
        assert weights64 is None or len(weights64) == 64 * nb
        verdict = C.create_string_buffer(max(nb, 1))
        bo = C.create_string_buffer(33)
        self._chk(self._L.bpgpu_ipp_verify_rlc(self.h, n, nb, proofs, proof_len, label, len(label), transcript, Gf, Hf, P, Q, G, H, gens_m,
                                               weights64, verdict, bo))
        return verdict.raw[:nb], bo.raw[0] == 0, bo.raw[1:33]

    def ipp_verification_scalars(self, n, proofs, proof_len, label=b"", transcripts=None, want_transcripts=False):
        """InnerProductProof::verification_scalars for len(proofs) / proof_len proofs (bpgpu_ipp_verification_scalars): returns
        (u_sq bytes, u_inv_sq bytes, s bytes, status bytes[, advanced transcripts])."""
        nb = len(proofs) // proof_len if proof_len else 0
        k = max(0, (proof_len // 32 - 2) // 2)
        stride = 0
        if transcripts is not None:
            assert len(transcripts) in (TRANSCRIPT_BYTES, TRANSCRIPT_BYTES * nb)
            stride = 0 if (len(transcripts) == TRANSCRIPT_BYTES and nb != 1) else TRANSCRIPT_BYTES
        us, ui = C.create_string_buffer(32 * max(k * nb, 1)), C.create_string_buffer(32 * max(k * nb, 1))
        s_, st = C.create_string_buffer(32 * max(n * nb, 1)), C.create_string_buffer(max(nb, 1))
        tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_ipp_verification_scalars(self.h, n, nb, proofs, proof_len, label, len(label), transcripts, stride, us, ui, s_, tso, st))
        out = (us.raw[:32 * k * nb], ui.raw[:32 * k * nb], s_.raw[:32 * n * nb], st.raw[:nb])
        return out + (tso.raw[:TRANSCRIPT_BYTES * nb],) if want_transcripts else out

    def rangeproof_audit_shares(self, n, party_index, shares, bit_commitments, poly_commitments, challenges, want_checks=False):
        """ProofShare::audit_share for len(party_index) shares (bpgpu_rangeproof_audit_shares); challenges: 96 bytes shared or per share."""
        ns = len(party_index)
        assert len(shares) == ns * 32 * (3 + 2 * n) and len(bit_commitments) == 96 * ns and len(poly_commitments) == 64 * ns
        assert len(challenges) in (96, 96 * ns)
        shared = 1 if (len(challenges) == 96 and ns != 1) else 0
        pi = (C.c_uint32 * max(ns, 1))(*party_index)
        verdict = C.create_string_buffer(max(ns, 1))
        chk = C.create_string_buffer(64 * max(ns, 1)) if want_checks else None
        self._chk(self._L.bpgpu_rangeproof_audit_shares(self.h, n, ns, pi, shares, bit_commitments, poly_commitments, challenges, shared, verdict, chk))
        return (verdict.raw[:ns], chk.raw[:64 * ns]) if want_checks else verdict.raw[:ns]

    def linear_verify_batch(self, n, proofs, proof_len, Cs, G, F, B, b, label=b"", transcript=None, want_msm=False, want_transcripts=False):
        """LinearProof::verify for len(Cs) / 32 proofs (bpgpu_linear_verify_batch).  G: n points shared by the batch; b: per-proof
        vectors (nb * n scalars) or one shared vector (n scalars)."""
        nb = len(Cs) // 32
        assert len(proofs) == nb * proof_len and len(b) in (32 * n, 32 * n * nb)
        assert (G is None and F is None and B is None) or (len(G) == 32 * n and len(F) == len(B) == 32)   # None: the context's generators
        shared = 1 if (len(b) == 32 * n and nb != 1) else 0
        verdict = C.create_string_buffer(max(nb, 1))
        msm = C.create_string_buffer(32 * max(nb, 1)) if want_msm else None
        tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_linear_verify_batch(self.h, n, nb, proofs, proof_len, label, len(label), transcript, Cs, G, F, B, b, shared,
                                                    verdict, msm, tso))
        out = (verdict.raw[:nb],) + ((msm.raw[:32 * nb],) if want_msm else ()) + ((tso.raw[:TRANSCRIPT_BYTES * nb],) if want_transcripts else ())
        return out if len(out) > 1 else out[0]

    def linear_verify_rlc(self, n, proofs, proof_len, Cs, G, F, B, b, label=b"", transcript=None, weights64=None, want_transcripts=False):
        """Batch-combined LinearProof verification (bpgpu_linear_verify_rlc): arguments as linear_verify_batch, weights64: 64 bytes per
        proof or None (drawn by the library).  Returns (verdict bytes, batch_ok, 32-byte encoding of the combined point[, transcripts]).
        On a failing combination the verdicts come from the per-proof path (automatic fallback)."""
        nb = len(Cs) // 32
        assert len(proofs) == nb * proof_len and len(b) in (32 * n, 32 * n * nb)
        assert (G is None and F is None and B is None) or (len(G) == 32 * n and len(F) == len(B) == 32)   # None: the context's generators
        assert weights64 is None or len(weights64) == 64 * nb
        shared = 1 if (len(b) == 32 * n and nb != 1) else 0
        verdict = C.create_string_buffer(max(nb, 1))
        bo = C.create_string_buffer(33)
        tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_linear_verify_rlc(self.h, n, nb, proofs, proof_len, label, len(label), transcript, Cs, G, F, B, b, shared,
                                                  weights64, verdict, bo, tso))
        out = (verdict.raw[:nb], bo.raw[0] == 0, bo.raw[1:33])
        return out + (tso.raw[:TRANSCRIPT_BYTES * nb],) if want_transcripts else out

    def linear_create_batch(self, n, Cs, rs, a, b, G, F, B, label=b"", transcript=None, rng=None, want_transcripts=False):
        """LinearProof::create for len(Cs) / 32 proofs (bpgpu_linear_create_batch): returns (proofs bytes, status bytes[, transcripts])."""
        nb = len(Cs) // 32
        assert len(rs) == 32 * nb and len(a) == 32 * n * nb and len(b) in (32 * n, 32 * n * nb)
        assert (G is None and F is None and B is None) or (len(G) == 32 * n and len(F) == len(B) == 32)   # None: the context's generators
        shared = 1 if (len(b) == 32 * n and nb != 1) else 0
        lg = n.bit_length() - 1
        assert rng is None or len(rng) == 64 * (2 * lg + 2) * nb
        pl = 32 * (2 * lg + 3)
        out, st = C.create_string_buffer(pl * max(nb, 1)), C.create_string_buffer(max(nb, 1))
        tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_linear_create_batch(self.h, n, nb, label, len(label), transcript, rng, Cs, rs, a, b, shared, G, F, B, out, st, tso))
        res = (out.raw[:pl * nb], st.raw[:nb])
        return res + (tso.raw[:TRANSCRIPT_BYTES * nb],) if want_transcripts else res

    def ipp_create_batch(self, n, Q, Gf, Hf, G, H, a, b, label=b"", transcript=None):
        """InnerProductProof::create for nbatch proofs (bpgpu_ipp_create_batch).  G/H of n*32 bytes = bases shared by the batch.
        Returns (proofs bytes, status bytes)."""
        nb = len(Q) // 32
        assert len(a) == len(b) == len(Gf) == len(Hf) == 32 * n * nb and len(G) == len(H) and len(G) in (32 * n, 32 * n * nb)
        shared = 1 if (len(G) == 32 * n and nb != 1) else 0
        pl = 32 * (2 * (n.bit_length() - 1) + 2)
        out, st = C.create_string_buffer(pl * max(nb, 1)), C.create_string_buffer(max(nb, 1))
        self._chk(self._L.bpgpu_ipp_create_batch(self.h, n, nb, label, len(label), transcript, Q, Gf, Hf, G, H, shared, a, b, out, st))
        return out.raw[:pl * nb], st.raw[:nb]

    # ---- inner-product and linear proofs on the callers' own transcripts (bpgpu_*_ts) ----
    @staticmethod
    def _ts_stride(transcripts, nb):
        """transcripts: ONE 208-byte state (before innerproduct_domain_sep) for every proof, or one per proof"""
        assert transcripts is not None and len(transcripts) in (TRANSCRIPT_BYTES, TRANSCRIPT_BYTES * nb)
        return TRANSCRIPT_BYTES if (nb != 1 and len(transcripts) == TRANSCRIPT_BYTES * nb) else 0

    def ipp_verify_batch_ts(self, n, proofs, proof_len, transcripts, Gf, Hf, P, Q, G, H, want_msm=False, want_transcripts=False):
        """InnerProductProof::verify of len(P) / 32 proofs, each on its caller's own transcript (bpgpu_ipp_verify_batch_ts).  G, H: n points
        each shared by the batch, or n per proof."""
        nb = len(P) // 32
        assert len(proofs) == nb * proof_len and len(Gf) == len(Hf) == 32 * n * nb and len(Q) == 32 * nb
        assert len(G) == len(H) and len(G) in (32 * n, 32 * n * nb)
        shared = 1 if (len(G) == 32 * n and nb != 1) else 0
        verdict = C.create_string_buffer(max(nb, 1))
        msm = C.create_string_buffer(32 * max(nb, 1)) if want_msm else None
        tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_ipp_verify_batch_ts(self.h, n, nb, proofs, proof_len, transcripts, self._ts_stride(transcripts, nb), Gf, Hf, P, Q, G, H,
                                                    shared, verdict, msm, tso))
        out = (verdict.raw[:nb],) + ((msm.raw[:32 * nb],) if want_msm else ()) + ((tso.raw[:TRANSCRIPT_BYTES * nb],) if want_transcripts else ())
        return out if len(out) > 1 else out[0]

    def ipp_verify_rlc_ts(self, n, proofs, proof_len, transcripts, Gf, Hf, P, Q, G, H, gens_m=1, weights64=None, want_transcripts=False):
        """ipp_verify_rlc on the callers' own transcripts (bpgpu_ipp_verify_rlc_ts).  Returns (verdict bytes, batch_ok, 32-byte encoding of
        the combined point[, transcripts])."""
        nb = len(P) // 32
        assert len(proofs) == nb * proof_len and len(Gf) == len(Hf) == 32 * n * nb and len(Q) == 32 * nb
        assert (G is None and H is None) or len(G) == len(H) == 32 * n
        assert weights64 is None or len(weights64) == 64 * nb
        verdict = C.create_string_buffer(max(nb, 1))
        bo = C.create_string_buffer(33)
        tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_ipp_verify_rlc_ts(self.h, n, nb, proofs, proof_len, transcripts, self._ts_stride(transcripts, nb), Gf, Hf, P, Q, G, H,
                                                  gens_m, weights64, verdict, bo, tso))
        out = (verdict.raw[:nb], bo.raw[0] == 0, bo.raw[1:33])
        return out + (tso.raw[:TRANSCRIPT_BYTES * nb],) if want_transcripts else out

    def linear_verify_batch_ts(self, n, proofs, proof_len, transcripts, Cs, G, F, B, b, want_msm=False, want_transcripts=False):
        """linear_verify_batch on the callers' own transcripts (bpgpu_linear_verify_batch_ts)."""
        nb = len(Cs) // 32
        assert len(proofs) == nb * proof_len and len(b) in (32 * n, 32 * n * nb)
        assert (G is None and F is None and B is None) or (len(G) == 32 * n and len(F) == len(B) == 32)   # None: the context's generators
        shared = 1 if (len(b) == 32 * n and nb != 1) else 0
        verdict = C.create_string_buffer(max(nb, 1))
        msm = C.create_string_buffer(32 * max(nb, 1)) if want_msm else None
        tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_linear_verify_batch_ts(self.h, n, nb, proofs, proof_len, transcripts, self._ts_stride(transcripts, nb), Cs, G, F, B, b,
                                                       shared, verdict, msm, tso))
        out = (verdict.raw[:nb],) + ((msm.raw[:32 * nb],) if want_msm else ()) + ((tso.raw[:TRANSCRIPT_BYTES * nb],) if want_transcripts else ())
        return out if len(out) > 1 else out[0]

    def linear_verify_rlc_ts(self, n, proofs, proof_len, transcripts, Cs, G, F, B, b, weights64=None, want_transcripts=False):
        """linear_verify_rlc on the callers' own transcripts (bpgpu_linear_verify_rlc_ts).  Returns (verdict bytes, batch_ok, 32-byte encoding
        of the combined point[, transcripts])."""
        nb = len(Cs) // 32
        assert len(proofs) == nb * proof_len and len(b) in (32 * n, 32 * n * nb)
        assert (G is None and F is None and B is None) or (len(G) == 32 * n and len(F) == len(B) == 32)
        assert weights64 is None or len(weights64) == 64 * nb
        shared = 1 if (len(b) == 32 * n and nb != 1) else 0
        verdict = C.create_string_buffer(max(nb, 1))
        bo = C.create_string_buffer(33)
        tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_linear_verify_rlc_ts(self.h, n, nb, proofs, proof_len, transcripts, self._ts_stride(transcripts, nb), Cs, G, F, B, b,
                                                     shared, weights64, verdict, bo, tso))
        out = (verdict.raw[:nb], bo.raw[0] == 0, bo.raw[1:33])
        return out + (tso.raw[:TRANSCRIPT_BYTES * nb],) if want_transcripts else out

    def ipp_create_batch_ts(self, n, transcripts, Q, Gf, Hf, G, H, a, b, want_transcripts=False):
        """ipp_create_batch on the callers' own transcripts (bpgpu_ipp_create_batch_ts): returns (proofs bytes, status bytes[, the states as
        create() leaves them])."""
        nb = len(Q) // 32
        assert len(a) == len(b) == len(Gf) == len(Hf) == 32 * n * nb and len(G) == len(H) and len(G) in (32 * n, 32 * n * nb)
        shared = 1 if (len(G) == 32 * n and nb != 1) else 0
        pl = 32 * (2 * (n.bit_length() - 1) + 2)
        out, st = C.create_string_buffer(pl * max(nb, 1)), C.create_string_buffer(max(nb, 1))
        tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_ipp_create_batch_ts(self.h, n, nb, transcripts, self._ts_stride(transcripts, nb), Q, Gf, Hf, G, H, shared, a, b, out, st,
                                                    tso))
        res = (out.raw[:pl * nb], st.raw[:nb])
        return res + (tso.raw[:TRANSCRIPT_BYTES * nb],) if want_transcripts else res

    def linear_create_batch_ts(self, n, transcripts, Cs, rs, a, b, G, F, B, rng32=None, want_transcripts=False):
        """linear_create_batch on the callers' own transcripts, the random scalars drawn on the device (bpgpu_linear_create_batch_ts).
        rng32: 32 bytes per proof, the seed of its ChaChaRng (None: the library draws them).  Returns (proofs bytes, status bytes[,
        transcripts])."""
        nb = len(Cs) // 32
        assert len(rs) == 32 * nb and len(a) == 32 * n * nb and len(b) in (32 * n, 32 * n * nb)
        assert (G is None and F is None and B is None) or (len(G) == 32 * n and len(F) == len(B) == 32)
        assert rng32 is None or len(rng32) == 32 * nb
        shared = 1 if (len(b) == 32 * n and nb != 1) else 0
        pl = 32 * (2 * (n.bit_length() - 1) + 3)
        out, st = C.create_string_buffer(pl * max(nb, 1)), C.create_string_buffer(max(nb, 1))
        tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_linear_create_batch_ts(self.h, n, nb, transcripts, self._ts_stride(transcripts, nb), rng32, Cs, rs, a, b, shared, G, F,
                                                       B, out, st, tso))
        res = (out.raw[:pl * nb], st.raw[:nb])
        return res + (tso.raw[:TRANSCRIPT_BYTES * nb],) if want_transcripts else res

    def rangeproof_prove_batch(self, n, m, values, blindings, label=b"", transcript=None, rng=None, want_transcripts=False):
        """RangeProof::prove_multiple_with_rng for len(values) / m proofs (bpgpu_rangeproof_prove_batch): returns
        (proofs bytes, commitments bytes[, final transcript states])."""
        nb = len(values) // m
        assert len(values) == nb * m and len(blindings) == 32 * nb * m
        per = 64 * (m * (2 * n + 2) + 2 * m)
        assert rng is None or len(rng) == per * nb
        pl = 32 * (9 + 2 * ((n * m).bit_length() - 1))
        va = (C.c_uint64 * max(len(values), 1))(*values)
        proofs, coms = C.create_string_buffer(pl * max(nb, 1)), C.create_string_buffer(32 * m * max(nb, 1))
        tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_rangeproof_prove_batch(self.h, n, m, nb, va, blindings, label, len(label), transcript, rng, proofs, coms, tso))
        out = (proofs.raw[:pl * nb], coms.raw[:32 * m * nb])
        return out + (tso.raw[:TRANSCRIPT_BYTES * nb],) if want_transcripts else out

    def rangeproof_prove_batch_ts(self, n, m, values, blindings, transcripts, rng32=None, want_transcripts=False):
        """The same proofs on the callers' own transcripts, the random scalars drawn on the device (bpgpu_rangeproof_prove_batch_ts).
        transcripts: one 208-byte state (before rangeproof_domain_sep) shared by every proof, or one per proof; rng32: 32 bytes per
        proof, the seed of its ChaChaRng (None: the library draws them).  Returns (proofs bytes, commitments bytes[, final states])."""
        nb = len(values) // m
        assert len(values) == nb * m and len(blindings) == 32 * nb * m
        assert transcripts is None or len(transcripts) in (TRANSCRIPT_BYTES, TRANSCRIPT_BYTES * nb)
        assert rng32 is None or len(rng32) == 32 * nb
        stride = TRANSCRIPT_BYTES if (transcripts is not None and nb != 1 and len(transcripts) == TRANSCRIPT_BYTES * nb) else 0
        pl = 32 * (9 + 2 * ((n * m).bit_length() - 1))
        va = (C.c_uint64 * max(len(values), 1))(*values)
        proofs, coms = C.create_string_buffer(pl * max(nb, 1)), C.create_string_buffer(32 * m * max(nb, 1))
        tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_rangeproof_prove_batch_ts(self.h, n, m, nb, va, blindings, transcripts, stride, rng32, proofs, coms, tso))
        out = (proofs.raw[:pl * nb], coms.raw[:32 * m * nb])
        return out + (tso.raw[:TRANSCRIPT_BYTES * nb],) if want_transcripts else out

    def rangeproof_prove_batch_ts_dev(self, n, m, nbatch, d_values, d_blindings, d_transcripts, transcript_stride, d_rng32, d_proofs, d_commitments,
                                      d_transcripts_out=None, stream=None):
        """bpgpu_rangeproof_prove_batch_ts_dev: every buffer a device address (int), asynchronous on `stream`."""
        self._chk(self._L.bpgpu_rangeproof_prove_batch_ts_dev(self.h, n, m, nbatch, d_values, d_blindings, d_transcripts, transcript_stride, d_rng32, d_proofs,
                                                              d_commitments, d_transcripts_out, stream))

    # ---- rewindable range proofs (bpgpu_rangeproof_prove_batch_rw / _rewind_batch) ----
    def rangeproof_prove_batch_rw(self, n, m, values, blindings, transcripts, rng32, messages=None, want_transcripts=False):
        """rangeproof_prove_batch_ts with a_blinding = draw 0 - (value + 2^64 message): whoever holds rng32[p] gets value, message and
        blinding back with rangeproof_rewind_batch (bpgpu_rangeproof_prove_batch_rw).  m must be 1 and rng32 is required; messages: 16
        bytes per proof, or None (every message 0).  Returns (proofs bytes, commitments bytes[, final states])."""
        nb = len(values) // max(m, 1)
        assert len(values) == nb * m and len(blindings) == 32 * nb * m
        assert transcripts is None or len(transcripts) in (TRANSCRIPT_BYTES, TRANSCRIPT_BYTES * nb)
        assert (rng32 is None or len(rng32) == 32 * nb) and (messages is None or len(messages) == 16 * nb)
        stride = TRANSCRIPT_BYTES if (transcripts is not None and nb != 1 and len(transcripts) == TRANSCRIPT_BYTES * nb) else 0
        pl = 32 * (9 + 2 * ((n * m).bit_length() - 1))
        va = (C.c_uint64 * max(len(values), 1))(*values)
        proofs, coms = C.create_string_buffer(pl * max(nb, 1)), C.create_string_buffer(32 * m * max(nb, 1))
        tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_rangeproof_prove_batch_rw(self.h, n, m, nb, va, blindings, transcripts, stride, rng32,
                                                          None if messages is None else bytes(messages), proofs, coms, tso))
        out = (proofs.raw[:pl * nb], coms.raw[:32 * m * nb])
        return out + (tso.raw[:TRANSCRIPT_BYTES * nb],) if want_transcripts else out

    def rangeproof_prove_batch_rw_dev(self, n, m, nbatch, d_values, d_blindings, d_transcripts, transcript_stride, d_rng32, d_messages, d_proofs,
                                      d_commitments, d_transcripts_out=None, stream=None):
        """bpgpu_rangeproof_prove_batch_rw_dev: every buffer a device address (int; d_messages may be None), asynchronous on `stream`."""
        self._chk(self._L.bpgpu_rangeproof_prove_batch_rw_dev(self.h, n, m, nbatch, d_values, d_blindings, d_transcripts, transcript_stride, d_rng32, d_messages,
                                                              d_proofs, d_commitments, d_transcripts_out, stream))

    def rangeproof_rewind_batch(self, n, proofs, proof_len, commitments, transcripts, rng32):
        """Rewind len(commitments) / 32 (proof, commitment) rows under the seeds rng32 (bpgpu_rangeproof_rewind_batch): one launch, lane =
        row.  transcripts: one 208-byte state (before rangeproof_domain_sep) shared by every row, or one per row.  Returns (status
        bytes, [values], messages bytes (16 per row), blindings bytes (32 per row)); a row's data is zero unless its status is
        REWIND_OK.  This does not verify the proofs."""
        nb = len(commitments) // 32
        assert len(commitments) == 32 * nb and len(proofs) == nb * proof_len and len(rng32) == 32 * nb
        st, va = C.create_string_buffer(max(nb, 1)), (C.c_uint64 * max(nb, 1))()
        msg, bl = C.create_string_buffer(16 * max(nb, 1)), C.create_string_buffer(32 * max(nb, 1))
        self._chk(self._L.bpgpu_rangeproof_rewind_batch(self.h, n, nb, bytes(proofs), proof_len, bytes(commitments), transcripts,
                                                        self._ts_stride(transcripts, nb), bytes(rng32), st, va, msg, bl))
        return st.raw[:nb], list(va)[:nb], msg.raw[:16 * nb], bl.raw[:32 * nb]

    def rangeproof_rewind_batch_dev(self, n, nbatch, d_proofs, proof_len, d_commitments, d_transcripts, transcript_stride, d_rng32, d_status, d_values,
                                    d_messages, d_blindings, stream=None):
        """bpgpu_rangeproof_rewind_batch_dev: every buffer a device address (int), asynchronous on `stream`."""
        self._chk(self._L.bpgpu_rangeproof_rewind_batch_dev(self.h, n, nbatch, d_proofs, proof_len, d_commitments, d_transcripts, transcript_stride, d_rng32,
                                                            d_status, d_values, d_messages, d_blindings, stream))

    # ---- scanning under many keys (bpgpu_rangeproof_scan_batch) ----
    def rangeproof_scan_batch(self, n, proofs, proof_len, commitments, transcripts, keys32):
        """Scan len(commitments) / 32 (proof, commitment) rows under the len(keys32) / 32 wallet keys, replaying each row's transcript
        once (bpgpu_rangeproof_scan_batch).  transcripts as in rangeproof_rewind_batch.  Returns (status bytes, [key indices], [values],
        messages bytes, blindings bytes): a row's key index is 0xFFFFFFFF and its data zero unless its status is REWIND_OK.  This does
        not verify the proofs."""
        nb, nk = len(commitments) // 32, len(keys32) // 32
        assert len(commitments) == 32 * nb and len(proofs) == nb * proof_len and len(keys32) == 32 * nk
        st, va, ki = C.create_string_buffer(max(nb, 1)), (C.c_uint64 * max(nb, 1))(), (C.c_uint32 * max(nb, 1))()
        msg, bl = C.create_string_buffer(16 * max(nb, 1)), C.create_string_buffer(32 * max(nb, 1))
        self._chk(self._L.bpgpu_rangeproof_scan_batch(self.h, n, nb, bytes(proofs), proof_len, bytes(commitments), transcripts,
                                                      self._ts_stride(transcripts, nb), bytes(keys32), nk, st, ki, va, msg, bl))
        return st.raw[:nb], list(ki)[:nb], list(va)[:nb], msg.raw[:16 * nb], bl.raw[:32 * nb]

    def rangeproof_scan_batch_dev(self, n, nbatch, d_proofs, proof_len, d_commitments, d_transcripts, transcript_stride, d_keys32, nkeys, d_status, d_key_index,
                                  d_values, d_messages, d_blindings, stream=None):
        """bpgpu_rangeproof_scan_batch_dev: every buffer a device address (int), asynchronous on `stream`."""
        self._chk(self._L.bpgpu_rangeproof_scan_batch_dev(self.h, n, nbatch, d_proofs, proof_len, d_commitments, d_transcripts, transcript_stride, d_keys32, nkeys,
                                                          d_status, d_key_index, d_values, d_messages, d_blindings, stream))

    # ---- batches of Pedersen commitments and openings (bpgpu_pedersen_commit_batch / _open_batch) ----
    def pedersen_commit_batch(self, values, value_bytes, blindings=None, rng_seed32=None, first_draw=0, want_blindings=False):
        """len(values) / value_bytes commitments value B + blinding B_blinding in one launch.  values: packed little-endian u64
        (value_bytes = 8) or 32-byte scalars (32).  blindings: 32 bytes per row, or None: row i takes draw first_draw + i of
        ChaChaRng::from_seed(rng_seed32) (rng_seed32 None: the library draws the seed, and the blindings are always returned).
        Returns (commitments bytes, status bytes[, blindings bytes])."""
        assert value_bytes in (8, 32) and len(values) % value_bytes == 0
        nb = len(values) // value_bytes
        assert blindings is None or len(blindings) == 32 * nb
        assert rng_seed32 is None or len(rng_seed32) == 32
        want_blindings = want_blindings or (blindings is None and rng_seed32 is None)
        out, st = C.create_string_buffer(32 * max(nb, 1)), C.create_string_buffer(max(nb, 1))
        blo = C.create_string_buffer(32 * max(nb, 1)) if want_blindings else None
        self._chk(self._L.bpgpu_pedersen_commit_batch(self.h, nb, bytes(values), value_bytes, blindings, rng_seed32, first_draw, out, blo, st))
        res = (out.raw[:32 * nb], st.raw[:nb])
        return res + (blo.raw[:32 * nb],) if want_blindings else res

    def pedersen_open_batch(self, commitments, values, value_bytes, blindings):
        """does (values[i], blindings[i]) open commitments[i]?  Returns the verdict bytes: 0 yes, 1 no (VerificationError: also a
        commitment that is no valid encoding), 2 a non-canonical scalar (FormatError)."""
        assert value_bytes in (8, 32) and len(values) % value_bytes == 0
        nb = len(values) // value_bytes
        assert len(commitments) == len(blindings) == 32 * nb
        vd = C.create_string_buffer(max(nb, 1))
        self._chk(self._L.bpgpu_pedersen_open_batch(self.h, nb, bytes(commitments), bytes(values), value_bytes, bytes(blindings), vd))
        return vd.raw[:nb]

    def pedersen_commit_batch_dev(self, nbatch, d_values, value_bytes, d_blindings, d_rng_seed32, first_draw, d_commitments, d_blindings_out, d_status,
                                  stream=None):
        """bpgpu_pedersen_commit_batch_dev: every buffer a device address (int, or None), asynchronous on `stream`."""
        self._chk(self._L.bpgpu_pedersen_commit_batch_dev(self.h, nbatch, d_values, value_bytes, d_blindings, d_rng_seed32, first_draw, d_commitments,
                                                          d_blindings_out, d_status, stream))

    def pedersen_open_batch_dev(self, nbatch, d_commitments, d_values, value_bytes, d_blindings, d_verdict, stream=None):
        """bpgpu_pedersen_open_batch_dev: every buffer a device address (int), asynchronous on `stream`."""
        self._chk(self._L.bpgpu_pedersen_open_batch_dev(self.h, nbatch, d_commitments, d_values, value_bytes, d_blindings, d_verdict, stream))

    # ---- signed sums of commitments and the balance check (bpgpu_pedersen_sum_batch / _balance_batch) ----
    @staticmethod
    def _psum_args(row_offsets, points, signs, values, value_bytes, blindings):
        row_offsets = [int(x) for x in row_offsets]
        nb = len(row_offsets) - 1
        assert nb >= 0 and (points is None or len(points) == 32 * row_offsets[-1]) and (signs is None or len(signs) == row_offsets[-1])
        assert values is None or len(values) == value_bytes * nb
        assert blindings is None or len(blindings) == 32 * nb
        b = lambda x: None if x is None else bytes(x)
        return nb, (C.c_uint32 * (nb + 1))(*row_offsets), b(points), b(signs), b(values), b(blindings)

    def pedersen_sum_batch(self, row_offsets, points, signs=None, values=None, value_bytes=8, blindings=None):
        """Row r: compress(sum of +-points[row_offsets[r] : row_offsets[r + 1]] + values[r] B + blindings[r] B_blinding).  points: 32
        bytes per term; signs: one byte per term (0 add, 1 subtract) or None; values: packed u64 (value_bytes = 8) or 32-byte scalars
        (32), or None; blindings: 32 bytes per row, or None.  Returns (32 bytes per row, BPGPU_MSM_* status bytes)."""
        nb, off, points, signs, values, blindings = self._psum_args(row_offsets, points, signs, values, value_bytes, blindings)
        out, st = C.create_string_buffer(32 * max(nb, 1)), C.create_string_buffer(max(nb, 1))
        self._chk(self._L.bpgpu_pedersen_sum_batch(self.h, nb, off, points, signs, values, value_bytes, blindings, out, st))
        return out.raw[:32 * nb], st.raw[:nb]

    def pedersen_balance_batch(self, row_offsets, points, signs=None, values=None, value_bytes=8, blindings=None):
        """Does the signed sum of row r's points open to (values[r], blindings[r])?  Returns the verdict bytes: 0 yes, 1 no
        (VerificationError: also a term that does not decode), 2 a non-canonical scalar (FormatError)."""
        nb, off, points, signs, values, blindings = self._psum_args(row_offsets, points, signs, values, value_bytes, blindings)
        vd = C.create_string_buffer(max(nb, 1))
        self._chk(self._L.bpgpu_pedersen_balance_batch(self.h, nb, off, points, signs, values, value_bytes, blindings, vd))
        return vd.raw[:nb]

    def pedersen_sum_batch_dev(self, row_offsets, d_points, d_signs, d_values, value_bytes, d_blindings, d_out, d_status, stream=None):
        """bpgpu_pedersen_sum_batch_dev: row_offsets a host sequence, every buffer a device address (int, or None), asynchronous on `stream`."""
        row_offsets = [int(x) for x in row_offsets]
        nb = len(row_offsets) - 1
        self._chk(self._L.bpgpu_pedersen_sum_batch_dev(self.h, nb, (C.c_uint32 * (nb + 1))(*row_offsets), d_points, d_signs, d_values, value_bytes, d_blindings,
                                                       d_out, d_status, stream))

    def pedersen_balance_batch_dev(self, row_offsets, d_points, d_signs, d_values, value_bytes, d_blindings, d_verdict, stream=None):
        """bpgpu_pedersen_balance_batch_dev: row_offsets a host sequence, every buffer a device address (int, or None), asynchronous on `stream`."""
        row_offsets = [int(x) for x in row_offsets]
        nb = len(row_offsets) - 1
        self._chk(self._L.bpgpu_pedersen_balance_batch_dev(self.h, nb, (C.c_uint32 * (nb + 1))(*row_offsets), d_points, d_signs, d_values, value_bytes, d_blindings,
                                                           d_verdict, stream))

    # ---- proofs of knowledge of commitment openings (bpgpu_opening_*) ----
    @staticmethod
    def _opening_args(form, nb, values, value_bytes):
        assert form in (OPENING_FULL, OPENING_BLINDING) and value_bytes in (8, 32)
        assert values is None or len(values) == value_bytes * nb
        return None if values is None else bytes(values)

    def opening_create_batch_ts(self, form, transcripts, commitments, values, value_bytes, blindings, rng32=None, want_transcripts=False):
        """Proofs that the caller knows the openings (values[i], blindings[i]) of commitments[i], each on its caller's own transcript
        (bpgpu_opening_create_batch_ts).  form OPENING_FULL: value and blinding secret, 96-byte proofs; OPENING_BLINDING: the value is
        public (values None: every value 0), 64-byte proofs.  rng32: 32 bytes per proof, the seed of its ChaChaRng (None: the library
        draws them); never one seed for two statements or transcripts.  Returns (proofs bytes, status bytes[, transcripts])."""
        nb = len(commitments) // 32
        values = self._opening_args(form, nb, values, value_bytes)
        assert len(commitments) == len(blindings) == 32 * nb and (rng32 is None or len(rng32) == 32 * nb)
        pl = 96 if form == OPENING_FULL else 64
        out, st = C.create_string_buffer(pl * max(nb, 1)), C.create_string_buffer(max(nb, 1))
        tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_opening_create_batch_ts(self.h, form, nb, transcripts, self._ts_stride(transcripts, nb), rng32, bytes(commitments), values,
                                                        value_bytes, bytes(blindings), out, st, tso))
        res = (out.raw[:pl * nb], st.raw[:nb])
        return res + (tso.raw[:TRANSCRIPT_BYTES * nb],) if want_transcripts else res

    def opening_verify_batch_ts(self, form, proofs, proof_len, transcripts, commitments, values=None, value_bytes=8, want_msm=False, want_transcripts=False):
        """Verify len(commitments) / 32 opening proofs one by one (bpgpu_opening_verify_batch_ts).  values: the public values of form
        OPENING_BLINDING (None: every value 0); None in form OPENING_FULL.  Returns the verdict bytes[, msm_out][, transcripts]."""
        nb = len(commitments) // 32
        values = self._opening_args(form, nb, values, value_bytes)
        assert len(proofs) == nb * proof_len
        verdict = C.create_string_buffer(max(nb, 1))
        msm = C.create_string_buffer(32 * max(nb, 1)) if want_msm else None
        tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_opening_verify_batch_ts(self.h, form, nb, bytes(proofs), proof_len, transcripts, self._ts_stride(transcripts, nb),
                                                        bytes(commitments), values, value_bytes, verdict, msm, tso))
        out = (verdict.raw[:nb],) + ((msm.raw[:32 * nb],) if want_msm else ()) + ((tso.raw[:TRANSCRIPT_BYTES * nb],) if want_transcripts else ())
        return out if len(out) > 1 else out[0]

    def opening_verify_rlc_ts(self, form, proofs, proof_len, transcripts, commitments, values=None, value_bytes=8, weights64=None, want_transcripts=False):
        """The same verdicts through ONE combined check (bpgpu_opening_verify_rlc_ts; per-proof fallback where it does not decide).
        Returns (verdict bytes, batch_ok, 32-byte encoding of the combined point[, transcripts])."""
        nb = len(commitments) // 32
        values = self._opening_args(form, nb, values, value_bytes)
        assert len(proofs) == nb * proof_len and (weights64 is None or len(weights64) == 64 * nb)
        verdict = C.create_string_buffer(max(nb, 1))
        bo = C.create_string_buffer(33)
        tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_opening_verify_rlc_ts(self.h, form, nb, bytes(proofs), proof_len, transcripts, self._ts_stride(transcripts, nb),
                                                      bytes(commitments), values, value_bytes, weights64, verdict, bo, tso))
        out = (verdict.raw[:nb], bo.raw[0] == 0, bo.raw[1:33])
        return out + (tso.raw[:TRANSCRIPT_BYTES * nb],) if want_transcripts else out

    def opening_verify_batch_ts_dev(self, form, nbatch, d_proofs, proof_len, shared_transcript, d_transcripts, d_commitments, d_values, value_bytes,
                                    d_verdict, d_msm_out=None, d_transcripts_out=None, stream=None):
        """bpgpu_opening_verify_batch_ts_dev: shared_transcript a 208-byte host state or None, every buffer a device address (int, or
        None), asynchronous on `stream`."""
        self._chk(self._L.bpgpu_opening_verify_batch_ts_dev(self.h, form, nbatch, d_proofs, proof_len, shared_transcript, d_transcripts, d_commitments,
                                                            d_values, value_bytes, d_verdict, d_msm_out, d_transcripts_out, stream))

    def opening_verify_rlc_ts_dev(self, form, nbatch, d_proofs, proof_len, shared_transcript, d_transcripts, d_commitments, d_values, value_bytes,
                                  d_weights64, d_verdict, d_batch_out=None, d_transcripts_out=None, stream=None):
        """bpgpu_opening_verify_rlc_ts_dev: as above; undecided verdicts read BPGPU_VERDICT_UNDECIDED (5)."""
        self._chk(self._L.bpgpu_opening_verify_rlc_ts_dev(self.h, form, nbatch, d_proofs, proof_len, shared_transcript, d_transcripts, d_commitments,
                                                          d_values, value_bytes, d_weights64, d_verdict, d_batch_out, d_transcripts_out, stream))

    # ---- proofs of recorded linear relations between points (bpgpu_sigma_*) ----
    def sigma_relation_create(self, desc):
        """Record a relation from its canonical descriptor bytes (include/bpgpu.h) -> (handle, S, P, E, digest).  The handle belongs to
        this context; release it with sigma_relation_destroy."""
        h = C.c_void_p()
        self._chk(self._L.bpgpu_sigma_relation_create(self.h, bytes(desc), len(desc), C.byref(h)))
        S, P, E, dg = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.create_string_buffer(32)
        self._chk(self._L.bpgpu_sigma_relation_shape(h, C.byref(S), C.byref(P), C.byref(E), dg))
        return h, S.value, P.value, E.value, dg.raw

    def sigma_relation_destroy(self, rel):
        self._L.bpgpu_sigma_relation_destroy(rel)

    def sigma_create_batch_ts(self, rel, shape, transcripts, points, secrets, rng32=None, want_transcripts=False):
        """Proofs of the relation `rel` (shape = (S, P, E)) for len(points) / (32 P) rows, each on its caller's own transcript
        (bpgpu_sigma_create_batch_ts).  rng32: 32 bytes per row, the seed of its ChaChaRng (None: the library draws them); never one seed
        for two statements or transcripts.  Returns (proofs bytes, status bytes[, transcripts])."""
        S, P, E = shape
        nb = len(points) // (32 * P)
        assert len(points) == 32 * P * nb and len(secrets) == 32 * S * nb and (rng32 is None or len(rng32) == 32 * nb)
        pl = 32 * (E + S)
        out, st = C.create_string_buffer(pl * max(nb, 1)), C.create_string_buffer(max(nb, 1))
        tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_sigma_create_batch_ts(self.h, rel, nb, transcripts, self._ts_stride(transcripts, nb), rng32, bytes(points), bytes(secrets), out, st, tso))
        res = (out.raw[:pl * nb], st.raw[:nb])
        return res + (tso.raw[:TRANSCRIPT_BYTES * nb],) if want_transcripts else res

    def sigma_verify_batch_ts(self, rel, shape, proofs, transcripts, points, want_msm=False, want_transcripts=False):
        """Verify the rows one by one (bpgpu_sigma_verify_batch_ts).  Returns the verdict bytes[, msm_out (E x 32 bytes per row)][, transcripts]."""
        S, P, E = shape
        nb, pl = len(points) // (32 * P), 32 * (E + S)
        assert len(points) == 32 * P * nb and len(proofs) == nb * pl
        verdict = C.create_string_buffer(max(nb, 1))
        msm = C.create_string_buffer(32 * E * max(nb, 1)) if want_msm else None
        tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_sigma_verify_batch_ts(self.h, rel, nb, bytes(proofs), pl, transcripts, self._ts_stride(transcripts, nb), bytes(points), verdict, msm, tso))
        out = (verdict.raw[:nb],) + ((msm.raw[:32 * E * nb],) if want_msm else ()) + ((tso.raw[:TRANSCRIPT_BYTES * nb],) if want_transcripts else ())
        return out if len(out) > 1 else out[0]

    def sigma_verify_rlc_ts(self, rel, shape, proofs, transcripts, points, weights64=None, want_transcripts=False):
        """The same verdicts through ONE combined check (bpgpu_sigma_verify_rlc_ts; per-proof fallback where it does not decide).
        weights64: 64 bytes per (row, equation).  Returns (verdict bytes, batch_ok, 32-byte encoding of the combined point[, transcripts])."""
        S, P, E = shape
        nb, pl = len(points) // (32 * P), 32 * (E + S)
        assert len(points) == 32 * P * nb and len(proofs) == nb * pl and (weights64 is None or len(weights64) == 64 * E * nb)
        verdict = C.create_string_buffer(max(nb, 1))
        bo = C.create_string_buffer(33)
        tso = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_sigma_verify_rlc_ts(self.h, rel, nb, bytes(proofs), pl, transcripts, self._ts_stride(transcripts, nb), bytes(points), weights64,
                                                    verdict, bo, tso))
        out = (verdict.raw[:nb], bo.raw[0] == 0, bo.raw[1:33])
        return out + (tso.raw[:TRANSCRIPT_BYTES * nb],) if want_transcripts else out

    def sigma_verify_batch_ts_dev(self, rel, nbatch, d_proofs, proof_len, shared_transcript, d_transcripts, d_points, d_verdict, d_msm_out=None,
                                  d_transcripts_out=None, stream=None):
        """bpgpu_sigma_verify_batch_ts_dev: shared_transcript a 208-byte host state or None, every buffer a device address (int, or
        None), asynchronous on `stream`."""
        self._chk(self._L.bpgpu_sigma_verify_batch_ts_dev(self.h, rel, nbatch, d_proofs, proof_len, shared_transcript, d_transcripts, d_points, d_verdict,
                                                          d_msm_out, d_transcripts_out, stream))

    def sigma_verify_rlc_ts_dev(self, rel, nbatch, d_proofs, proof_len, shared_transcript, d_transcripts, d_points, d_weights64, d_verdict,
                                d_batch_out=None, d_transcripts_out=None, stream=None):
        """bpgpu_sigma_verify_rlc_ts_dev: as above; undecided verdicts read BPGPU_VERDICT_UNDECIDED (5)."""
        self._chk(self._L.bpgpu_sigma_verify_rlc_ts_dev(self.h, rel, nbatch, d_proofs, proof_len, shared_transcript, d_transcripts, d_points, d_weights64,
                                                        d_verdict, d_batch_out, d_transcripts_out, stream))

    # ---- batches of transcripts (bpgpu_transcript_batch) ----
    @staticmethod
    def _ts_ops(raw):
        """[(kind, label, data address or None, stride, len, lens address or None)] -> (bpgpu_ts_op array, what must stay alive)"""
        arr = (TsOp * max(len(raw), 1))()
        keep = []
        for o, (kind, label, data, stride, length, lens) in zip(arr, raw):
            lb = C.create_string_buffer(bytes(label), max(len(label), 1))
            keep.append(lb)
            o.kind, o.label, o.label_len, o.data, o.stride, o.len, o.lens = kind, C.addressof(lb), len(label), data, stride, length, lens
        return arr, keep

    def transcript_batch(self, nbatch, ops, label=None, states=None):
        """One script over nbatch transcripts, host buffers (bpgpu_transcript_batch).  Start: label (Transcript::new(label) for every row)
        or states (one 208-byte state for all rows, or one per row).  ops, in order:
            ("append", label, messages)      messages: one bytes object for every row, or a list of nbatch bytes objects of any lengths
            ("append_u64", label, xs)        xs: one int, or a list of nbatch
            ("challenge", label, n)          n challenge bytes per row
            ("challenge_scalar", label)      the crate's challenge_scalar, 32 canonical bytes per row
        Returns (states: nbatch x 208 bytes, [per challenge op, in order: list of nbatch bytes objects])."""
        assert (label is None) != (states is None)
        assert states is None or len(states) in (TRANSCRIPT_BYTES, TRANSCRIPT_BYTES * nbatch)
        stride_in = TRANSCRIPT_BYTES if (states is not None and nbatch != 1 and len(states) == TRANSCRIPT_BYTES * nbatch) else 0
        raw, keep, outs = [], [], []
        for op in ops:
            kind, lbl = op[0], bytes(op[1])
            if kind == "append" and isinstance(op[2], (bytes, bytearray, memoryview)):
                buf = C.create_string_buffer(bytes(op[2]), max(len(op[2]), 1))
                keep.append(buf)
                raw.append((TS_APPEND, lbl, C.addressof(buf), 0, len(op[2]), None))
            elif kind == "append":
                msgs = [bytes(m) for m in op[2]]
                assert len(msgs) == nbatch
                ln = max([len(m) for m in msgs] or [0])
                ragged = any(len(m) != ln for m in msgs)
                buf = C.create_string_buffer(b"".join(m + bytes(ln - len(m)) for m in msgs), max(ln * nbatch, 1))
                lens = (C.c_uint32 * max(nbatch, 1))(*[len(m) for m in msgs]) if ragged else None
                keep += [buf, lens]
                raw.append((TS_APPEND, lbl, C.addressof(buf), ln, ln, C.addressof(lens) if ragged else None))
            elif kind == "append_u64":
                xs = [op[2]] if isinstance(op[2], int) else list(op[2])
                assert isinstance(op[2], int) or len(xs) == nbatch
                buf = (C.c_uint64 * len(xs))(*xs)
                keep.append(buf)
                raw.append((TS_APPEND_U64, lbl, C.addressof(buf), 8 if not isinstance(op[2], int) else 0, 8, None))
            elif kind in ("challenge", "challenge_scalar"):
                n = op[2] if kind == "challenge" else 32
                buf = C.create_string_buffer(max(n * nbatch, 1))
                keep.append(buf)
                outs.append((buf, n))
                raw.append((TS_CHALLENGE if kind == "challenge" else TS_CHALLENGE_SCALAR, lbl, C.addressof(buf), max(n, 1), n, None))
            else:
                raise ValueError("unknown transcript operation %r" % (kind,))
        arr, keep2 = self._ts_ops(raw)
        out = C.create_string_buffer(TRANSCRIPT_BYTES * max(nbatch, 1))
        self._chk(self._L.bpgpu_transcript_batch(self.h, nbatch, label, len(label) if label is not None else 0, states, stride_in, arr, len(raw), out))
        return out.raw[:TRANSCRIPT_BYTES * nbatch], [[b.raw[r * max(n, 1):r * max(n, 1) + n] for r in range(nbatch)] for b, n in outs]

    def transcript_batch_dev(self, nbatch, raw_ops, d_states_out, label=None, d_states_in=None, stride_in=0, stream=None):
        """bpgpu_transcript_batch_dev: raw_ops = [(kind, label bytes, device address of data, stride, len, device address of lens or None)];
        the states are device addresses (int); asynchronous on `stream`."""
        arr, keep = self._ts_ops(raw_ops)
        self._chk(self._L.bpgpu_transcript_batch_dev(self.h, nbatch, label, len(label) if label is not None else 0, d_states_in, stride_in, arr, len(raw_ops),
                                                     d_states_out, stream))

    # ---- the multi-party aggregation protocol (bpgpu_mpc_*; the typestate classes of range_proof_mpc.py are batches of one) ----
    def mpc_state_bytes(self, n):
        return self._L.bpgpu_mpc_state1_bytes(n), self._L.bpgpu_mpc_state2_bytes(n)

    @staticmethod
    def _mpc_seeded(npar, rng, rng_seed32, first_draw):
        """the seeded form's arguments: None when neither keyword is given, else (rng32 bytes or None, uint64 array or None);
        first_draw alone: the seeded call with rng32 = NULL (the library draws the seeds)."""
        if rng_seed32 is None and first_draw is None:
            return None
        if rng is not None:
            raise ValueError("rng bytes and rng_seed32 / first_draw exclude each other")
        seeds = None if rng_seed32 is None else bytes(rng_seed32)
        if seeds is not None and len(seeds) != 32 * npar:
            raise ValueError("rng_seed32: 32 bytes per party")
        if first_draw is not None and len(first_draw) != npar:
            raise ValueError("first_draw: one block index per party")
        return seeds, (None if first_draw is None else (C.c_uint64 * max(npar, 1))(*first_draw))

    def mpc_party_bit_commit(self, n, party_index, values, blindings, rng=None, rng_seed32=None, first_draw=None):
        """Party::new + assign_position_with_rng for len(party_index) parties: returns (bit_commitments 96 bytes each, state1 blobs as one
        bytearray -- secrets: zero it when done).  rng_seed32 (32 bytes per party; None: seeds drawn by the library) and/or first_draw
        (one block index per party) instead of rng: bpgpu_mpc_party_bit_commit_seeded, party p's rng being
        ChaChaRng::from_seed(rng_seed32[32 p:32 p + 32]) advanced by first_draw[p] draws."""
        npar = len(party_index)
        seeded = self._mpc_seeded(npar, rng, rng_seed32, first_draw)
        assert len(values) == npar and len(blindings) == 32 * npar
        assert rng is None or len(rng) == 64 * (2 * n + 2) * npar
        pi = (C.c_uint32 * max(npar, 1))(*party_index)
        va = (C.c_uint64 * max(npar, 1))(*values)
        s1 = self._L.bpgpu_mpc_state1_bytes(n)
        bc = C.create_string_buffer(96 * max(npar, 1))
        st = bytearray(s1 * max(npar, 1))
        stb = (C.c_char * len(st)).from_buffer(st)
        try:
            if seeded:
                self._chk(self._L.bpgpu_mpc_party_bit_commit_seeded(self.h, n, npar, pi, va, blindings, seeded[0], seeded[1], bc, C.cast(stb, C.c_char_p)))
            else:
                self._chk(self._L.bpgpu_mpc_party_bit_commit(self.h, n, npar, pi, va, blindings, rng, bc, C.cast(stb, C.c_char_p)))
        finally:
            del stb
        return bc.raw[:96 * npar], (st if npar else bytearray())

    def mpc_party_poly_commit(self, n, state1, bit_challenges, rng=None, rng_seed32=None, first_draw=None):
        """apply_challenge_with_rng: state1 blobs, (y, z) per party (64 bytes each) or one shared pair -> (poly_commitments, state2 bytearray, status).
        rng_seed32 / first_draw as in mpc_party_bit_commit (bpgpu_mpc_party_poly_commit_seeded; first_draw None: 2n + 2 for every party)."""
        s1, s2 = self.mpc_state_bytes(n)
        npar = len(state1) // s1
        seeded = self._mpc_seeded(npar, rng, rng_seed32, first_draw)
        assert len(state1) == npar * s1 and len(bit_challenges) in (64, 64 * npar)
        assert rng is None or len(rng) == 128 * npar
        shared = 1 if (len(bit_challenges) == 64 and npar != 1) else 0
        pc, status = C.create_string_buffer(64 * max(npar, 1)), C.create_string_buffer(max(npar, 1))
        st = bytearray(s2 * max(npar, 1))
        stb = (C.c_char * len(st)).from_buffer(st)
        try:
            if seeded:
                self._chk(self._L.bpgpu_mpc_party_poly_commit_seeded(self.h, n, npar, bytes(state1), bytes(bit_challenges), shared, seeded[0], seeded[1], pc,
                                                                     C.cast(stb, C.c_char_p), status))
            else:
                self._chk(self._L.bpgpu_mpc_party_poly_commit(self.h, n, npar, bytes(state1), bytes(bit_challenges), shared, rng, pc, C.cast(stb, C.c_char_p), status))
        finally:
            del stb
        return pc.raw[:64 * npar], (st if npar else bytearray()), status.raw[:npar]

    def mpc_party_proof_share(self, n, state2, poly_challenges):
        """PartyAwaitingPolyChallenge::apply_challenge: state2 blobs, x per party (32 bytes each) or one shared -> (shares, status)."""
        _, s2 = self.mpc_state_bytes(n)
        npar = len(state2) // s2
        assert len(state2) == npar * s2 and len(poly_challenges) in (32, 32 * npar)
        shared = 1 if (len(poly_challenges) == 32 and npar != 1) else 0
        sl = 32 * (3 + 2 * n)
        sh, status = C.create_string_buffer(sl * max(npar, 1)), C.create_string_buffer(max(npar, 1))
        self._chk(self._L.bpgpu_mpc_party_proof_share(self.h, n, npar, bytes(state2), bytes(poly_challenges), shared, sh, status))
        return sh.raw[:sl * npar], status.raw[:npar]

    @staticmethod
    def _mpc_ts(nsess, label, transcripts):
        if transcripts is None:
            return label, len(label), None, 0
        assert len(transcripts) in (TRANSCRIPT_BYTES, TRANSCRIPT_BYTES * nsess)
        return None, 0, bytes(transcripts), (0 if (len(transcripts) == TRANSCRIPT_BYTES and nsess != 1) else TRANSCRIPT_BYTES)

    def mpc_dealer_bit_challenge(self, n, m, bit_commitments, label=b"", transcripts=None):
        """Dealer::new + receive_bit_commitments for len(bit_commitments) / (96 m) sessions -> (y z per session, compress(A) compress(S) per
        session, advanced transcripts, status).  transcripts: None (Transcript::new(label)), one 208-byte state, or one per session."""
        ns = len(bit_commitments) // (96 * m)
        assert len(bit_commitments) == ns * 96 * m
        lb, ll, ts, stride = self._mpc_ts(ns, label, transcripts)
        ch, sums = C.create_string_buffer(64 * max(ns, 1)), C.create_string_buffer(64 * max(ns, 1))
        tso, status = C.create_string_buffer(TRANSCRIPT_BYTES * max(ns, 1)), C.create_string_buffer(max(ns, 1))
        self._chk(self._L.bpgpu_mpc_dealer_bit_challenge(self.h, n, m, ns, bytes(bit_commitments), lb, ll, ts, stride, ch, sums, tso, status))
        return ch.raw[:64 * ns], sums.raw[:64 * ns], tso.raw[:TRANSCRIPT_BYTES * ns], status.raw[:ns]

    def mpc_dealer_poly_challenge(self, m, poly_commitments, transcripts):
        """receive_poly_commitments -> (x per session, compress(T_1) compress(T_2) per session, advanced transcripts, status)."""
        ns = len(poly_commitments) // (64 * m)
        assert len(poly_commitments) == ns * 64 * m and len(transcripts) == TRANSCRIPT_BYTES * ns
        ts = C.create_string_buffer(bytes(transcripts), TRANSCRIPT_BYTES * max(ns, 1))
        x, sums, status = C.create_string_buffer(32 * max(ns, 1)), C.create_string_buffer(64 * max(ns, 1)), C.create_string_buffer(max(ns, 1))
        self._chk(self._L.bpgpu_mpc_dealer_poly_challenge(self.h, m, ns, bytes(poly_commitments), ts, x, sums, status))
        return x.raw[:32 * ns], sums.raw[:64 * ns], ts.raw[:TRANSCRIPT_BYTES * ns], status.raw[:ns]

    def mpc_dealer_assemble(self, n, m, shares, bit_commitments, poly_commitments, challenges, transcripts, label=b"", initial_transcripts=None,
                            rng64=None, trusted=False):
        """assemble_shares + receive_shares_with_rng / receive_trusted_shares -> (proofs, bad_shares (m bytes per session), status,
        advanced transcripts).  challenges: y, z, x per session; label / initial_transcripts: what Dealer::new was given."""
        sl = 32 * (3 + 2 * n)
        ns = len(shares) // (sl * m)
        assert len(shares) == ns * sl * m and len(bit_commitments) == ns * 96 * m and len(poly_commitments) == ns * 64 * m
        assert len(challenges) == 96 * ns and len(transcripts) == TRANSCRIPT_BYTES * ns and (rng64 is None or len(rng64) == 64 * ns)
        lb, ll, its, stride = self._mpc_ts(ns, label, initial_transcripts)
        pl = 32 * (9 + 2 * ((n * m).bit_length() - 1))
        ts = C.create_string_buffer(bytes(transcripts), TRANSCRIPT_BYTES * max(ns, 1))
        pr, bad, status = C.create_string_buffer(pl * max(ns, 1)), C.create_string_buffer(m * max(ns, 1)), C.create_string_buffer(max(ns, 1))
        self._chk(self._L.bpgpu_mpc_dealer_assemble(self.h, n, m, ns, bytes(shares), bytes(bit_commitments), bytes(poly_commitments), bytes(challenges), ts,
                                                    lb, ll, its, stride, rng64, 1 if trusted else 0, pr, bad, status))
        return pr.raw[:pl * ns], bad.raw[:m * ns], status.raw[:ns], ts.raw[:TRANSCRIPT_BYTES * ns]

    # ---- instrumentation ----
    def profile_enable(self, on=True):
        self._chk(self._L.bpgpu_profile_enable(self.h, 1 if on else 0))

    def profile_reset(self):
        self._chk(self._L.bpgpu_profile_reset(self.h))

    def profile_report(self):
        buf = C.create_string_buffer(1 << 16)
        self._chk(self._L.bpgpu_profile_report(self.h, buf, len(buf)))
        out = {}
        for line in buf.value.decode().splitlines():
            name, n, ms = line.split()
            out[name] = (int(n), float(ms))
        return out


def _profile_report_of(L, h):
    buf = C.create_string_buffer(1 << 16)
    if L.bpgpu_profile_report(h, buf, len(buf)) != 0:
        raise BpgpuError("bpgpu_profile_report failed")
    out = {}
    for line in buf.value.decode().splitlines():
        name, n, ms = line.split()
        out[name] = (int(n), float(ms))
    return out


class Ticket:
    """One request in flight in the pool's combining queue (bpgpu_pool_rangeproof_submit_ts)."""

    def __init__(self, pool, h, nb, verdict, msm, ts_out):
        self.pool, self.h, self.nb, self._v, self._m, self._t = pool, h, nb, verdict, msm, ts_out

    def done(self):
        return self.h is None or self.pool._L.bpgpu_pool_ticket_done(self.pool.h, self.h) == 1

    def wait(self):
        if self.h is not None:
            h, self.h = self.h, None
            self.pool._chk(self.pool._L.bpgpu_pool_ticket_wait(self.pool.h, h))
        out = [self._v.raw[:self.nb]]
        if self._m is not None:
            out.append(self._m.raw[:32 * self.nb])
        if self._t is not None:
            out.append(self._t.raw[:TRANSCRIPT_BYTES * self.nb])
        return tuple(out) if len(out) > 1 else out[0]


class DevTicket:
    """One submitted device-pointer batch (bpgpu_pool_rangeproof_submit_dev_ex)."""

    def __init__(self, pool, h):
        self.pool, self.h = pool, h

    def stream_wait(self, stream):
        """make `stream` (raw hipStream_t as int; 0 = default stream) wait on the device for this batch's verdicts"""
        self.pool._chk(self.pool._L.bpgpu_pool_ticket_stream_wait(self.pool.h, self.h, stream or None))

    def done(self):
        return self.h is None or self.pool._L.bpgpu_pool_ticket_done(self.pool.h, self.h) == 1

    def wait(self):
        if self.h is not None:
            h, self.h = self.h, None
            self.pool._chk(self.pool._L.bpgpu_pool_ticket_wait(self.pool.h, h))


class Pool:
    """Owns one bpgpu_pool: `lanes` contexts on each of `devices` (include/bpgpu.h, "pool").  The scheduler of the library:
    one synchronous call for any number of proofs from host memory (verify), or asynchronous device-pointer batches that the
    pool coalesces into wide launch chains (submit_dev / flush / wait)."""

    def __init__(self, devices=(0,), lanes=0, **options):
        self._L = lib()
        h = C.c_void_p()
        devs = (C.c_int * len(devices))(*devices)
        rc = self._L.bpgpu_pool_create(devs, len(devices), lanes, C.byref(h))
        if rc != 0:
            raise BpgpuError("bpgpu_pool_create(devices=%s) failed: %s (no CPU fallback)" % (list(devices), ERR_NAMES.get(rc, rc)))
        self.h = h
        for k, v in options.items():
            if v is not None:
                self.set_option(k, v)

    def close(self):
        if getattr(self, "h", None):
            self._L.bpgpu_pool_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise BpgpuError("%s: %s" % (ERR_NAMES.get(rc, rc), self._L.bpgpu_pool_last_error(self.h).decode()))

    def set_option(self, key, value):
        self._chk(self._L.bpgpu_pool_set_option(self.h, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_int64(0)
        self._chk(self._L.bpgpu_pool_get_option(self.h, key.encode(), C.byref(v)))
        return v.value

    @property
    def n_devices(self):
        return self._L.bpgpu_pool_devices(self.h)

    @property
    def n_lanes(self):
        return self._L.bpgpu_pool_lanes(self.h)

    def gens_create(self, gens_capacity, party_capacity):
        self._chk(self._L.bpgpu_pool_gens_create(self.h, gens_capacity, party_capacity))

    def gens_load(self, gens_capacity, party_capacity, G, H, B, B_blinding):
        assert len(G) == len(H) == 32 * gens_capacity * party_capacity
        self._chk(self._L.bpgpu_pool_gens_load(self.h, gens_capacity, party_capacity, G, H, B, B_blinding))

    def gens_add_shape(self, n2, m2):
        """a second, larger-window table for the smaller shape (n2, m2), both windows re-balanced under one budget (bpgpu_pool_gens_add_shape)"""
        self._chk(self._L.bpgpu_pool_gens_add_shape(self.h, n2, m2))

    def rangeproof_verify(self, n, m, proofs, proof_len, commitments, label, rng64=None, want_msm=False):
        """ONE call, any number of proofs, host memory in and out (bpgpu_pool_rangeproof_verify)."""
        nb = len(proofs) // proof_len if proof_len else 0
        assert len(proofs) == nb * proof_len and len(commitments) == 32 * m * nb
        assert rng64 is None or len(rng64) == 64 * nb
        verdict = C.create_string_buffer(max(nb, 1))
        msm = C.create_string_buffer(32 * max(nb, 1)) if want_msm else None
        self._chk(self._L.bpgpu_pool_rangeproof_verify(self.h, n, m, nb, proofs, proof_len, commitments, label, len(label), rng64, verdict, msm))
        return (verdict.raw[:nb], msm.raw[:32 * nb]) if want_msm else verdict.raw[:nb]

    def rangeproof_verify_rlc_mixed(self, groups, rng64=None, weights64=None):
        """Context.rangeproof_verify_rlc_mixed through the pool (bpgpu_pool_rangeproof_verify_rlc_mixed): the whole call on the next device"""
        rc, verdict, ok, enc = _rlc_mixed_call(self._L.bpgpu_pool_rangeproof_verify_rlc_mixed, self.h, groups, rng64, weights64)
        self._chk(rc)
        return verdict, ok, enc

    def rangeproof_verify_rlc_mixed_ts(self, groups, rng64=None, weights64=None, want_transcripts=False):
        """Context.rangeproof_verify_rlc_mixed_ts through the pool (bpgpu_pool_rangeproof_verify_rlc_mixed_ts): the whole call on the next device"""
        rc, out = _rlc_mixed_ts_call(self._L.bpgpu_pool_rangeproof_verify_rlc_mixed_ts, self.h, groups, rng64, weights64, want_transcripts)
        self._chk(rc)
        return out

    def rangeproof_verify_ts(self, n, m, proofs, proof_len, commitments, transcripts, rng64=None, want_msm=False, want_transcripts=True):
        """The reference's call shape (bpgpu_pool_rangeproof_verify_ts): blocking, any number of threads at once; `transcripts`
        is ONE 208-byte state for all proofs or one per proof.  Returns (verdict, [msm,] [transcripts_out])."""
        nb = len(proofs) // proof_len if proof_len else 0
        assert len(proofs) == nb * proof_len and len(commitments) == 32 * m * nb
        assert len(transcripts) in (TRANSCRIPT_BYTES, TRANSCRIPT_BYTES * nb)
        stride = TRANSCRIPT_BYTES if (len(transcripts) == TRANSCRIPT_BYTES * nb and nb != 1) or (nb == 1 and want_transcripts) else 0
        assert rng64 is None or len(rng64) == 64 * nb
        verdict = C.create_string_buffer(max(nb, 1))
        msm = C.create_string_buffer(32 * max(nb, 1)) if want_msm else None
        ts_out = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        self._chk(self._L.bpgpu_pool_rangeproof_verify_ts(self.h, n, m, nb, proofs, proof_len, commitments, transcripts, stride, rng64, verdict, msm, ts_out))
        out = [verdict.raw[:nb]]
        if want_msm:
            out.append(msm.raw[:32 * nb])
        if want_transcripts:
            out.append(ts_out.raw[:TRANSCRIPT_BYTES * nb])
        return tuple(out) if len(out) > 1 else out[0]

    def submit_ts(self, n, m, proofs, proof_len, commitments, transcripts, rng64=None, want_msm=False, want_transcripts=True):
        """The non-blocking form (bpgpu_pool_rangeproof_submit_ts).  Returns a Ticket; ticket.wait() -> as rangeproof_verify_ts."""
        nb = len(proofs) // proof_len if proof_len else 0
        assert len(proofs) == nb * proof_len and len(commitments) == 32 * m * nb
        assert len(transcripts) in (TRANSCRIPT_BYTES, TRANSCRIPT_BYTES * nb)
        stride = TRANSCRIPT_BYTES if (len(transcripts) == TRANSCRIPT_BYTES * nb and nb != 1) or (nb == 1 and want_transcripts) else 0
        verdict = C.create_string_buffer(max(nb, 1))
        msm = C.create_string_buffer(32 * max(nb, 1)) if want_msm else None
        ts_out = C.create_string_buffer(TRANSCRIPT_BYTES * max(nb, 1)) if want_transcripts else None
        t = C.c_void_p()
        self._chk(self._L.bpgpu_pool_rangeproof_submit_ts(self.h, n, m, nb, proofs, proof_len, commitments, transcripts, stride, rng64, verdict, msm, ts_out,
                                                          C.byref(t)))
        return Ticket(self, t, nb, verdict, msm, ts_out)

    def submit_dev(self, dev_index, n, m, nbatch, d_proofs, proof_len, d_commitments, label, d_rng64, d_verdict, d_msm_out=None):
        """queue a device-resident batch (raw device pointers as ints); see flush / wait"""
        self._chk(self._L.bpgpu_pool_rangeproof_submit_dev(self.h, dev_index, n, m, nbatch, d_proofs, proof_len, d_commitments, label, len(label),
                                                           d_rng64, d_verdict, d_msm_out))

    def submit_dev_ex(self, dev_index, n, m, nbatch, d_proofs, proof_len, d_commitments, label, d_rng64, d_verdict, d_msm_out=None, producer_stream=None,
                      want_ticket=True):
        """submit_dev with a completion contract (bpgpu_pool_rangeproof_submit_dev_ex): producer_stream = raw hipStream_t (int; 0 = the
        legacy default stream) the inputs are produced on, or None; returns a DevTicket (or None)."""
        t = C.c_void_p()
        self._chk(self._L.bpgpu_pool_rangeproof_submit_dev_ex(self.h, dev_index, n, m, nbatch, d_proofs, proof_len, d_commitments, label, len(label), d_rng64,
                                                              d_verdict, d_msm_out, producer_stream or None, 0 if producer_stream is None else 1,
                                                              C.byref(t) if want_ticket else None))
        return DevTicket(self, t) if want_ticket else None

    def submit_rlc_dev(self, dev_index, n, m, nbatch, d_proofs, proof_len, d_commitments, label, d_rng64, d_verdict, d_batch_out=None, producer_stream=None,
                       want_ticket=False):
        """queue a device-resident batch for the batch-combined check (bpgpu_pool_rangeproof_submit_rlc_dev): one identity check per launch chain"""
        t = C.c_void_p()
        self._chk(self._L.bpgpu_pool_rangeproof_submit_rlc_dev(self.h, dev_index, n, m, nbatch, d_proofs, proof_len, d_commitments, label, len(label), d_rng64,
                                                               d_verdict, d_batch_out, producer_stream or None, 0 if producer_stream is None else 1,
                                                               C.byref(t) if want_ticket else None))
        return DevTicket(self, t) if want_ticket else None

    def gather_dev(self, root, parts, sizes, d_dst, stream=None):
        """bpgpu_pool_gather_dev: every shard's device-resident verdict bytes to one buffer on pool device `root` (raw device pointers as ints)"""
        n = self.n_devices
        assert len(parts) == len(sizes) == n
        self._chk(self._L.bpgpu_pool_gather_dev(self.h, root, (C.c_void_p * n)(*parts), (C.c_size_t * n)(*sizes), d_dst, stream or None))

    def flush(self):
        self._chk(self._L.bpgpu_pool_flush(self.h))

    def wait(self):
        self._chk(self._L.bpgpu_pool_wait(self.h))

    # ---- the boundary function through the combining queue (blocking, any number of threads) ----
    def msm_batch_shared(self, n, m, nbatch, n_unique, gen_scalars, uniq_scalars, uniq_points):
        """optional_multiscalar_mul in the mega-check shape, one call per MSM (or a few) from any thread (bpgpu_pool_msm_batch_shared)."""
        assert len(gen_scalars) == 32 * (2 * n * m + 2) * nbatch
        assert len(uniq_scalars) == len(uniq_points) == 32 * n_unique * nbatch
        out, st = C.create_string_buffer(32 * max(nbatch, 1)), C.create_string_buffer(max(nbatch, 1))
        self._chk(self._L.bpgpu_pool_msm_batch_shared(self.h, n, m, nbatch, n_unique, gen_scalars, uniq_scalars, uniq_points, out, st))
        return out.raw[:32 * nbatch], st.raw[:nbatch]

    def msm_batch(self, n_terms, scalars, points):
        """a ragged batch of multiscalar multiplications (bpgpu_pool_msm_batch): MSMs of equal length share launch chains."""
        nb = len(n_terms)
        assert len(scalars) == len(points) == 32 * sum(n_terms)
        nt = (C.c_uint32 * max(nb, 1))(*n_terms)
        out, st = C.create_string_buffer(32 * max(nb, 1)), C.create_string_buffer(max(nb, 1))
        self._chk(self._L.bpgpu_pool_msm_batch(self.h, nb, nt, scalars, points, out, st))
        return out.raw[:32 * nb], st.raw[:nb]

    def msm_shared_submit_dev(self, dev_index, n, m, nbatch, n_unique, d_gen_scalars, d_uniq_scalars, d_uniq_points, d_out, d_status, producer_stream=None,
                              want_ticket=False):
        """device-resident MSM batch on the next lane of pool device dev_index (bpgpu_pool_msm_batch_shared_submit_dev; raw device pointers as ints)"""
        t = C.c_void_p()
        self._chk(self._L.bpgpu_pool_msm_batch_shared_submit_dev(self.h, dev_index, n, m, nbatch, n_unique, d_gen_scalars, d_uniq_scalars or None, d_uniq_points or None,
                                                                 d_out, d_status, producer_stream or None, 0 if producer_stream is None else 1,
                                                                 C.byref(t) if want_ticket else None))
        return DevTicket(self, t) if want_ticket else None

    def ipp_verify(self, n, proofs, proof_len, label, Gf, Hf, P, Q, G, H, want_msm=False):
        """InnerProductProof::verify for len(proofs) / proof_len proofs through the queue (bpgpu_pool_ipp_verify)."""
        nb = len(proofs) // proof_len if proof_len else 0
        assert len(Gf) == len(Hf) == len(G) == len(H) == 32 * n * nb and len(P) == len(Q) == 32 * nb
        verdict = C.create_string_buffer(max(nb, 1))
        msm = C.create_string_buffer(32 * max(nb, 1)) if want_msm else None
        self._chk(self._L.bpgpu_pool_ipp_verify(self.h, n, nb, proofs, proof_len, label, len(label), Gf, Hf, P, Q, G, H, verdict, msm))
        return (verdict.raw[:nb], msm.raw[:32 * nb]) if want_msm else verdict.raw[:nb]

    def trace_dump(self, path):
        self._chk(self._L.bpgpu_pool_trace_dump(self.h, path.encode()))

    # ---- instrumentation (per lane context) ----
    def _lanes(self, every=1):
        for d in range(self.n_devices):
            for l in range(0, self.n_lanes, every):
                yield self._L.bpgpu_pool_lane(self.h, d, l)

    def profile_enable(self, on=True, every=1):
        for h in self._lanes():
            self._L.bpgpu_profile_enable(h, 0)
        if on:
            for h in self._lanes(every):
                self._L.bpgpu_profile_enable(h, 1)

    def profile_reset(self):
        for h in self._lanes():
            self._L.bpgpu_profile_reset(h)

    def profile_report(self):
        out = {}
        for h in self._lanes():
            for name, (cnt, ms) in _profile_report_of(self._L, h).items():
                o = out.get(name, (0, 0.0))
                out[name] = (o[0] + cnt, o[1] + ms)
        return out
