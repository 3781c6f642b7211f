"""The limb-bound corpus of test_limb_bounds_on_cpu.py through the DEVICE build of the same headers, on real wavefronts:
GPU output == CPU harness output == big ints, for every case.

What this covers: tests/gpu_prims/prims.hip compiles fe25519.h, sc25519.h, ge25519.h and horner_wave.h (through the shared
wrappers of tests/cpu_harness/limb_ops.h) for gfx950 in a translation unit of its own -- fe_* / sc28_* / ge_* one lane per case,
the hw_* wavefront arithmetic one 64-lane workgroup per case on real DPP row shifts / rotations and the LDS exchanges of
wv_row_gather16 / wv_rows4, and the __device__ copies of six horner_wave.h drivers (hw_invsqrt_raw_fe, hw_ristretto_decode,
hw_point_shift, hw_shift_table8, hw_horner_msm, hw_horner8_msm).  Where the code is shared the outputs must agree with the host
harness limb for limb; the driver pairs (separate device and host copies) must agree by value mod p.

What it does not cover: these are not the product's code objects (libbpgpu.so's kernels, their register allocation and inlining
differ), and hw_colsum_horner_msm's device copy is not launched here; the MSM parity tests (test_gpu_msm.py,
test_gpu_msm_edge_forms.py) run those."""
import ctypes as C
import os
import subprocess

import pytest

import harness_lib
import limb_corpus as LC
from test_limb_bounds_on_cpu import decode_encodings

pytestmark = pytest.mark.gpu

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_prims")
_SO = os.path.join(_DIR, "libprims.so")


def _build():
    csrc = os.path.join(os.path.dirname(os.path.dirname(_DIR)), "bulletproofs_amd", "csrc")
    srcs = [os.path.join(_DIR, "prims.hip"), os.path.join(os.path.dirname(_DIR), "cpu_harness", "limb_ops.h")]
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if (not os.path.exists(_SO)) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in srcs):
        hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-shared", "-fPIC", "-o", _SO, os.path.join(_DIR, "prims.hip")])
    return _SO


@pytest.fixture(scope="module")
def G():
    return LC.Backend(C.CDLL(_build()), "g_")


@pytest.fixture(scope="module")
def H():
    return LC.Backend(harness_lib.lib(), "h_")


def test_field_primitives_on_device_match_host_limb_for_limb(G, H):
    assert LC.check_fe(G) == LC.check_fe(H)


def test_hw_limbs_to_fe_on_device_match_host_limb_for_limb(G, H):
    out, ok = G.limbs_to_fe([[0xffff] * 15 + [0x1ffff]])
    assert LC.fev(out[0]) % LC.P == 75 and ok[0]
    assert LC.check_limbs_to_fe(G) == LC.check_limbs_to_fe(H)


def test_scalar_montgomery_primitives_on_device_match_host_limb_for_limb(G, H):
    assert LC.check_sc(G) == LC.check_sc(H)


def test_point_formulas_on_device_match_host_limb_for_limb(G, H):
    assert LC.check_ge(G) == LC.check_ge(H)


def test_wavefront_arithmetic_on_real_dpp_and_lds_matches_host_emulation(G, H):
    assert LC.check_hw(G) == LC.check_hw(H)


def test_device_copies_of_the_wavefront_drivers_match_the_host_copies(G, H):
    enc = decode_encodings()
    g, h = LC.check_drivers(G, enc), LC.check_drivers(H, enc)
    assert g.keys() == h.keys()
    for key in g:
        for a, b in zip(g[key], h[key]):   # by value: the two copies are separate code
            assert [LC.fev(a[i:i + 10]) % LC.P for i in range(0, len(a), 10)] == [LC.fev(b[i:i + 10]) % LC.P for i in range(0, len(b), 10)], key
