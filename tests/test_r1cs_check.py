"""The R1CS witness check without a GPU: the pure-Python twin on gadgets whose unsatisfied sets are known, the device code of
csrc/r1cs_check.h lane by lane on the host (tests/r1cs_check_harness: a shared library, and once more as a stand-alone executable
under AddressSanitizer and UBSan), the recorder's locate option, and the argument checks of bpgpu_r1cs_witness_check."""
import ctypes as C
import hashlib
import os
import subprocess

import pytest

import r1cs_check_twin as K
import r1cs_corpus as G
import r1cs_twin as R


def _chal(tag, n):
    return [int.from_bytes(hashlib.shake_256(b"check challenge " + tag + b"%d" % i).digest(64), "little") % R.L for i in range(n)]


# ---- the twin ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.CASES, ids=[c[0] for c in K.CASES])
def test_twin_on_the_known_gadgets(case):
    name, _, _, Q, nch, bad = case
    rec = K.record(case)
    d = rec.descriptor()
    assert len(d[5]) == Q and len(d[4]) == nch
    assert K.unsatisfied(rec, [K.CHALLENGE] * nch) == bad


def test_twin_corpus_cases_are_satisfied():
    for case in G.SMALL:
        rec = G.record_prover(case)
        assert K.unsatisfied(rec, _chal(case.name.encode(), case.nch)) == [], case.name


# ---- the device code on the host ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("r1ch")
    lib = C.CDLL(K.build_harness(tmp))
    lib.r1ch_run_file.argtypes = [C.c_char_p, C.c_char_p]
    return lib, tmp


def _run(harness, name, provers, challenges):
    lib, tmp = harness
    fin, fout = str(tmp / (name + ".bin")), str(tmp / (name + ".out"))
    with open(fin, "wb") as f:
        f.write(K.case_file(provers, challenges))
    assert lib.r1ch_run_file(fin.encode(), fout.encode()) == 0, name
    return K.parse_output(open(fout, "rb").read(), len(provers)), fin


def _expect(out, provers, challenges):
    for b, (rec, ch) in enumerate(zip(provers, challenges)):
        first, count, mp = K.report(rec, ch)
        assert out["status"][b] == 0
        assert out["first"][b] == (0xffffffff if first is None else first), b
        assert out["count"][b] == count, b
        assert out["maps"][b][:len(mp)] == mp and not any(out["maps"][b][len(mp):]), b


def test_chunk_is_a_power_of_two_between_32_and_256(harness):
    assert harness[0].r1ch_chunk() in (32, 64, 128, 256)


@pytest.mark.parametrize("case", G.SMALL, ids=[c.name for c in G.SMALL])
def test_corpus_cases_report_all_satisfied(harness, case):
    nb = 3
    provers = [G.record_prover(case, idx) for idx in range(nb)]
    challenges = [_chal(case.name.encode() + b"/%d/" % idx, case.nch) for idx in range(nb)]
    out, _ = _run(harness, case.name, provers, challenges)
    assert out["status"] == [0] * nb and out["first"] == [0xffffffff] * nb and out["count"] == [0] * nb
    assert not any(any(m) for m in out["maps"])
    _expect(out, provers, challenges)


@pytest.mark.parametrize("case", K.CASES, ids=[c[0] for c in K.CASES])
def test_gadget_cases_match_the_twin(harness, case):
    name, _, _, _, nch, bad = case
    rec = K.record(case)
    challenges = [[K.CHALLENGE] * nch, _chal(name.encode(), nch)]
    out, _ = _run(harness, name, [rec, rec], challenges)
    _expect(out, [rec, rec], challenges)
    assert out["first"][0] == (bad[0] if bad else 0xffffffff) and out["count"][0] == len(bad)


def test_long_rows_on_the_host(harness):
    """rows of 0 .. 600 terms: whichever chunk length, rows at its boundary and rows of several chunks; a failing short row behind a
    long one, a failing long row"""
    lengths = [0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 600, 3]
    chunk = harness[0].r1ch_chunk()
    ok = K.long_row_prover(lengths)
    bad_short = K.long_row_prover(lengths, broken=len(lengths) - 1)
    bad_long = K.long_row_prover(lengths, broken=lengths.index(600))
    provers = [ok, bad_short, bad_long]
    out, _ = _run(harness, "long", provers, [[]] * 3)
    _expect(out, provers, [[]] * 3)
    assert out["first"] == [0xffffffff, len(lengths) - 1, lengths.index(600)]
    nlong = sum(1 for ln in lengths if ln > chunk)
    assert out["longs"] == nlong and out["slots"] == sum(-(-ln // chunk) for ln in lengths if ln > chunk)
    assert out["units"] == len(lengths) - nlong + out["slots"]


def test_sanitized_harness(harness, tmp_path):
    """the same harness as a stand-alone executable under AddressSanitizer and UBSan (host code only; run once as a child process)"""
    exe = K.build_harness(tmp_path, sanitized=True)
    assert exe is not None, "g++ could not build the sanitized harness"
    assert subprocess.run([exe, "--chunk"], capture_output=True, text=True).stdout.split() == ["CHUNK", str(harness[0].r1ch_chunk())]
    lengths = [0, 1, 33, 129, 257, 600, 2]
    provers = [K.long_row_prover(lengths), K.long_row_prover(lengths, broken=6), K.record(K.CASES[1])]
    for name, ps, ch in (("long", provers[:2], [[], []]), ("shuffle", provers[2:], [[K.CHALLENGE]])):
        want, fin = _run(harness, "san-" + name, ps, ch)
        fout = str(tmp_path / (name + ".out"))
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
        assert r.returncode == 0, r.stderr[-4000:]
        assert K.parse_output(open(fout, "rb").read(), len(ps)) == want


# ---- the recorder -------------------------------------------------------------------------------------------------------------
def test_locate_leaves_the_recording_unchanged_and_names_the_line():
    for case in K.CASES:
        plain, located = K.record(case), K.record(case, locate=True)
        assert plain.descriptor() == located.descriptor() and plain.structure() == located.structure()
        assert plain.where(0) is None and len(located.locations) == len(located.descriptor()[5])
    from bulletproofs_amd import r1cs
    cs = r1cs.Prover(bytes(208), locate=True)
    x, y = cs.commit(3, 1), cs.commit(4, 2)
    import inspect
    line = inspect.currentframe().f_lineno
    _, _, o = cs.multiply(x, y)          # line + 1: constraints 0 and 1
    cs.constrain(o - 12)                 # line + 2: constraint 2

    def cb(cs):
        z = cs.challenge_scalar(b"c")
        cs.constrain(x * z - y * z)      # line + 6: constraint 3

    cs.specify_randomized_constraints(cb)
    cs._finish()
    here = os.path.abspath(__file__)
    got = [(os.path.abspath(f), ln) for f, ln in cs.locations]
    assert got == [(here, line + 1), (here, line + 1), (here, line + 2), (here, line + 6)]
    assert cs.where(3).endswith("test_r1cs_check.py:%d" % (line + 6))
    e = r1cs.Unsatisfied(3, cs.where(3))
    assert isinstance(e, r1cs.R1CSError) and e.constraint == 3 and e.where == cs.where(3) and "test_r1cs_check.py" in str(e)


# ---- the ABI's argument checks (the built library, no GPU) ----------------------------------------------------------------------
def test_witness_check_rejects_bad_arguments():
    from bulletproofs_amd import r1cs
    L = r1cs.lib()
    shuffle, example = K.record(K.CASES[0]), K.record(K.CASES[3])
    cs, ws, ce, we = shuffle.circuit(), shuffle.witness(), example.circuit(), example.witness()
    v, free, _ = (lambda i: (i[0], i[2], None))(shuffle.inputs())
    first, status = (C.c_uint32 * 1)(), C.create_string_buffer(1)
    chal = (5).to_bytes(32, "little")
    maps = C.create_string_buffer(8)
    INVALID = -1
    # challenges == NULL with a challenge recorded; map_stride below ceil(9 / 8); a witness program of another circuit -- each refused
    # before the context is looked at (none exists without a GPU)
    assert L.bpgpu_r1cs_witness_check(None, cs._h, ws._h, 1, v, free, None, first, None, None, 0, status) == INVALID
    assert L.bpgpu_r1cs_witness_check(None, cs._h, ws._h, 1, v, free, chal, first, None, maps, 1, status) == INVALID
    assert L.bpgpu_r1cs_witness_check(None, cs._h, we._h, 1, v, free, chal, first, None, None, 0, status) == INVALID
    assert L.bpgpu_r1cs_witness_check(None, ce._h, ws._h, 1, v, free, None, first, None, None, 0, status) == INVALID
    assert L.bpgpu_r1cs_witness_check(None, None, ws._h, 1, v, free, chal, first, None, None, 0, status) == INVALID
    assert L.bpgpu_r1cs_prove_batch_checked(None, cs._h, ws._h, 0, None, None, None, None, 0, None, None, 0, None, None, None, None, None) == INVALID
