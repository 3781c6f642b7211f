"""The transcript-batch interpreter without a GPU: ts_batch.h's lane body (tsb_load / tsb_begin / tsb_advance / tsb_permute / tsb_end /
tsb_store) compiled for the host (tests/ts_batch_harness) and driven as k_ts_batch drives it -- wavefronts of lanes that each run to
their own rate boundary and are then permuted together -- against the oracle twin's Transcript, row by row and byte for byte: every
start position of the 166-byte rate, message / label / challenge lengths around the boundary, shared and per-row messages, per-row
lengths, scripts of one and of the most operations.  The same harness also runs as a stand-alone program under AddressSanitizer and
UBSan with every buffer at its exact size."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "ts_batch_harness", "harness.cpp")
L_ORDER = 2**252 + 27742317777372353535851937790883648493
TS_WORDS = 52
APPEND, CHALLENGE, CHALLENGE_SCALAR = 0, 1, 2       # ts_batch.h TSB_*
MAX_OPS = 32                                        # include/bpgpu.h BPGPU_TS_MAX_OPS
MSG_LENGTHS = [0, 1, 3, 4, 5, 163, 164, 165, 166, 167, 168, 331, 332, 333, 1000]
LABEL_LENGTHS = [0, 1, 165, 167]
CHALLENGE_LENGTHS = [0, 1, 16, 32, 64, 165, 166, 167, 400]


class Op(C.Structure):
    """ts_batch.h tsb_op"""
    _fields_ = [("kind", C.c_uint32), ("label_off", C.c_uint32), ("label_len", C.c_uint32), ("len", C.c_uint32), ("stride", C.c_uint64),
                ("data", C.c_void_p), ("lens", C.c_void_p)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tsbatch") / "libtsbatch.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.tsb_run.restype = C.c_uint64
    lib.tsb_run.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(Op), C.c_uint32, C.c_char_p, C.POINTER(C.c_uint64)]
    return lib


def _state_of(t):
    """the 208-byte state of an oracle-twin transcript (include/bpgpu.h BPGPU_TRANSCRIPT_BYTES)"""
    s = t.strobe
    return bytes(s.st) + bytes([s.pos, s.pos_begin, s.cur_flags]) + bytes(5)


def _msg(tag, n):
    return bytes((tag * 31 + 7 * i + (i >> 8)) & 0xff for i in range(n))


@pytest.fixture(scope="module")
def at_position():
    """position 0 .. 165 -> a bound transcript standing there, found by search over the length of a session id (as
    tests/test_rpp_seed_on_cpu._wrapping_transcripts finds its wrapping ones)"""
    import bp_twin
    found = {}
    for length in range(400):
        t = bp_twin.Transcript(b"payment-protocol v3")
        t.append_message(b"session", _msg(length, length))
        found.setdefault(t.strobe.pos, t)
        if len(found) == 166:
            break
    assert sorted(found) == list(range(166))
    return found


def _run(harness, starts, script, W=64, shared_start=False):
    """script: [("append", label, messages)] with messages one bytes object (shared: stride 0) or a list of per-row bytes (packed at the
    stride of the longest, `lens` given when they differ; the buffer ends with the last row's own bytes), ("challenge", label, n),
    ("scalar", label).  Returns (states, [outputs of the challenge ops: per row], permutation rounds, rounds a serial loop would take)."""
    nrows = len(starts)
    ts_in = b"".join(_state_of(t) for t in ([starts[0]] if shared_start else starts))
    ts_in_buf = C.create_string_buffer(ts_in, len(ts_in))
    ts_out = C.create_string_buffer(4 * TS_WORDS * nrows)
    ops = (Op * len(script))()
    keep, outs, labels = [], [], b""
    for o, step in zip(ops, script):
        kind, label = step[0], step[1]
        o.label_off, o.label_len = len(labels), len(label)
        labels += label
        if kind == "append" and isinstance(step[2], bytes):
            buf = C.create_string_buffer(step[2], max(len(step[2]), 1))
            lens = (C.c_uint32 * nrows)(*step[3]) if len(step) > 3 else None        # rows take prefixes of the one message
            o.kind, o.len, o.stride, o.data, o.lens = APPEND, len(step[2]), 0, C.addressof(buf), C.addressof(lens) if lens else None
            keep += [buf, lens]
        elif kind == "append":
            msgs = step[2]
            assert len(msgs) == nrows
            ln = max(len(m) for m in msgs)
            packed = b"".join(m + bytes(ln - len(m)) for m in msgs[:-1]) + msgs[-1]
            buf = C.create_string_buffer(packed, max(len(packed), 1))
            lens = (C.c_uint32 * nrows)(*[len(m) for m in msgs])
            o.kind, o.len, o.stride, o.data = APPEND, ln, ln, C.addressof(buf)
            o.lens = C.addressof(lens) if any(len(m) != ln for m in msgs) else None
            keep += [buf, lens]
        else:
            n = step[2] if kind == "challenge" else 32
            buf = C.create_string_buffer(b"\x5a" * (n * nrows + 1), n * nrows + 1)       # one guard byte behind the last row
            o.kind, o.len, o.stride, o.data, o.lens = (CHALLENGE, n, n, C.addressof(buf), None) if kind == "challenge" else (CHALLENGE_SCALAR, 64, 32, C.addressof(buf), None)
            keep.append(buf)
            outs.append((buf, n))
    serial = C.c_uint64()
    rounds = harness.tsb_run(W, nrows, C.addressof(ts_in_buf), 0 if shared_start else TS_WORDS, C.addressof(ts_out), ops, len(script), labels, C.byref(serial))
    assert rounds != 2**64 - 1
    for buf, n in outs:
        assert buf.raw[n * nrows:] == b"\x5a"
    states = [ts_out.raw[4 * TS_WORDS * r:4 * TS_WORDS * (r + 1)] for r in range(nrows)]
    return states, [[buf.raw[n * r:n * (r + 1)] for r in range(nrows)] for buf, n in outs], rounds, serial.value


def _expect(t0, script, r):
    """the twin: (state, [challenge outputs]) of one row"""
    t = t0.clone()
    outs = []
    for step in script:
        if step[0] == "append":
            t.append_message(step[1], step[2][r] if not isinstance(step[2], bytes) else step[2][:step[3][r]] if len(step) > 3 else step[2])
        elif step[0] == "challenge":
            outs.append(t.challenge_bytes(step[1], step[2]))
        else:
            outs.append((int.from_bytes(t.challenge_bytes(step[1], 64), "little") % L_ORDER).to_bytes(32, "little"))
    return _state_of(t), outs


def _check(harness, starts, script, **kw):
    states, outs, rounds, serial = _run(harness, starts, script, **kw)
    for r in range(len(starts)):
        want_state, want_outs = _expect(starts[0] if kw.get("shared_start") else starts[r], script, r)
        assert [o[r] for o in outs] == want_outs, r
        assert states[r] == want_state, r
    return rounds, serial


def test_every_start_position_of_the_rate(harness, at_position):
    """166 rows standing at positions 0 .. 165 (164 and 165: the two framing bytes of begin_op straddle the rate) in three wavefronts of
    mixed positions: a per-row append, a challenge, an append_u64 and a challenge scalar"""
    starts = [at_position[p] for p in range(166)]
    script = [("append", b"context", [_msg(r, 5) for r in range(166)]), ("challenge", b"binding", 16),
              ("append", b"n", [(r * 0x0101010101010101 % 2**64).to_bytes(8, "little") for r in range(166)]), ("scalar", b"x")]
    _check(harness, starts, script)


@pytest.mark.parametrize("pos", [0, 100, 164, 165])
def test_message_lengths_around_the_rate_as_per_row_lengths(harness, at_position, pos):
    """one op, len = 1000, lens = every length of the matrix in neighbouring rows (0 beside 1000, both ways): rows that wrap zero, one, two
    and six times inside the same op; the message buffer ends with the last row's own bytes"""
    lengths = [0, 1000] + MSG_LENGTHS[1:-1] + [1000, 0]
    starts = [at_position[pos]] * len(lengths)
    rounds, serial = _check(harness, starts, [("append", b"m", [_msg(i, n) for i, n in enumerate(lengths)]), ("challenge", b"c", 8)])
    assert rounds <= 8 < serial      # 1000 bytes are six or seven blocks: the wavefront pays for its longest row, not for the sum


def test_message_lengths_around_the_rate_as_shared_messages(harness, at_position):
    """the same lengths as one op each with ONE message for all rows (stride 0), rows at five positions"""
    starts = [at_position[p] for p in (0, 1, 83, 164, 165)]
    _check(harness, starts, [("append", b"m%d" % n, _msg(n, n)) for n in MSG_LENGTHS])


def test_label_lengths(harness, at_position):
    starts = [at_position[p] for p in (0, 1, 83, 164, 165)]
    script = []
    for n in LABEL_LENGTHS:
        script += [("append", _msg(n + 1, n), [_msg(r, 3 + r) for r in range(5)]), ("challenge", _msg(n + 2, n), 7)]
    _check(harness, starts, script)


def test_challenge_lengths(harness, at_position):
    starts = [at_position[p] for p in (0, 1, 83, 164, 165)]
    _check(harness, starts, [("challenge", b"c%d" % n, n) for n in CHALLENGE_LENGTHS])


def test_challenge_scalar_is_the_wide_reduction(harness, at_position):
    """CHALLENGE_SCALAR == int.from_bytes(challenge_bytes(label, 64), "little") % l, canonical, and the state moves as for 64 bytes"""
    starts = [at_position[p] for p in range(0, 166, 11)]
    states, outs, _, _ = _run(harness, starts, [("scalar", b"y"), ("scalar", b"z")])
    for r, t0 in enumerate(starts):
        t = t0.clone()
        for k, label in enumerate((b"y", b"z")):
            x = int.from_bytes(t.challenge_bytes(label, 64), "little") % L_ORDER
            assert int.from_bytes(outs[k][r], "little") == x < L_ORDER
        assert states[r] == _state_of(t)


def test_scripts_of_one_op_of_the_most_ops_and_of_the_readme_binding(harness, at_position):
    import bp_twin
    starts = [at_position[p] for p in (0, 57, 164, 165)]
    _check(harness, starts, [("append", b"one", b"op")])
    most = []
    for i in range(MAX_OPS):
        most.append(("append", b"a%d" % i, [_msg(i + r, (37 * i + r) % 90) for r in range(4)]) if i % 3 else ("challenge", b"c%d" % i, i))
    _check(harness, starts, most)
    # README: Transcript::new("payment-protocol v3") shared by the rows, then a 32-byte session id each
    fresh = [bp_twin.Transcript(b"payment-protocol v3")] * 70
    _check(harness, fresh, [("append", b"session", [_msg(r, 32) for r in range(70)])], shared_start=True)
    _check(harness, fresh, [("append", b"session", [_msg(r, 32) for r in range(70)])], W=7)


def test_lens_of_zero_and_len_in_neighbouring_rows(harness, at_position):
    """rows alternate between appending nothing and appending all `len` bytes; a shared message and a per-row one in the same script"""
    starts = [at_position[(29 * r) % 166] for r in range(9)]
    script = [("append", b"ragged", [_msg(r, 0 if r % 2 else 200) for r in range(9)]), ("append", b"shared", _msg(3, 40)),
              ("append", b"ragged2", [_msg(r, 200 if r % 2 else 0) for r in range(9)]), ("challenge", b"c", 32)]
    _check(harness, starts, script)


def test_rows_take_per_row_prefixes_of_one_shared_message(harness, at_position):
    """stride 0 together with lens: row 0 takes nothing, later rows more, some all 300 bytes"""
    starts = [at_position[(23 * r) % 166] for r in range(20)]
    lens = [0, 300, 1, 166] + [(37 * r) % 301 for r in range(4, 20)]
    _check(harness, starts, [("append", b"shared", _msg(7, 300), lens), ("challenge", b"c", 16)])


def test_a_wavefront_at_64_positions_permutes_together(harness, at_position):
    """64 rows at 64 different positions append 400 bytes: every row wraps two or three times, at 64 different bytes -- the wavefront takes
    at most four permutation rounds for the op where a lane-by-lane loop takes over 128"""
    starts = [at_position[(5 * r) % 166] for r in range(64)]
    assert len({t.strobe.pos for t in starts}) == 64
    rounds, serial = _check(harness, starts, [("append", b"blob", [_msg(r, 400) for r in range(64)])])
    assert rounds <= 4 and serial >= 128


def test_stand_alone_harness_is_clean_under_address_and_ub_sanitizers(tmp_path):
    """the harness as a program with its own main, -fsanitize=address,undefined, every buffer at its exact size -- the per-row lens case
    among them: the message buffer ends where the last row's own length ends"""
    exe = str(tmp_path / "ts_batch_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTSB_HARNESS_MAIN", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ts_batch harness ok" in out.stdout
