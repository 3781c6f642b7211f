"""The staging state machine of the host-pointer entry points on the CPU: bulletproofs_amd/csrc/host_io.h compiled with g++ against
the fake HIP runtime of tests/cpu_pool/ (streams are threads that perform the copies), as a stand-alone program (tests/cpu_host_io/)
-- once optimised, once under AddressSanitizer + UndefinedBehaviorSanitizer (runtimes linked statically), where a pinned block freed
while a copy is queued or read after its release is a reported use-after-free.  The program checks: the region layout (offsets = running sums of 256-byte
aligned sizes, inputs < outputs < device-only, host and device offsets equal, empty regions take no room); a block outgrown inside a
call (retired, readable after finish, kept by a reopen, freed by the next call); the reuse guard (the next call's first allocation
waits for a call left in flight, after a mark only up to the mark); finish (return-code priority, exactly the declared secret bytes
and every device buffer cleared, whatever the call's return code); submit / collect (delivered once, by collect or by the next open);
a device-pointer call (the body on the caller's stream or the context's own, under the lock, one ctx_leave behind it whatever it
returns, none and no body where ctx_enter fails, return-code priority); the delivery of a combined check (no rerun where the batch
result's byte 0 is 0, one rerun otherwise whose verdicts alone replace the first pass's, also from a retired block, and a failed
rerun leaves the caller's verdicts untouched)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "cpu_host_io")
STAGES = ["layout ok", "growth ok", "reuse guard ok", "finish ok", "submit/collect ok", "dev call ok", "combined delivery ok", "all ok"]


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-j2"], cwd=DIR, stdout=subprocess.DEVNULL)
    return os.path.join(DIR, "build")


@pytest.mark.parametrize("exe", ["host_io_test", "host_io_test_asan"])
def test_staging_state_machine(built, exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([os.path.join(built, exe)], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[:6000]
    assert [ln for ln in p.stdout.splitlines() if ln.endswith(" ok")] == STAGES
