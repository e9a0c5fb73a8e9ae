"""The queue behind the stream pool (csrc/bpsw_ext_group.h: the calls that find every pooled stream busy, and the groups the extension
calls among them form) as a stand-alone program under ThreadSanitizer (tests/ext_group_host/): sixteen threads over one to four fake
streams whose "launch" sleeps.  Every call must complete exactly once, no group may exceed the maximum, a caller that runs alone is never
grouped, and -- callers queued one by one behind a busy stream -- leaders and the members they take come in arrival order.  The
reference has nothing of the kind (one synchronous call per batch, src/main/jni_fpga/sw_extend_fpga.c:116-193); the contract is pinned."""
import os
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ext_group_host")


def _run(san, *args):
    tag = san.replace(",", "_")
    r = subprocess.run(["make", "-C", HERE, "-s", f"SAN={san}"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 second_deadlock_stack=1", ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([os.path.join(HERE, "_build", f"ext_group_host_{tag}")] + [str(a) for a in args], env=env, capture_output=True,
                       text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "WARNING: ThreadSanitizer" not in out and "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("EXTGROUP")][0].split()
    return dict(zip(line[1::2], line[2::2])) if line[1] != "fifo" else dict(zip(line[2::2], line[3::2]))


@pytest.mark.parametrize("streams,max_group", [(1, 8), (2, 8), (4, 8), (3, 3), (4, 1)])
def test_sixteen_callers_under_thread_sanitizer(streams, max_group):
    f = _run("thread", "stress", 16, 150, streams, max_group)
    assert int(f["wrong"]) == 0 and int(f["calls"]) == 16 * 150
    assert int(f["largest"]) <= max_group
    if max_group == 1:
        assert int(f["groups"]) == int(f["members"])
    elif streams == 1:
        assert int(f["largest"]) > 1, "sixteen callers behind one stream never formed a group"


def test_leaders_and_members_come_in_arrival_order():
    assert int(_run("thread", "fifo")["wrong"]) == 0


def test_queue_under_address_and_ub_sanitizers():
    assert int(_run("address,undefined", "stress", 16, 150, 2, 8)["wrong"]) == 0
