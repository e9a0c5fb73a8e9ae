"""Extension calls that wait for a stream ride one launch chain (csrc/bpsw_ext_group.h; ext_sift_kernel and ext_kernel over gridDim.y
batch descriptors): with ONE pooled stream kept busy, k calls of contexts of their own are queued (the library's gauge says when all
of them are), must be launched as one group -- nine as a group of eight and one of one -- and must each return what
pyoracle.Oracle().wire_extend computes for its batch, word for word.  The scenarios live in tests/ext_group_child.py and run in child
processes: the switches (BPSW_STREAM_POOL=1, BPSW_EXT_SIFT_MIN=64, BPSW_EXT_RING=0, BPSW_EXT_INJECT_DEFER, BPSW_EXT_GROUP_MAX) are
read once per process.  The reference has no such path (one synchronous call per batch: src/main/jni_fpga/sw_extend_fpga.c:116-193)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _child(scenario, **extra):
    env = dict(os.environ, BPSW_STREAM_POOL="1", BPSW_EXT_SIFT_MIN="64", BPSW_EXT_RING="0")
    for k in ("BPSW_EXT_INJECT_DEFER", "BPSW_EXT_GROUP_MAX", "BPSW_STREAM_SHARE", "BPSW_ZEROCOPY", "BPSW_EXT_LAZY_FULL", "BPSW_LIB"):
        env.pop(k, None)
    env.update({k: str(v) for k, v in extra.items()})
    r = subprocess.run([sys.executable, os.path.join(HERE, "ext_group_child.py"), scenario], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"EXTGROUP ok {scenario}" in r.stdout, r.stdout[-2000:]


def test_one_two_eight_and_nine_waiting_calls_are_one_group_and_nine_are_eight_and_one():
    _child("sizes")


def test_members_of_every_size_scoring_and_entry_group_and_the_other_plans_run_alone():
    """64, 65, 200 and 1 000 tasks, other gap costs with another matrix, a member that reads through the view and one the sift finishes
    whole are one group; the 1-task batch (below the sift threshold), a coordinate batch, a classify call and a batch with a 300-base
    flank run alone around them, a malformed batch is refused before it joins; the same contexts through three groups in another
    order each (a stale queue word of one round would spoil the next)"""
    _child("mixed")


def test_every_member_of_a_group_makes_its_own_late_launch():
    """BPSW_EXT_INJECT_DEFER=3: every third task that reaches the short kernel is deferred, so every member with such a task finds a posted
    defer length and launches the full kernel itself, once (ext_full_relaunches) -- the member the sift finishes whole posts a zero and
    launches nothing; with BPSW_EXT_SIFT_MIN=1 the 1-task batch is a member too: a full group of eight"""
    _child("mixed", BPSW_EXT_INJECT_DEFER=3, BPSW_EXT_SIFT_MIN=1)


def test_group_max_of_one_switches_grouping_off():
    _child("off", BPSW_EXT_GROUP_MAX=1)
