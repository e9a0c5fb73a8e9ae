"""The pull of the rescue ring (csrc/bpsw_ring_pull_core.h, swp_pull_unit in csrc/bpsw_swalign.hip): a batch above BPSW_RING_ZC_BYTES
that goes through the submission ring is not copied; every resident worker stages its own unit in LDS.

The switches are read once per process, so the tables of tests/ring_pull_tables.py run in two child processes, each to its end: one
with the ring forced on every batch (BPSW_RING_LONE_LAUNCH=0), every batch above the zero-copy threshold (BPSW_RING_ZC_BYTES=64) and
the pull on every ring class (BPSW_RING_PULL=1; unset, class 5 keeps the copy), and one with BPSW_RING_PULL=0, which copies as before.  Here every job's seven fields are held against the oracle, the two
runs against each other byte for byte, and the counters against the path each table names."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bpsw_hip
import pyoracle as po
import ring_pull_tables as rt
import sw_cases as sc
from conftest import region_fields_equal

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TABLES = rt.tables()


def _child(tmp, name, **env):
    path = os.path.join(str(tmp), name + ".npz")
    e = dict(os.environ, BPSW_RING_LONE_LAUNCH="0", BPSW_RING_ZC_BYTES="64", **env)
    for k in ("BPSW_RING", "BPSW_ZEROCOPY", "BPSW_SW_PACK", "BPSW_SW_HALVES"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "ring_pull_tables.py"), path], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return dict(np.load(path))


@pytest.fixture(scope="module")
def pulled(tmp_path_factory):
    return _child(tmp_path_factory.mktemp("ring_pull"), "pull", BPSW_RING_PULL="1")


@pytest.fixture(scope="module")
def copied(tmp_path_factory):
    return _child(tmp_path_factory.mktemp("ring_copy"), "copy", BPSW_RING_PULL="0")


@pytest.mark.parametrize("name", sorted(TABLES))
def test_every_field_equals_the_oracle_through_the_pull(pulled, orc, name):
    jobs, expect = TABLES[name]
    want = orc.sw_align2_jobs(sc.apply(orc.default_opt(), sc.DEFAULT), sc.XTRA, **jobs)[0]
    got = pulled[name]
    assert got.shape == want.shape == (len(jobs["q_len"]), 7)
    assert np.array_equal(got, want), f"{int((got != want).any(axis=1).sum())} of {len(want)} jobs differ, first {np.nonzero((got != want).any(axis=1))[0][:4]}"
    ring_calls, submitted, h2d_ms = pulled[name + ".how"]
    if expect == "pull":
        assert ring_calls == 1 and submitted == 1, "the batch did not go through the ring"
        assert h2d_ms == 0.0, "the batch was copied"
    else:
        assert ring_calls == 0 and submitted == 0, "a window beyond the resident kernel's rows went through the ring"


@pytest.mark.parametrize("name", sorted(TABLES))
def test_the_copy_gives_identical_bytes(pulled, copied, name):
    assert pulled[name].tobytes() == copied[name].tobytes()
    ring_calls, _, h2d_ms = copied[name + ".how"]
    if TABLES[name][1] == "pull":
        assert ring_calls == 1 and h2d_ms > 0.0, "BPSW_RING_PULL=0 did not restore the copy"


@pytest.mark.parametrize("name", sorted(rt.groups()))
def test_groups_through_the_pull(pulled, copied, orc, name):
    g, _ = rt.make_group(name)
    wcnt, wregs, _, _ = orc.matesw_group(orc.default_opt(), g, po.RESCUE_C)
    assert np.array_equal(pulled[name + ".cnt"], wcnt)
    region_fields_equal(pulled[name + ".regs"], wregs)
    ring_calls, sw_calls, h2d_ms = pulled[name + ".how"]
    assert sw_calls >= 1 and ring_calls == sw_calls and h2d_ms == 0.0, (ring_calls, sw_calls, h2d_ms)
    assert pulled[name + ".cnt"].tobytes() == copied[name + ".cnt"].tobytes() and pulled[name + ".regs"].tobytes() == copied[name + ".regs"].tobytes()
    assert copied[name + ".how"][2] > 0.0


def test_the_tripwire_saw_no_late_record(pulled, copied):
    for run in (pulled, copied):
        on, checked, faults = run["integrity"]
        assert on and checked > 150 and faults == 0
