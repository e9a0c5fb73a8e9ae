"""Every kernel form of csrc/bpsw_swalign.hip -- swp_kernel<C, KL>, swp_resident_kernel<3|5>, sw4_kernel, sw_kernel<C> -- against the
oracle's restatement of SWUtil.SWAlign2, on the job tables of tests/sw_cases.py: every job of every table, all seven fields, bit-exact.

Which form a batch runs follows from its scoring, its longest mate, its longest window, its size and the process's switches
(launch_sw_kernel, sw_ring_class, the lone-launch rule of sw_stage_run); sw_cases.kernel_for restates that, and _run checks the one part
of it that the library reports: the `submitted` counter of the submission ring moves exactly for the batches that had to take the ring.
At the suite's environment a process reaches the packed kernels of every class (keys in LDS, and in HBM for the long windows), both
resident kernels, and sw_kernel<C> through scorings the packed form refuses and mates above 256 bases.  The switches are read once
per process, so the rest runs in child processes (test_forms_behind_a_switch), one per row of CHILDREN; each child ends with
test_forms_reached, which names the instantiations its environment was started for."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import bpsw_hip
import sw_cases as sc

pytestmark = pytest.mark.gpu
GUARD = "BPSW_TEST_SW_FORMS_CHILD"
SWITCHES = ("BPSW_RING", "BPSW_RING_LONE_LAUNCH", "BPSW_SW_PACK", "BPSW_SW_QUAD", "BPSW_SW_KEYS_LDS", "BPSW_ZEROCOPY")

REACHED = {}      # kernel instantiation -> the batches that ran it in this process
RAN = set()       # the tests of this file that ran to their end in this process


def _run(ctx, orc, batch):
    """one batch against the oracle; asserts which way it went where the library says so; returns the kernel's name"""
    env = os.environ
    jobs = sc.jobs_from(batch.pairs)
    opt = sc.apply(bpsw_hip.default_opt(), batch.scoring)
    if sc.ring_class(batch, env) and len(batch.pairs) >= sc.LONE_LAUNCH_MIN and sc.lone_launch(env):
        time.sleep(0.03)      # the lone-launch rule: no extension call on the device in the last 20 ms
    s0 = ctx.ring_stats()[1]
    got = ctx.swalign2_batch(opt, batch.xtra, **jobs)
    moved = ctx.ring_stats()[1] - s0
    want = sc.want(orc, batch)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (f"{batch.name} / {batch.scoring.name} / xtra {batch.xtra:#x}: {bad.size}/{len(want)} jobs differ, first {bad[:5]} "
                           f"{[batch.tags[k] for k in bad[:5]]}: got {got[bad[:3]]} want {want[bad[:3]]}")
    if sc.takes_ring(batch, env):
        assert moved == 1, f"{batch.name}: a ring-eligible batch of {len(batch.pairs)} jobs did not go through the ring"
    elif sc.lone_launch(env):
        assert moved == 0, f"{batch.name}: took the ring"
    kernel = sc.kernel_for(batch, env, moved > 0)
    REACHED.setdefault(kernel, []).append(batch.name)
    return kernel


def _plain():
    return not any(k in os.environ for k in SWITCHES)


# ---- the tables ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scoring", (sc.DEFAULT,) + sc.PACKED_TABLE_SCORINGS, ids=lambda s: s.name)
@pytest.mark.parametrize("c", range(1, 6))
def test_packed_lengths(ctx, orc, c, scoring):
    """class C's table as one batch (75 jobs: a launch of swp_kernel<C> for a lone caller) and in batches of 13-15 (the ring)"""
    batch = sc.with_scoring(sc.length_cases("packed")[c - 1], scoring)
    kernels = {_run(ctx, orc, batch)} | {_run(ctx, orc, b) for b in sc.chunks(batch)}
    if _plain():
        assert kernels == {f"swp_kernel<{c},lds>", f"swp_resident_kernel<{3 if c <= 3 else 5}>"}
    RAN.add("packed_lengths")


@pytest.mark.parametrize("c", (1, 2, 3, 4, 6, 8))
def test_sw32_lengths(ctx, orc, c):
    """the 32-bit table of sw_kernel<C>: under the default scoring (which the packed form takes up to 256 bases unless it is switched
    off: its windows of 2048 rows and more keep the row keys in HBM) and under (5, 3), which the packed form refuses"""
    batch = sc.length_cases("sw32")[(1, 2, 3, 4, 6, 8).index(c)]
    k1 = _run(ctx, orc, batch)
    k2 = _run(ctx, orc, sc.with_scoring(batch, sc.M5X3))
    if os.environ.get("BPSW_SW_QUAD") != "1":
        assert k2 == f"sw_kernel<{c}>"
    if _plain():
        assert k1 == (f"sw_kernel<{c}>" if c > 4 else f"swp_kernel<{c + 1},hbm>")
    if c == 3:
        for b in (sc.length_cases("sw32")[6], sc.with_scoring(sc.length_cases("sw32")[6], sc.M5X3)):     # the lone job
            _run(ctx, orc, b)
    RAN.add("sw32_lengths")


def test_quad_lengths(ctx, orc):
    for batch in sc.length_cases("quad"):
        _run(ctx, orc, batch)
        _run(ctx, orc, sc.with_scoring(batch, sc.M5X3))
    for batch in sc.reduced_cases():
        _run(ctx, orc, batch)
    RAN.add("quad_lengths")


def test_quad_fallback_at_161_bases(ctx, orc):
    """one mate of Q4_COLS + 1 = 161 bases in a batch: no quad form, and still exact"""
    rng = np.random.default_rng(161)
    base = sc.length_cases("quad")[0]
    mate = rng.integers(0, 4, sc.Q4_COLS + 1).tolist()
    window = rng.integers(0, 4, 200).tolist() + mate + rng.integers(0, 4, 100).tolist()
    for scoring in (sc.DEFAULT, sc.M5X3):
        batch = sc.Batch("quad_with_161", scoring, sc.XTRA, base.pairs[:40] + [(mate, window, 0)], base.tags[:40] + [("q161",)])
        assert _run(ctx, orc, batch) != "sw4_kernel"
    RAN.add("quad_fallback")


def test_second_best_tables(ctx, orc):
    for batch in sc.second_best_cases():
        _run(ctx, orc, batch)
    RAN.add("second_best")


def test_stop_tables(ctx, orc):
    for batch in sc.stop_cases():
        _run(ctx, orc, batch)
        if batch.name == "stop_duo_cap":
            _run(ctx, orc, sc.Batch(batch.name + "_swapped", batch.scoring, batch.xtra, batch.pairs[1:] + batch.pairs[:1], batch.tags[1:] + batch.tags[:1]))
    RAN.add("stop")


def test_n_tables(ctx, orc):
    for batch in sc.n_cases():
        _run(ctx, orc, batch)
    b = sc.n_cases()[0]      # ... and the first sixty duos one at a time and in fives, as a lone caller's small batches go
    for at in range(0, 120, 2):
        _run(ctx, orc, sc.Batch(f"n_one[{at}:{at + 2}]", b.scoring, b.xtra, b.pairs[at:at + 2], b.tags[at:at + 2]))
    for at in range(0, 120, 10):
        _run(ctx, orc, sc.Batch(f"n_one[{at}:{at + 10}]", sc.DEFAULT_G5241, b.xtra, b.pairs[at:at + 10], b.tags[at:at + 10]))
    RAN.add("n_tables")


def test_scoring_tables(ctx, orc):
    kernels = {}
    for batch in sc.scoring_cases():
        kernels[batch.scoring.name] = _run(ctx, orc, batch)
        for b in sc.chunks(batch)[:3]:
            _run(ctx, orc, b)
    if os.environ.get("BPSW_SW_PACK") != "0":
        assert all(kernels[s.name].startswith("swp_") for s in sc.PACKABLE), kernels
    assert all(not kernels[s.name].startswith("swp_") for s in sc.REFUSING), kernels
    # the fourth neighbour never reaches a kernel: a negative gap cost is refused at the entry
    opt = sc.apply(bpsw_hip.default_opt(), sc.DEFAULT)
    opt.e_ins = -1
    with pytest.raises(bpsw_hip.BpswError, match=r"\(-1\)"):
        ctx.swalign2_batch(opt, sc.XTRA, **sc.jobs_from(sc.scoring_cases()[0].pairs))
    _run(ctx, orc, sc.scoring_cases()[0])
    RAN.add("scoring")


@pytest.mark.parametrize("c", range(1, 6))
def test_ends_in_first_columns(ctx, orc, c):
    batch = sc.ends_in_first_columns()[c - 1]
    _run(ctx, orc, batch)
    for b in sc.chunks(batch, sizes=(5, 6, 7)):
        _run(ctx, orc, b)
    RAN.add("ends")


@pytest.mark.parametrize("batch", sc.key_edge_cases(), ids=lambda b: b.name)
def test_key_edges(ctx, orc, batch):
    """1024 / 1025 rows: the resident kernel's cap for class 3 (ring / launch); 1536 / 1537: the last window whose keys stay in LDS,
    and the resident kernel's cap for class 5"""
    kernel = _run(ctx, orc, batch)
    c, rows, n = batch.tags[0][1], batch.tags[0][2], len(batch.pairs)
    if _plain():
        if n < sc.LONE_LAUNCH_MIN and rows <= sc.RESIDENT_ROWS[c]:
            assert kernel == f"swp_resident_kernel<{c}>"
        else:
            assert kernel == f"swp_kernel<{c},{'lds' if rows <= sc.PK_KEYS_LDS_MAX else 'hbm'}>"
    RAN.add("key_edges")


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(ctx, orc):
    good = sc.ends_in_first_columns()[2]
    rng = np.random.default_rng(513)
    mate = rng.integers(0, 4, sc.MAX_QLEN + 1).tolist()
    with pytest.raises(bpsw_hip.BpswError, match=r"\(-4\)"):        # BPSW_ERR_LIMIT
        ctx.swalign2_batch(bpsw_hip.default_opt(), sc.XTRA, **sc.jobs_from(good.pairs[:3] + [(mate, mate + [0] * 30, 0)]))
    _run(ctx, orc, good)
    window = rng.integers(0, 4, sc.MAX_TLEN + 1).tolist()
    with pytest.raises(bpsw_hip.BpswError, match=r"\(-4\)"):
        ctx.swalign2_batch(bpsw_hip.default_opt(), sc.XTRA, **sc.jobs_from(good.pairs[:3] + [(mate[:100], window, 0)]))
    _run(ctx, orc, good)
    empty = ctx.swalign2_batch(bpsw_hip.default_opt(), sc.XTRA, **sc.jobs_from([]))
    assert empty.shape == (0, 7)
    _run(ctx, orc, good)


# ---- the longest window --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mate_len", (240, 300))
def test_longest_window(orc, mate_len):
    """four windows of BPSW_SW_MAX_TLEN = 65 535 rows; te = 65 534 with te2 near row 300, and the other way round.  In a context of its
    own: the row scratch grows to 16 x 65 536 bytes per resident wave (8 GiB at 256 CUs), and a context's arenas only grow."""
    batch = sc.longest_window(mate_len)
    own = bpsw_hip.Context(0)
    try:
        kernel = _run(own, orc, batch)
    finally:
        own.close()
    if os.environ.get("BPSW_SW_PACK") != "0":
        assert kernel == ("swp_kernel<5,hbm>" if mate_len <= 256 else "sw_kernel<6>")
    RAN.add("longest")


# ---- what this process reached -------------------------------------------------------------------------------------------------
PACKED_TABLES = {"packed_lengths", "second_best", "stop", "n_tables", "scoring", "ends"}
CHILDREN = {
    # name: (environment, -k selection, the tests that must have run, the instantiations that must have been reached,
    #        timeout in seconds = about ten times the wall time of the child measured on an MI355X, given next to it)
    "ring_off": ({"BPSW_RING": "0"}, "packed_lengths or second_best or stop_tables or n_tables or scoring or ends_in", PACKED_TABLES,
                 {f"swp_kernel<{c},lds>" for c in range(1, 6)}, 50),      # measured: 5.1 s
    "ring_always": ({"BPSW_RING_LONE_LAUNCH": "0"}, "packed_lengths or second_best or stop_tables or n_tables or scoring or ends_in", PACKED_TABLES,
                    {"swp_resident_kernel<3>", "swp_resident_kernel<5>"}, 50),      # measured: 5.0 s
    "pack_off": ({"BPSW_SW_PACK": "0", "BPSW_SW_QUAD": "0"}, "sw32_lengths or second_best or stop_tables or n_tables", {"sw32_lengths", "second_best", "stop", "n_tables"},
                 {f"sw_kernel<{c}>" for c in (1, 2, 3, 4, 6, 8)}, 45),      # measured: 4.3 s
    "quad": ({"BPSW_SW_PACK": "0", "BPSW_SW_QUAD": "1"}, "quad_lengths or quad_fallback or second_best or stop_tables", {"quad_lengths", "quad_fallback", "second_best", "stop"},
             {"sw4_kernel", "sw_kernel<3>"}, 40),      # measured: 3.6 s
    "keys_hbm": ({"BPSW_SW_KEYS_LDS": "0", "BPSW_RING": "0"}, "packed_lengths or key_edges", {"packed_lengths", "key_edges"},
                 {f"swp_kernel<{c},hbm>" for c in range(1, 6)}, 40),      # measured: 3.8 s
}
PLAIN_TESTS = PACKED_TABLES | {"sw32_lengths", "quad_lengths", "quad_fallback", "key_edges", "longest"}
PLAIN_KERNELS = ({f"swp_kernel<{c},lds>" for c in range(1, 6)} | {f"swp_kernel<{c},hbm>" for c in range(2, 6)} |
                 {"swp_resident_kernel<3>", "swp_resident_kernel<5>"} | {f"sw_kernel<{c}>" for c in (1, 2, 3, 4, 6, 8)})


def test_forms_reached():
    """last of the tables' tests: the instantiations this process's environment is there for were run (REACHED is filled by _run from the
    batch geometry, the switches and the ring's counter).  Means something only after the tests it names; a narrower selection passes."""
    child = os.environ.get(GUARD)
    if child:
        _, _, tests, kernels, _ = CHILDREN[child]
    elif _plain():
        tests, kernels = PLAIN_TESTS, PLAIN_KERNELS
    else:
        return
    if not tests <= RAN:
        assert not child, f"the child {child} did not run {sorted(tests - RAN)}"
        return
    assert kernels <= set(REACHED), f"not reached: {sorted(kernels - set(REACHED))}"
    if child == "quad":      # the stop and second-best tables with mates of up to 160 bases went through the quad form as well
        assert any(n.startswith("stop30_q150") for n in REACHED["sw4_kernel"]) and "sb_plateau" in REACHED["sw4_kernel"]
    if child == "keys_hbm":
        assert "swp_kernel<5,lds>" not in REACHED and "swp_kernel<3,lds>" not in REACHED


# ---- the forms behind a switch: child processes ---------------------------------------------------------------------------------
_CHILD_FAILED = []


@pytest.mark.parametrize("child", list(CHILDREN))
def test_forms_behind_a_switch(child):
    if os.environ.get(GUARD):
        pytest.skip("already a child of this test")
    if _CHILD_FAILED:
        pytest.skip(f"the child {_CHILD_FAILED[0]} failed: no further processes on the device")
    env, select, _, _, limit = CHILDREN[child]
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), "-k", f"{select} or forms_reached"],
                           env=dict(os.environ, **env, **{GUARD: child}), capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        _CHILD_FAILED.append(child)
        raise
    print(f"child {child}: {time.perf_counter() - t0:.1f} s, exit {r.returncode}; {r.stdout.strip().splitlines()[-1:]}")
    if r.returncode != 0:
        _CHILD_FAILED.append(child)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and " failed" not in r.stdout and " skipped" not in r.stdout, r.stdout[-500:]
