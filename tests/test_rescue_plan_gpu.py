"""The host layer of boundary 1 (csrc/bpsw_rescue.cpp: plan, lean speculation, replay, output assembly, the per-context scratch) on
the hand-built groups of tests/rescue_cases.py, against the oracle's sequential walk -- exact, every field of every region.

How the counters are read (bpsw_matesw_group): sw_jobs grows by every job a round launches; `used` marks a launched job the replay
consumed and sw_wasted grows by those it did not; sw_replayed_rounds grows by the rounds after the first.  The lean plan launches, per
end, only the first anchor that has a job against the mate's INITIAL list, and an end's anchors are judged against a list that only
the other end's anchors change -- so every launched job is one the sequential walk runs too: nothing is wasted, launched jobs minus
wasted ones equal the walk's n_sw, and a second round runs exactly when n_sw exceeds that first round
(rescue_cases.first_round_jobs; tests/test_rescue_cases.py holds each case's claim to it).  A mate of length 0 is the one exception:
the oracle counts an SW call the library never makes, so those cases are compared but not counted."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import bpsw_hip
import pyoracle as po
import rescue_cases as rc
from conftest import region_fields_equal

pytestmark = pytest.mark.gpu
MODES = [po.RESCUE_C, po.RESCUE_SCALA]
MODE_IDS = ["c", "scala"]


def opt_of(factory, overrides):
    opt = factory()
    for k, v in overrides.items():
        setattr(opt, k, v)
    return opt


@pytest.fixture(scope="module")
def walked(orc):
    """the oracle's answer for every case in both flavours, computed once and left unchanged: {(name, mode): (cnt, regs, n_sw)}"""
    out = {}
    for name, (g, o, _) in rc.CASES.items():
        for mode in MODES:
            cnt, regs, n_sw, _cells = orc.matesw_group(opt_of(orc.default_opt, o), g, mode)
            out[name, mode] = (cnt, regs, n_sw)
    return out


@pytest.fixture(scope="module", autouse=True)
def _reference_loaded(ctx):
    ctx.ref_load(rc.PAC, rc.L_PAC)


def same(got_cnt, got, want_cnt, want):
    assert np.array_equal(got_cnt, want_cnt)
    region_fields_equal(got, want)
    assert np.array_equal(got["hash"], want["hash"])


def delta(s0, s1):
    return (s1.sw_jobs - s0.sw_jobs, s1.sw_wasted - s0.sw_wasted, s1.sw_replayed_rounds - s0.sw_replayed_rounds)


@pytest.mark.parametrize("form", ["bytes", "coords"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", list(rc.CASES))
def test_parity_and_accounting(ctx, walked, name, mode, form):
    g, o, claims = rc.CASES[name]
    want_cnt, want, n_sw = walked[name, mode]
    s0 = ctx.stats()
    got_cnt, got = ctx.matesw_group(opt_of(bpsw_hip.default_opt, o), g if form == "bytes" else rc.as_coords(g), mode)
    jobs, wasted, rounds = delta(s0, ctx.stats())
    print(f"{name} mode {mode} {form}: jobs {jobs} wasted {wasted} later rounds {rounds}; the walk's n_sw {n_sw}")
    same(got_cnt, got, want_cnt, want)
    if not claims.get("zero_len"):
        assert jobs - wasted == n_sw
        assert wasted == 0                                   # lean speculation launches nothing the walk does not run
    assert (rounds > 0) == claims["second_round"]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_fast_path_equals_general_walk(ctx, mode):
    """B: a one-hit-per-end pair (the plan's straight-line code) and its twin with a far, sub-threshold second hit (rc != 1: the
    general walk) are touched alike, on both sides of both limits of every orientation"""
    for fast, walk, _pes, _r, _label, touched in rc.B_TABLE:
        seen = []
        for name in (fast, walk):
            g, o, _ = rc.CASES[name]
            s0 = ctx.stats()
            ctx.matesw_group(opt_of(bpsw_hip.default_opt, o), g, mode)
            seen.append(ctx.stats().sw_jobs - s0.sw_jobs)
        assert (seen[0] > 0) == (seen[1] > 0) == touched, (fast, seen)
        assert seen[0] == seen[1], (fast, seen)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", list(rc.G_ORDERS))
def test_assembly_equals_the_pairs_one_by_one(ctx, walked, name, mode):
    g, o, _ = rc.CASES[name]
    pairs, pes = rc.SPECS[name]
    opt = opt_of(bpsw_hip.default_opt, o)
    got_cnt, got = ctx.matesw_group(opt, g, mode)
    same(got_cnt, got, *walked[name, mode][:2])
    cnts, regs = [], []
    for k, p in enumerate(pairs):
        c1, r1 = ctx.matesw_group(opt, rc.build([p], pes, **o), mode)
        r1 = r1.copy()
        keep = r1["hash"] != 0
        r1["hash"][keep] += np.uint64(k << 8)                # build numbers the input hashes by the pair's place in its group
        cnts.append(c1); regs.append(r1)
    same(got_cnt, got, np.concatenate(cnts), np.concatenate(regs))


def test_scratch_is_clean_between_calls(orc):
    """mate_slot, staged_mates, job_round and results stay in the context: a 64-pair group with a second round, a one-pair group, an
    empty group and the first group again, each equal to what a fresh context returns"""
    big, o_big, claims = rc.CASES["I_seed1"]
    assert big.group_size == 64 and claims["second_round"]
    one, o_one, _ = rc.CASES["E_justifier_removed"]
    empty = rc.build([], rc.PES_FR)
    assert empty.group_size == 0
    seq = [(big, o_big), (one, o_one), (empty, {}), (big, o_big)]
    for mode in MODES:
        fresh = []
        for g, o in seq[:3]:
            c = bpsw_hip.Context(0)
            try:
                cnt, regs = c.matesw_group(opt_of(bpsw_hip.default_opt, o), g, mode)
                fresh.append((cnt.copy(), regs.copy()))
            finally:
                c.close()
        fresh.append(fresh[0])
        c = bpsw_hip.Context(0)
        try:
            for (g, o), (want_cnt, want) in zip(seq, fresh):
                s0 = c.stats()
                cnt, regs = c.matesw_group(opt_of(bpsw_hip.default_opt, o), g, mode)
                same(cnt, regs, want_cnt, want)
                if g is big:
                    assert c.stats().sw_replayed_rounds > s0.sw_replayed_rounds
        finally:
            c.close()
        want_cnt, want, _n, _ = orc.matesw_group(opt_of(orc.default_opt, o_big), big, mode)
        same(fresh[0][0], fresh[0][1], want_cnt, want)


# ---- the C ABI called directly: return codes, texts, what is written ----------------------------------------------------------------
def raw(ctx, opt, st, mode, out_cnt, out, cap, want_total=True):
    total = C.c_int64(-7)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    code = bpsw_hip.load_library().bpsw_matesw_group(ctx.h if ctx is not None else None, C.byref(opt) if opt is not None else None,
                                     C.byref(st) if st is not None else None, mode, p(out_cnt), p(out), cap,
                                     C.byref(total) if want_total else None)
    return code, total.value, bpsw_hip.load_library().bpsw_last_error().decode()


def out_buffers(g, n_regs=None):
    cnt = np.full(2 * g.group_size + 2, 0x5A5A5A5A, np.int32)
    regs = np.frombuffer(bytes([0xA5]) * (64 * (int(g.regs.shape[0] + 4 * g.ref_rb.shape[0] + 16) if n_regs is None else n_regs)),
                         bpsw_hip.ALNREG_DTYPE).copy()
    return cnt, regs


def d_case_still_right(ctx, walked):
    g, o, _ = rc.CASES["D_each_orientation"]
    for mode in MODES:
        cnt, regs = ctx.matesw_group(opt_of(bpsw_hip.default_opt, o), g, mode)
        same(cnt, regs, *walked["D_each_orientation", mode][:2])


def test_capacity_is_checked_before_anything_is_written(ctx, walked):
    name = "G_mixed"
    g, o, _ = rc.CASES[name]
    want_cnt, want, _ = walked[name, po.RESCUE_C]
    total = int(want.shape[0])
    assert total > g.regs.shape[0]
    opt, st = opt_of(bpsw_hip.default_opt, o), g.as_struct()
    for cap in (total - 1, 0):
        cnt, regs = out_buffers(g)
        code, got_total, text = raw(ctx, opt, st, po.RESCUE_C, cnt, regs, cap)
        assert (code, got_total, text) == (-3, total, "matesw_group: out_regs too small")
        assert (cnt == 0x5A5A5A5A).all() and (regs.view(np.uint8) == 0xA5).all()
    cnt, regs = out_buffers(g, total + 1)
    code, got_total, _ = raw(ctx, opt, st, po.RESCUE_C, cnt, regs, total)
    assert (code, got_total) == (0, total)
    same(cnt[:2 * g.group_size], regs[:total], want_cnt, want)
    assert (cnt[2 * g.group_size:] == 0x5A5A5A5A).all() and (regs[total:].view(np.uint8) == 0xA5).all()


def _fr_pair_group():
    """two pairs, each with one FR job: window row 1 of each anchor is aligned, rows 0, 2 and 3 lie under failed orientations"""
    return rc.build([rc.rescue_pair(rc.A_F, 1, 1, rc.PES_FR), rc.rescue_pair(rc.A_R, 1, 0, rc.PES_FR)], rc.PES_FR)


def _edit(field, index, value):
    def f(g):
        a = getattr(g, field).copy()
        a[index] = value
        return dataclasses.replace(g, **{field: a})
    return f


REFUSALS = [
    # (what, edit of the group, mode, which argument is null, return code, text)
    ("null_ctx", None, 0, "ctx", -1, "matesw_group: null argument"),
    ("null_opt", None, 0, "opt", -1, "matesw_group: null argument"),
    ("null_group", None, 0, "group", -1, "matesw_group: null argument"),
    ("null_out_cnt", None, 0, "out_cnt", -1, "matesw_group: null argument"),
    ("null_out_total", None, 0, "out_total", -1, "matesw_group: null argument"),
    ("bad_mode_2", None, 2, None, -1, "matesw_group: bad mode"),
    ("bad_mode_minus1", None, -1, None, -1, "matesw_group: bad mode"),
    ("negative_group_size", lambda g: dataclasses.replace(g, group_size=-1), 0, None, -1, "matesw_group: negative group size"),
    ("negative_reg_cnt", _edit("reg_cnt", 3, -1), 0, None, -1, "matesw_group: negative count"),
    ("negative_ref_cnt", _edit("ref_cnt", 0, -1), 0, None, -1, "matesw_group: negative count"),
    ("negative_seq_len", _edit("seq_len", 2, -150), 0, None, -1, "matesw_group: negative count"),
    ("mate_past_seq_pool", lambda g: _edit("seq_off", 3, g.seq_pool.size - 149)(g), 0, None, -1, "matesw_group: mate outside seq_pool"),
    ("mate_before_seq_pool", _edit("seq_off", 0, -1 << 40), 0, None, -1, "matesw_group: mate outside seq_pool"),
    ("window_past_ref_pool", lambda g: _edit("ref_off", 5, g.ref_pool.size - int(g.ref_len[5]) + 1)(g), 0, None, -1, "matesw_group: window outside ref_pool"),
    ("window_before_ref_pool", _edit("ref_off", 1, -16), 0, None, -1, "matesw_group: window outside ref_pool"),
]


@pytest.mark.parametrize("what,edit,mode,null,code,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(ctx, walked, what, edit, mode, null, code, text):
    g = _fr_pair_group()
    assert rc.first_round_jobs(g, bpsw_hip.default_opt()) == 2 and rc.window_ok(g, 1) and rc.window_ok(g, 5)
    if edit is not None:
        g = edit(g)
    keep = g.group_size
    if g.group_size < 0:
        g = dataclasses.replace(g, group_size=2)            # (as_struct and the buffers want a real size; the struct gets the bad one)
    cnt, regs = out_buffers(g)
    st = g.as_struct()
    st.group_size = keep
    got = raw(None if null == "ctx" else ctx, None if null == "opt" else bpsw_hip.default_opt(), None if null == "group" else st, mode,
              None if null == "out_cnt" else cnt, regs, regs.shape[0], want_total=null != "out_total")
    assert (got[0], got[2]) == (code, text)
    assert (cnt == 0x5A5A5A5A).all() and (regs.view(np.uint8) == 0xA5).all()
    d_case_still_right(ctx, walked)


def test_a_bad_offset_under_a_skipped_orientation_is_not_looked_at(ctx, orc):
    """ref_off is read for the windows that become jobs only: the same offsets that refuse the call above, on rows 0 and 6 (failed
    orientations), change nothing"""
    g = _fr_pair_group()
    bad = _edit("ref_off", 6, -16)(_edit("ref_off", 0, g.ref_pool.size + 1)(g))
    want_cnt, want, n_sw, _ = orc.matesw_group(orc.default_opt(), g, po.RESCUE_C)
    assert n_sw == 2
    same(*ctx.matesw_group(bpsw_hip.default_opt(), bad), want_cnt, want)


def test_window_of_65535_rows_runs_and_one_of_65536_is_refused(ctx, orc, walked):
    rng = np.random.default_rng(0x65535)
    mate = rng.integers(0, 4, rc.L).astype(np.uint8)

    def group(rows):
        w = rng.integers(0, 4, rows).astype(np.uint8)
        w[rows - 190:rows - 40] = rc.revcomp(mate)              # the true locus in the last 200 rows
        p = rc.pair(rc.read_at(rc.A_F), mate, [rc.full(rc.A_F)], [], win={(0, 0, 1): (1000, 1000 + rows, w)})
        return rc.build([p], rc.PES_FR)

    g = group(65535)
    want_cnt, want, n_sw, _ = orc.matesw_group(orc.default_opt(), g, po.RESCUE_C)
    assert n_sw == 1 and want_cnt.tolist() == [1, 1] and want["score"][1] == rc.L
    s0 = ctx.stats()
    same(*ctx.matesw_group(bpsw_hip.default_opt(), g), want_cnt, want)
    assert ctx.stats().sw_jobs - s0.sw_jobs == 1
    g = group(65536)
    cnt, regs = out_buffers(g)
    code, _total, text = raw(ctx, bpsw_hip.default_opt(), g.as_struct(), po.RESCUE_C, cnt, regs, regs.shape[0])
    assert (code, text) == (-4, "matesw_group: window longer than the kernel limit")
    assert (cnt == 0x5A5A5A5A).all() and (regs.view(np.uint8) == 0xA5).all()
    d_case_still_right(ctx, walked)
