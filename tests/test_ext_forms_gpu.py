"""Every named case of tests/ext_cases.py on every route of the extension, all ten output words == the oracle's.  tests/test_ext_cases.py
(no GPU) proves what each case reaches: a layout of csrc/bpsw_extend_rows.h and its changes, a phase of h1, a loop selector, an N row
at a chunk boundary, a z-drop at its margin, a tie, a full-kernel sweep.  Here the kernels run them at the shortcut masks 0 (pure DP),
16 (DP with the tail-row bound) and 63 (everything):
  * the resident short kernel (ext_resident_kernel): extend_batch on the small batches, the ring's counter says it went that way;
  * the launched short kernel (ext_kernel<., 1>): extend_batch_classify -- side_how rules the ring out --, and at masks 0 and 16 every
    non-empty side must have been SWEPT (how == 2): nothing named for a sweep form may be quietly taken by a shortcut;
  * the full kernel (ext_kernel<., 0>): the same tasks among more fillers with a 256-base flank than there are cases, so that
    2 n_long > n and the host sends the whole batch there: sw_extend_lean1 / lean2 / leanS / reg<3|4> with and without the hand-over /
    wave; flanks at the limits of include/bpsw.h, and one past each, which is refused;
  * a listed long task among short ones (n_long > 0 on the short kernel's launch);
  * the asynchronous device entry, where the short kernel defers the long tasks on its own."""
import os
import re

import numpy as np
import pytest

import bpsw_hip
import ext_cases as ec
import pyoracle as po

pytestmark = pytest.mark.gpu
MASKS = (0, 16, 63)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# csrc/bpsw_ring.h: the resident kernel's LDS holds target flanks of this many bases; longer ones take a launch
RING_RCAP = int(re.search(r"EXT_RING_RCAP = (\d+)", open(os.path.join(ROOT, "cloud-scale-bwamem_amd", "csrc", "bpsw_ring.h")).read()).group(1))


def _packed(orc, sc, cases):
    wire = bpsw_hip.wire_pack(ec.soa_of(cases, sc))
    want, _ = orc.wire_extend(wire, np.array(sc.mat, np.int8), sc.zdrop, sc.zmode)
    return sc, cases, wire, np.asarray(want)


@pytest.fixture(scope="module")
def tables(orc):
    """the oracle's records, computed once: `small` -- per Scoring the cases the resident kernel can hold --, `big` -- short flanks with a
    target beyond its LDS --, `long` -- the cases with a flank above 255 bases --, `mixed` -- small + long in one batch --, `full` --
    every case among its fillers"""
    def rlen(c):
        return max(len(s[1]) for s in (c.left, c.right) if s is not None)
    t = {"small": [], "big": [], "mixed": [], "full": []}
    for sc, cases in ec.batches(ec.cases()):
        short = [c for c in cases if not c.full_only]
        small = [c for c in short if rlen(c) <= RING_RCAP]
        big = [c for c in short if rlen(c) > RING_RCAP]
        long_ = [c for c in cases if c.full_only]
        assert len(small) <= 256                      # BPSW_EXT_RING_MAX_TASKS' default
        if small:
            t["small"].append(_packed(orc, sc, small))
        if big:
            t["big"].append(_packed(orc, sc, big))
        if long_:
            assert 2 * len(long_) <= len(short) + len(long_)          # use_short: the short kernel's launch, the long ones listed
            t["mixed"].append(_packed(orc, sc, short + long_) + (len(long_),))
        filler = [ec.one(f"filler{k}", [("M", 256), ("T", 10)], 50, sc, mat_max=cases[0].mat_max, salt=20 + k) for k in range(len(cases) + 1)]
        assert 2 * (len(filler) + len(long_)) > len(cases) + len(filler)   # !use_short: every task on the full kernel
        # (the fillers last: a case's index in the batch is its index in the table)
        t["full"].append(_packed(orc, sc, cases + filler))
    return t


def _with(ctx, sc, mask):
    ctx.set_ext_scoring(np.array(sc.mat, np.int8), sc.zdrop, sc.zmode)
    ctx.set_ext_shortcuts(mask)


@pytest.fixture
def restore(ctx):
    yield
    ctx.set_ext_scoring(po.default_mat(), 100, bpsw_hip.ZDROP_SCALA)     # (a null matrix would keep the one set last)
    ctx.set_ext_shortcuts(-1)


def _same(got, want, cases, what):
    got, want = np.asarray(got).reshape(-1, 10), want.reshape(-1, 10)
    bad = np.nonzero((got != want).any(axis=1))[0]
    names = [cases[k].name if k < len(cases) else "filler" for k in bad[:6]]
    assert bad.size == 0, f"{what}: {bad.size} tasks differ: {names}; first got {got[bad[0]]} want {want[bad[0]]}"


def _ring_expected(mask):
    """the extension ring takes an eligible small batch unless it is switched off, or the sift kernel runs in front of every batch (the
    forced-paths pass, tests/test_forced_paths_gpu.py: only with shortcut bit 32)"""
    off = os.environ.get("BPSW_EXT_RING", "1") == "0" or os.environ.get("BPSW_RING", "1") == "0" or os.environ.get("BPSW_RING_TEST_FAIL_LAUNCH")
    sifted = int(os.environ.get("BPSW_EXT_SIFT_MIN", "8192")) <= 1 and (mask & 32)
    return None if sifted else not off


@pytest.mark.parametrize("mask", MASKS)
def test_resident_short_kernel(ctx, tables, restore, mask):
    for sc, cases, wire, want in tables["small"]:
        _with(ctx, sc, mask)
        before = ctx.stats().ext_ring_calls
        got = ctx.extend_batch(wire)
        taken = ctx.stats().ext_ring_calls - before
        _same(got, want, cases, f"resident kernel, mask {mask}, w {sc.w}")
        if _ring_expected(mask) is not None:
            assert taken == (1 if _ring_expected(mask) else 0), (taken, sc)


@pytest.mark.parametrize("mask", MASKS)
def test_launched_short_kernel(ctx, tables, restore, mask):
    for sc, cases, wire, want in tables["small"] + tables["big"]:
        _with(ctx, sc, mask)
        before = ctx.stats().ext_ring_calls
        got, how = ctx.extend_batch_classify(wire)
        assert ctx.stats().ext_ring_calls == before
        _same(got, want, cases, f"short kernel, mask {mask}, w {sc.w}")
        sides = np.array([[c.left is not None, c.right is not None] for c in cases])
        if mask in (0, 16):
            assert np.array_equal(how, np.where(sides, 2, 0)), [c.name for c, h, s in zip(cases, how, sides) if (h != np.where(s, 2, 0)).any()]
        else:
            assert np.array_equal(how != 0, sides)


@pytest.mark.parametrize("mask", MASKS)
def test_full_kernel(ctx, tables, restore, mask):
    for sc, cases, wire, want in tables["full"]:
        _with(ctx, sc, mask)
        got, how = ctx.extend_batch_classify(wire)
        _same(got, want, cases, f"full kernel, mask {mask}, w {sc.w}")
        if mask in (0, 16):
            assert (how[how != 0] == 2).all()
        _same(ctx.extend_batch(wire), want, cases, f"full kernel (extend_batch), mask {mask}, w {sc.w}")


@pytest.mark.parametrize("mask", MASKS)
def test_a_listed_long_task_among_short_ones(ctx, tables, restore, mask):
    """flanks of 256 and BPSW_EXT_MAX_QLEN bases and a target of BPSW_EXT_MAX_RLEN between the short cases: the host lists them for the
    full kernel, which is launched with the short one -- no late launch (ext_full_relaunches stays where it is)"""
    assert tables["mixed"]
    for sc, cases, wire, want, n_long in tables["mixed"]:
        _with(ctx, sc, mask)
        before = ctx.stats().ext_full_relaunches
        _same(ctx.extend_batch(wire), want, cases, f"mixed batch, mask {mask}")
        assert ctx.stats().ext_full_relaunches == before


def test_one_past_each_limit_is_refused(ctx, restore):
    for c in ec.past_the_limits():
        wire = bpsw_hip.wire_pack(ec.soa_of([c], c.sc))
        with pytest.raises(bpsw_hip.BpswError):
            ctx.extend_batch(wire)
    # ... and the context still computes
    c = ec.cases()[0]
    assert ctx.extend_batch(bpsw_hip.wire_pack(ec.soa_of([c], c.sc))).size == 10


def test_asynchronous_device_entry(ctx, tables, restore):
    """extend_batch_device over the table: nobody has seen the records, the short kernel defers the flanks above 255 bases itself"""
    import torch
    for sc, cases, wire, want, *_ in tables["small"] + tables["big"] + tables["mixed"]:
        _with(ctx, sc, -1)
        n = len(cases)
        d_wire = torch.from_numpy(wire.copy()).to("cuda:0")
        d_out = torch.zeros(10 * n, dtype=torch.int16, device="cuda:0")
        torch.cuda.synchronize()
        ctx.extend_batch_device(d_wire.data_ptr(), wire.size, n, d_out.data_ptr())
        ctx.last_kernel_ms()
        torch.cuda.synchronize()
        _same(d_out.cpu().numpy(), want, cases, f"device entry, w {sc.w}")
