"""The sift kernel (csrc/bpsw_extend_sift.hip) on flanks that hold N: an N column is a deficit column of its own weight, judged one
task per lane instead of being handed to ext_kernel as a ticket.  Batches of 8 192 tasks -- the sift's launch threshold, the
smallest batch that reaches the kernel at the library's defaults.  Each case: results equal the oracle's, and the per-side verdicts
(bpsw_extend_batch_classify: shortcut / DP swept) are the same with the sift in front (shortcut bit 32) and without it -- the sift
resolves neither more nor fewer sides than ext_kernel's wave-wide forms.  tests/test_sift_n_host.py holds the same arithmetic
against the DP on a CPU."""
import numpy as np
import pytest

import bpsw_hip
from bpsw_hip import synth
import pyoracle as po

pytestmark = pytest.mark.gpu

N_TASKS = 8192


def _mat(a, mm, sn):
    m = np.full((5, 5), sn, np.int8)
    m[:4, :4] = mm
    for i in range(4):
        m[i, i] = a
    return m.reshape(-1)


def _same_with_and_without_the_sift(c, wire, want, mat=None):
    try:
        if mat is not None:
            c.set_ext_scoring(mat, 100, po.ZDROP_SCALA)
        c.set_ext_shortcuts(31)
        out0, how0 = c.extend_batch_classify(wire)
        c.set_ext_shortcuts(31 | 32)
        out1, how1 = c.extend_batch_classify(wire)
    finally:
        c.set_ext_shortcuts(-1)
        if mat is not None:
            c.set_ext_scoring(po.default_mat(), 100, po.ZDROP_SCALA)     # (a null matrix would keep the one set above)
    assert np.array_equal(out0, want) and np.array_equal(out1, want)
    diff = np.argwhere(how0 != how1)
    assert diff.size == 0, f"{len(diff)} sides judged differently; first (task, side) {diff[0]}: {how0[tuple(diff[0])]} without the sift, {how1[tuple(diff[0])]} with it"
    return how1


# 150 bp reads at two N rates (2 %: most flanks hold one, several columns each; 0.1 %: the bench's own rate), 100 bp reads, and a
# matrix of the family whose N score is below its mismatch score (dn 4 above dm 2: a gain of dn, a loss at a deficit column)
@pytest.mark.parametrize("read_len,n_rate,mat", [(150, 0.02, None), (150, 0.001, None), (100, 0.02, None), (150, 0.02, _mat(1, -1, -3))])
def test_flanks_with_n_through_the_sift(ctx, orc, read_len, n_rate, mat):
    soa = synth.ext_tasks(10000, read_len=read_len, sub_rate=0.01, indel_rate=0.001, n_rate=n_rate, seed=4400 + read_len + int(n_rate * 1e4))
    assert soa.n >= N_TASKS
    soa = soa.subset(slice(0, N_TASKS))
    pool = soa.pool.copy()
    pool[np.random.default_rng(read_len).random(pool.size) < n_rate / 2] = 4     # N in the target flanks as well
    soa.pool = pool
    wire = bpsw_hip.wire_pack(soa)
    want, _ = orc.wire_extend(wire, mat)
    how = _same_with_and_without_the_sift(ctx, wire, np.asarray(want).reshape(-1), mat)
    assert (how == 1).sum() > 0.3 * (how != 0).sum()          # the batch does exercise the forms


def test_coordinate_batch_with_n_in_the_reads(orc):
    """ext_sift_kernel<true>: the target flanks come from the resident 2-bit reference (no N there), the N are in the query"""
    c = bpsw_hip.Context(0)
    try:
        l_pac = 2_000_003
        pac = synth.hash_pac(l_pac, seed=291)
        c.ref_load(pac, l_pac)
        by, co = synth.ext_tasks_ref(6000, pac, l_pac, read_len=150, sub_rate=0.01, indel_rate=0.001, n_rate=0.02, seed=292)
        assert by.n >= N_TASKS and (co.seed_rbeg[:N_TASKS] >= l_pac).any() and (co.seed_rbeg[:N_TASKS] < l_pac).any()
        sel = slice(0, N_TASKS)
        by = by.subset(sel)
        co = bpsw_hip.ExtCoordTaskSoA(pool=co.pool, **{k: np.ascontiguousarray(getattr(co, k)[sel]) for k in (
            "left_qlen", "left_rlen", "right_qlen", "right_rlen", "left_q_off", "right_q_off", "reg_score", "q_beg", "h0", "idx",
            "seed_len", "seed_rbeg")})
        assert (by.pool == 4).any()
        want, _ = orc.wire_extend(bpsw_hip.wire_pack(by))
        how = _same_with_and_without_the_sift(c, bpsw_hip.wire_coords_pack(co), np.asarray(want).reshape(-1))
        assert (how == 1).sum() > 0.3 * (how != 0).sum()
    finally:
        c.close()
