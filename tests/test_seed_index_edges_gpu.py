"""bpsw_seed_batch (seed_smem_kernel + seed_sa_kernel, csrc/bpsw_seed.hip) on the index shapes that
tests/golden/seed_chain_small.npz avoids (tests/index_cases.py): seq_len a multiple of 128 and shorter than one block, `primary`
on a block's edge, in row 1 and in row seq_len, bases that do not occur, a suffix array with a single sample, interval lists at
read_len entries, reads with exactly 16 and 17 intervals around the first pass's rows of 16 records, the second pass on more reads
than its lanes.  The yardstick is tests/smem_plain.py -- seeding restated over the full suffix array, which tests/test_smem_plain.py
pins on the reference's C -- and the reference's recording itself (tests/golden/seed_index_edges.npz).  Every comparison is exact,
field by field, in value and order."""
import numpy as np
import pytest

import fmi_util as fu
import index_cases as ic
import smem_plain
from bpsw_hip import fmi

pytestmark = pytest.mark.gpu


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    for f in a.dtype.names:
        assert np.array_equal(a[f], b[f]), (what, f, int((a[f] != b[f]).sum()))


def _load(ctx, name, sa_intv=8):
    g, sa = ic.genome(name)
    idx, _ = fu.build_index(g, sa_intv, sa_full=sa)
    ctx.fmi_load(idx)
    assert ctx.fmi_length() == 2 * g.size
    return idx


def _check(got, iv, sd, what):
    """a seed_batch result against per-read lists of intervals and seeds"""
    icnt, ivs, scnt, sds = got
    wi, wiv = fu.flat(iv, fmi.SMEM_DTYPE)
    ws, wsd = fu.flat(sd, fmi.SEED_DTYPE)
    assert np.array_equal(icnt, wi), (what, "interval counts", np.nonzero(icnt != wi)[0][:8])
    _same(ivs, wiv, what + ": intervals")
    assert np.array_equal(scnt, ws), (what, "seed counts", np.nonzero(scnt != ws)[0][:8])
    _same(sds, wsd, what + ": seeds")


def _seed(ctx, optset, reads):
    return ctx.seed_batch(fu.sopt_from(ic.OPTION_SETS[optset]), reads if isinstance(reads, fmi.ReadBatch) else fmi.ReadBatch.from_list(list(reads)))


def _pick(name, optset, which):
    """the reads `which` of a genome with what the plain reference gives for them"""
    iv, sd = ic.expected(name, optset)
    r = ic.reads(name)
    return [r[k] for k in which], [iv[k] for k in which], [sd[k] for k in which]


@pytest.mark.parametrize("name", ic.GENOMES)
def test_every_row_of_the_index(ctx, name):
    """the four one-base reads with every interval kept: bwt_sa of every row from 1 to seq_len, against the suffix array itself --
    sampled every row, every 4th, every 32nd, and once (4 096 > seq_len: every walk ends at `primary`)"""
    g, sa_full = ic.genome(name)
    iv, sd = ic.expected(name, "every_row", True)
    for sa_intv in (1, 4, 32, 4096):
        idx = _load(ctx, name, sa_intv)
        assert idx.n_sa == (1 if sa_intv == 4096 else idx.seq_len // sa_intv + 1)
        got = _seed(ctx, "every_row", ic.ONE_BASE)
        seeds = fu.split(got[2], got[3])
        for c in range(4):
            rows = sa_full[idx.L2[c] + 1: idx.L2[c + 1] + 1]
            assert np.array_equal(seeds[c]["rbeg"], rows), (name, sa_intv, c, int((seeds[c]["rbeg"] != rows).sum()) if len(seeds[c]) == len(rows) else "count")
            assert np.all(seeds[c]["qbeg"] == 0) and np.all(seeds[c]["len"] == 1)
        assert int(got[2].sum()) == idx.seq_len
        _check(got, iv, sd, f"{name}, sa_intv {sa_intv}")


@pytest.mark.parametrize("name", ic.GENOMES)
def test_intervals_and_seeds_against_the_plain_reference(ctx, name):
    _load(ctx, name)
    rec = ic.recording()
    for optset in ic.OPTION_SETS:
        iv, sd = ic.expected(name, optset)
        got = _seed(ctx, optset, ic.reads(name))
        _check(got, iv, sd, f"{name} / {optset}")
        ic.check_recording(rec, f"{name}_{optset}", fu.split(got[0], got[1]), fu.split(got[2], got[3]))
        if optset == "max_occ_0":
            assert got[1].size and got[3].size == 0   # intervals, and no occurrence at all: the entry returns before seed_sa_kernel


def test_row_limit_of_the_first_pass(ctx):
    """rows of 16 records: a read with 16 intervals fits, one with 17 goes to the second pass"""
    name, optset = ic.ROW_LIMIT_BATCH
    _load(ctx, name)
    cnt = np.array([len(i) for i in ic.expected(name, optset)[0]])
    around = [int(np.nonzero(cnt == k)[0][0]) for k in (15, 16, 17, 18)]
    for order in (around, around[::-1]):
        r, iv, sd = _pick(name, optset, order)
        got = _seed(ctx, optset, r)
        assert got[0].tolist() == ([15, 16, 17, 18] if order is around else [18, 17, 16, 15])
        _check(got, iv, sd, f"reads with {got[0].tolist()} intervals")
    # the first and the last read of the batch overflow, the ones between do not
    over, under = np.nonzero(cnt > 16)[0], np.nonzero((cnt > 0) & (cnt <= 16))[0]
    order = [int(over[0])] + [int(k) for k in under[:70]] + [int(over[-1])]
    r, iv, sd = _pick(name, optset, order)
    _check(_seed(ctx, optset, r), iv, sd, "first and last read overflow")


def test_second_pass_on_more_reads_than_lanes(ctx):
    """64 resident lanes and more than 64 reads with over 16 intervals: the second pass takes its grid-stride path, every lane a second
    read from the todo list, with the room its row_base says"""
    name, optset = ic.ROW_LIMIT_BATCH
    _load(ctx, name)
    iv, sd = ic.expected(name, optset)
    assert sum(len(i) > 16 for i in iv) > 64
    ctx.lib.bpsw_seed_set_resident_lanes(64)
    try:
        got = _seed(ctx, optset, ic.reads(name))
    finally:
        ctx.lib.bpsw_seed_set_resident_lanes(0)
    _check(got, iv, sd, "64 resident lanes")


@pytest.mark.parametrize("optset", ["every_row", "no_exact"])
def test_lists_at_their_limit(ctx, optset):
    """reads of 256 bases whose interval shrinks with every base: the sweep's lists hold read_len entries, of list_cap = 257.  The call
    succeeds (no BPSW_ERR_DEVICE from the overflow flag) and gives what the plain reference gives"""
    _load(ctx, "runs")
    ix = ic.plain_index("runs")
    opt = ic.OPTION_SETS[optset]
    limit = ic.limit_reads()
    mixed = []
    for r in limit:
        mixed += ic.ONE_BASE + [r]
    mixed += ic.ONE_BASE
    for what, reads in (("alone", limit), ("among one-base reads", mixed)):
        iv = [smem_plain.intervals(ix, opt, r) for r in reads]
        sd = [smem_plain.seeds(ix, i) for i in iv]
        assert all(len(i) for r, i in zip(reads, iv) if len(r) == 256)
        _check(_seed(ctx, optset, reads), iv, sd, f"{optset}, {what}")


def test_pool_layout(ctx):
    """the reads laid into read_pool in reverse order, 1 to 7 bytes of filler between them, the last read of the pool ending on its last
    byte: read_off says where a read is, nothing else does"""
    name = "no_cg"
    _load(ctx, name)
    reads = ic.reads(name)
    gaps = [1 + k % 7 for k in range(len(reads))]
    ln = np.array([len(r) for r in reads], np.int32)
    off = np.zeros(len(reads), np.int64)
    pieces = []
    at = 0
    for k in range(len(reads) - 1, -1, -1):
        pieces.append(np.full(gaps[k], 4 if k % 2 else 0, np.uint8)); at += gaps[k]
        off[k] = at
        pieces.append(reads[k]); at += len(reads[k])
    pool = np.ascontiguousarray(np.concatenate(pieces))
    assert off[0] + ln[0] == pool.size and off[-1] == gaps[-1] and all(np.array_equal(pool[off[k]: off[k] + ln[k]], reads[k]) for k in range(len(reads)))
    for optset in ("defaults", "every_row"):
        iv, sd = ic.expected(name, optset)
        _check(_seed(ctx, optset, fmi.ReadBatch(ln, off, pool)), iv, sd, f"reversed pool, {optset}")


def test_reloads_between_indexes_of_different_size(ctx):
    """bpsw_fmi_load at seq_len 20 and 128 and with a single suffix-array sample, a larger index replaced by a smaller one and back:
    the length reported and the rows served are the new index's"""
    for name, sa_intv in (("runs", 8), ("tiny", 4096), ("one_block", 1), ("runs", 4096), ("tiny", 1), ("aligned_p_mid", 4096), ("one_block", 4096)):
        idx = _load(ctx, name, sa_intv)
        assert ctx.fmi_length() == idx.seq_len
        iv, sd = ic.expected(name, "every_row", True)
        _check(_seed(ctx, "every_row", ic.ONE_BASE), iv, sd, f"{name} after a reload, sa_intv {sa_intv}")
    ctx.fmi_unload()
    assert ctx.fmi_length() == 0
