"""The seeding plan on the device (BPSW_SEED_PLAN_DEVICE / BPSW_W1_SEED_PLAN_DEVICE: seed_plan_count_kernel, the three-launch scan of
csrc/bpsw_scan.hip, seed_plan_fill_kernel, then seed_sa_kernel unchanged on the device's tables) through bpsw_seed_batch_ex,
bpsw_worker1_batch and the two reads-to-text entries.

Every expectation is a committed recording of the reference (tests/golden/seed_chain_small.npz, tests/golden/seed_index_edges.npz
with the plain restatement tests/smem_plain.py that tests/test_smem_plain.py pins on it), the reference's chains through the round
loop, or the reference's / the oracle's SAM text -- never the same build's run without the flag.  Every comparison is exact, field by
field, in value and order.

The bus bytes are bounds stated from the layout, not from a run: with both flags the seeding stage fetches cnt (4 n bytes, and the
16-byte overflow word behind it, the pair rounded up to 16), then in one copy n_kept (8), read_occ (8 (n + 1)) and the plan's flag
words (16); it stages the read block and, when reads overflow the first pass's rows, their todo / base table."""
import copy

import numpy as np
import pytest

import bpsw_hip
import fmi_util as fu
import index_cases as ic
import pyoracle as po
from bpsw_hip import fmi
from conftest import region_fields_equal
from test_sam_pe_gpu import _paired_fixture
from test_sam_se_gpu import (NO_PES, TEXT_MODES, _contig_tables, _load, _pairs_with_a_one_base_mate, _single_end_of, fixture_reads,  # noqa: F401
                             gold)
from test_worker1_gpu import _opt, _ref_chain_batch

pytestmark = pytest.mark.gpu

PLAN = bpsw_hip.SEED_PLAN_DEVICE
W1_PLAN, W1_CHAIN = bpsw_hip.W1_SEED_PLAN_DEVICE, bpsw_hip.W1_CHAIN_DEVICE
N_READ = np.full(40, 4, np.uint8)   # all N: no interval, no seed


@pytest.fixture(scope="module")
def genomes(gold):
    """per genome of the fixture: bases, full suffix array (computed once), reads"""
    out = []
    for gi in (0, 1):
        l_pac = int(gold[f"g{gi}_l_pac"])
        g = fu.unpack_pac(gold[f"g{gi}_pac"], l_pac)
        _, sa = fu.build_index(g, 1)
        out.append((g, sa, fu.split(gold[f"g{gi}_read_len"], gold[f"g{gi}_read_pool"])))
    return out


@pytest.fixture(scope="module")
def c1(gold):
    """config c1 (genome 1, default options): per read the recorded intervals and seeds"""
    return fu.split(gold["c1_intv_cnt"], gold["c1_intv"]), fu.split(gold["c1_seed_cnt"], gold["c1_seeds"])


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    for f in a.dtype.names:
        assert np.array_equal(a[f], b[f]), (what, f, int((a[f] != b[f]).sum()))


def _check(got, iv, sd, what):
    """a seed_batch result against per-read lists of intervals and seeds; got[1] None: the call asked for no intervals"""
    icnt, ivs, scnt, sds = got
    wi, wiv = fu.flat(iv, fmi.SMEM_DTYPE)
    ws, wsd = fu.flat(sd, fmi.SEED_DTYPE)
    assert np.array_equal(icnt, wi), (what, "interval counts", np.nonzero(icnt != wi)[0][:8])
    if ivs is not None:
        _same(ivs, wiv, what + ": intervals")
    assert np.array_equal(scnt, ws), (what, "seed counts", np.nonzero(scnt != ws)[0][:8])
    _same(sds, wsd, what + ": seeds")


def _both_ways(ctx, so, reads, iv, sd, what):
    """through the flag with the intervals asked for and with intv == NULL; -> the first result"""
    rb = reads if isinstance(reads, fmi.ReadBatch) else fmi.ReadBatch.from_list(list(reads))
    got = ctx.seed_batch(so, rb, flags=PLAN)
    _check(got, iv, sd, what)
    bare = ctx.seed_batch(so, rb, flags=PLAN, intervals=False)
    assert bare[1] is None
    _check(bare, iv, sd, what + ", no intervals asked for")
    return got


# ---- 1. the goldens through the flag ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci,sa_intv", [(0, 1), (0, 32), (1, 8), (1, 1), (2, 32), (3, 8)])
def test_goldens_through_the_flag(ctx, gold, genomes, ci, sa_intv):
    gi = int(gold["configs"][ci][0])
    g, sa, reads = genomes[gi]
    ctx.fmi_load(fu.build_index(g, sa_intv, sa_full=sa)[0])
    key = f"c{ci}"
    rb = fmi.ReadBatch.from_list(reads)
    for intervals in (True, False):
        icnt, iv, scnt, sv = ctx.seed_batch(_opt(gold, key), rb, flags=PLAN, intervals=intervals)
        assert np.array_equal(icnt, gold[key + "_intv_cnt"])
        if intervals:
            _same(iv, gold[key + "_intv"], "intervals")
        else:
            assert iv is None
        assert np.array_equal(scnt, gold[key + "_seed_cnt"])
        _same(sv, gold[key + "_seeds"], "seeds")
    # flags == 0 is bpsw_seed_batch itself
    icnt, iv, scnt, sv = ctx.seed_batch(_opt(gold, key), rb, flags=0)
    assert np.array_equal(icnt, gold[key + "_intv_cnt"]) and np.array_equal(scnt, gold[key + "_seed_cnt"])
    _same(iv, gold[key + "_intv"], "intervals, flags 0")
    _same(sv, gold[key + "_seeds"], "seeds, flags 0")


# ---- 2. wavefront and grid-stride shapes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes_around_the_wavefront(ctx, gold, genomes, c1, n):
    g, sa, reads = genomes[1]
    ctx.fmi_load(fu.build_index(g, 8, sa_full=sa)[0])
    _both_ways(ctx, _opt(gold, "c1"), reads[:n], c1[0][:n], c1[1][:n], f"{n} reads")


def test_more_reads_than_resident_lanes(ctx, gold, genomes, c1):
    """128 resident lanes, the fixture's reads forward and reversed (210): every lane of seed_smem_kernel takes a second read"""
    g, sa, reads = genomes[1]
    ctx.fmi_load(fu.build_index(g, 8, sa_full=sa)[0])
    ctx.lib.bpsw_seed_set_resident_lanes(128)
    try:
        _both_ways(ctx, _opt(gold, "c1"), reads + reads[::-1], c1[0] + c1[0][::-1], c1[1] + c1[1][::-1], "forward and reversed")
    finally:
        ctx.lib.bpsw_seed_set_resident_lanes(0)


# ---- 3. index edge shapes -----------------------------------------------------------------------------------------------------------------------
def _load_case(ctx, name, sa_intv=8):
    g, sa = ic.genome(name)
    idx, _ = fu.build_index(g, sa_intv, sa_full=sa)
    ctx.fmi_load(idx)
    return idx


def _sopt(optset):
    return fu.sopt_from(ic.OPTION_SETS[optset])


def test_row_limit_of_the_first_pass(ctx):
    """reads with 15, 16, 17 and 18 intervals in both orders, a batch whose first and last read overflow, and the whole batch on 64
    resident lanes: more overflowing reads than the second pass has lanes, so the plan kernels look up rows of a todo list longer than a
    wavefront"""
    name, optset = ic.ROW_LIMIT_BATCH
    _load_case(ctx, name)
    iv, sd = ic.expected(name, optset)
    reads = ic.reads(name)
    cnt = np.array([len(i) for i in iv])
    around = [int(np.nonzero(cnt == k)[0][0]) for k in (15, 16, 17, 18)]
    over, under = np.nonzero(cnt > 16)[0], np.nonzero((cnt > 0) & (cnt <= 16))[0]
    assert over.size > 64
    for order in (around, around[::-1], [int(over[0])] + [int(k) for k in under[:70]] + [int(over[-1])]):
        _both_ways(ctx, _sopt(optset), [reads[k] for k in order], [iv[k] for k in order], [sd[k] for k in order], f"reads {order[:4]}...")
    ctx.lib.bpsw_seed_set_resident_lanes(64)
    try:
        got = _both_ways(ctx, _sopt(optset), reads, iv, sd, "64 resident lanes")
    finally:
        ctx.lib.bpsw_seed_set_resident_lanes(0)
    ic.check_recording(ic.recording(), f"{name}_{optset}", fu.split(got[0], got[1]), fu.split(got[2], got[3]))


@pytest.mark.parametrize("name", ["one_block", "no_cg", "a_only", "tiny"])
def test_index_edges_against_the_recording(ctx, name):
    """one_block: reads with 254 and 17 intervals; no_cg, a_only: kept zero-width intervals before and after non-empty ones (max_occ_0: a
    plan of zero-width intervals alone, n_kept > 0 and n_occ == 0); tiny: an index of 20 rows"""
    _load_case(ctx, name)
    rec = ic.recording()
    if name == "one_block":
        assert max(len(i) for i in ic.expected(name, "every_row")[0]) == 254
    if name in ("no_cg", "a_only"):
        c = ic.census(name, "every_row")
        assert c["zero_kept"] > 0
    for optset in ic.OPTION_SETS:
        iv, sd = ic.expected(name, optset)
        got = _both_ways(ctx, _sopt(optset), ic.reads(name), iv, sd, f"{name} / {optset}")
        ic.check_recording(rec, f"{name}_{optset}", fu.split(got[0], got[1]), fu.split(got[2], got[3]))
        if optset == "max_occ_0":
            assert got[1].size and got[3].size == 0


def test_zero_width_intervals_lie_before_and_after_real_ones():
    """what the two no-C/G genomes are in the batch for, counted on the plain reference (no device)"""
    t = [ic.census(n, o) for n in ("no_cg", "a_only") for o in ic.OPTION_SETS]
    assert any(c["zero_before_real"] for c in t) and any(c["zero_after_real"] for c in t)


@pytest.mark.parametrize("name", ["one_block", "tiny", "no_cg", "p_first", "p_last"])
def test_every_row_one_base_reads(ctx, name):
    """the four one-base reads with every interval kept: one interval a read, as wide as the base's row range"""
    rec = ic.recording()
    iv, sd = ic.expected(name, "every_row", True)
    for sa_intv in (1, 32):
        _load_case(ctx, name, sa_intv)
        got = _both_ways(ctx, _sopt("every_row"), ic.ONE_BASE, iv, sd, f"{name}, sa_intv {sa_intv}")
        ic.check_recording(rec, f"{name}_every_row_one", fu.split(got[0], got[1]), fu.split(got[2], got[3]))


# ---- 4. empty plans ------------------------------------------------------------------------------------------------------------------------------
def test_empty_plans(ctx, gold, genomes, c1):
    g, sa, reads = genomes[1]
    ctx.fmi_load(fu.build_index(g, 8, sa_full=sa)[0])
    so = _opt(gold, "c1")
    none_i, none_s = np.zeros(0, fmi.SMEM_DTYPE), np.zeros(0, fmi.SEED_DTYPE)
    for n in (1, 70):
        got = _both_ways(ctx, so, [N_READ] * n, [none_i] * n, [none_s] * n, f"{n} all-N reads")
        assert got[1].size == 0 and got[3].size == 0
    mid = [k for k in range(len(reads)) if len(c1[1][k])][:66]
    _both_ways(ctx, so, [N_READ] + [reads[k] for k in mid] + [N_READ], [none_i] + [c1[0][k] for k in mid] + [none_i],
               [none_s] + [c1[1][k] for k in mid] + [none_s], "first and last read without an interval")


# ---- 5. scan shapes ----------------------------------------------------------------------------------------------------------------------------
def _cycled(reads, c1, n):
    """n reads: the fixture's, cycled, every third one replaced by an all-N read -> (reads, expected intervals, expected seeds)"""
    none_i, none_s = np.zeros(0, fmi.SMEM_DTYPE), np.zeros(0, fmi.SEED_DTYPE)
    out, iv, sd, j = [], [], [], 0
    for k in range(n):
        if k % 3 == 2:
            out.append(N_READ); iv.append(none_i); sd.append(none_s)
        else:
            out.append(reads[j % len(reads)]); iv.append(c1[0][j % len(reads)]); sd.append(c1[1][j % len(reads)])
            j += 1
    return out, iv, sd


@pytest.mark.parametrize("n", [64, 65, 128, 129, 4096, 4097])
def test_scan_shapes_at_a_tile_of_64(ctx, gold, genomes, c1, n):
    """a tile of 64 items: 64 and 128 reads fill their tiles, 65 and 129 leave one item in the last; 4 096 reads give the second level
    exactly the 64 tile sums of its wavefront, 4 097 give it 65 and it loops with a carry"""
    g, sa, reads = genomes[1]
    ctx.fmi_load(fu.build_index(g, 8, sa_full=sa)[0])
    batch, iv, sd = _cycled(reads, c1, n)
    ctx.lib.bpsw_scan_set_tile(64)
    try:
        _both_ways(ctx, _opt(gold, "c1"), batch, iv, sd, f"{n} reads, tile 64")
    finally:
        ctx.lib.bpsw_scan_set_tile(0)


def test_scan_at_the_default_tile(ctx, gold, genomes, c1):
    """the same 4 097 reads at 2 048 items a tile: three tiles, the last with one item; and a tile size that is rounded up (100 -> 128)"""
    g, sa, reads = genomes[1]
    ctx.fmi_load(fu.build_index(g, 8, sa_full=sa)[0])
    batch, iv, sd = _cycled(reads, c1, 4097)
    _both_ways(ctx, _opt(gold, "c1"), batch, iv, sd, "4 097 reads, default tile")
    ctx.lib.bpsw_scan_set_tile(100)
    try:
        _both_ways(ctx, _opt(gold, "c1"), batch[:300], iv[:300], sd[:300], "300 reads, tile 100 -> 128")
    finally:
        ctx.lib.bpsw_scan_set_tile(0)


# ---- 6. bus bytes ----------------------------------------------------------------------------------------------------------------------------
def _align16(v):
    return (v + 15) & ~15


def test_bus_bytes_of_the_seeding_stage(ctx, gold, genomes, c1):
    g, sa, reads = genomes[1]
    ctx.ref_load(gold["g1_pac"], g.size)
    ctx.fmi_load(fu.build_index(g, 8, sa_full=sa)[0])
    n = 4097
    batch, iv, sd = _cycled(reads, c1, n)
    rb = fmi.ReadBatch.from_list(batch)
    opt, so = bpsw_hip.default_opt(), _opt(gold, "c1")
    read_block = _align16(4 * n) + _align16(8 * n) + _align16(rb.read_pool.size) + 16
    m = sum(len(i) > 16 for i in iv)                         # reads that overflow the first pass's rows of 16 records
    assert m > 0
    table = _align16(4 * m) + _align16(8 * (m + 1))          # their todo / base table, staged for the second pass and the plan kernels
    ctx.worker1_batch(opt, so, rb, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=W1_PLAN | W1_CHAIN)
    h2d, d2h = ctx.last_seed_bytes()
    print("both flags:", h2d, d2h, "bounds", read_block + 4096 + table, 4 * n + 8 * (n + 1) + 4096)
    assert 0 < d2h <= 4 * n + 8 * (n + 1) + 4096
    assert read_block <= h2d <= read_block + 4096 + table
    # without the new flag every read's row of 16 records of 40 bytes comes back: the counter counts
    ctx.worker1_batch(opt, so, rb, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=W1_CHAIN)
    h2d0, d2h0 = ctx.last_seed_bytes()
    print("chain flag alone:", h2d0, d2h0)
    assert d2h0 >= 640 * n and h2d0 > h2d
    # the plan flag alone: the seeds come back (16 bytes an occurrence), the intervals do not
    ctx.worker1_batch(opt, so, rb, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=W1_PLAN)
    n_occ = sum(int(i["x2"][i["kept"] != 0].sum()) for i in iv)
    assert ctx.last_seed_bytes()[1] <= 4 * n + 8 * (n + 1) + 4096 + 16 * n_occ + 16
    # ... and bpsw_seed_batch_ex with intv == NULL fetches the same
    ctx.seed_batch(so, rb, flags=PLAN, intervals=False)
    assert ctx.last_seed_bytes()[1] <= 4 * n + 8 * (n + 1) + 4096 + 16 * n_occ + 16


# ---- 7. worker1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w1", [W1_PLAN, W1_PLAN | W1_CHAIN])
@pytest.mark.parametrize("ci,flags", [(1, 0), (1, bpsw_hip.C2A_SORT_DEDUP), (2, 0), (3, bpsw_hip.C2A_SORT_DEDUP | bpsw_hip.C2A_DEDUP_SCALA)])
def test_worker1_equals_reference_chains_through_the_round_loop(ctx, gold, fixture_reads, ci, flags, w1):
    g, idx, reads = fixture_reads[:3]
    ctx.ref_load(gold["g1_pac"], g.size)
    ctx.fmi_load(idx)
    rb = fmi.ReadBatch.from_list(reads)
    opt, key = bpsw_hip.default_opt(), f"c{ci}"
    cnt, regs = ctx.worker1_batch(opt, _opt(gold, key), rb, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=flags | w1)
    wcnt, wregs = ctx.chain2aln_batch(opt, _ref_chain_batch(gold, key, rb, g.size), zdrop_mode=bpsw_hip.ZDROP_BWA, flags=flags)
    assert np.array_equal(cnt, wcnt) and cnt.sum() > len(reads) // 2
    region_fields_equal(regs, wregs)
    assert all(t >= 0 for t in bpsw_hip.last_worker1_times())


def test_worker1_flat_jni_passes_the_flag_through(ctx, gold, fixture_reads, monkeypatch):
    """worker1FlatJNI hands its flags to bpsw_worker1_batch: the regions with both flags are the ones of the reference's chains"""
    from bpsw_hip import jnishim
    monkeypatch.setenv("BPSW_ZDROP", "bwa")
    g, idx, reads = fixture_reads[:3]
    rb = fmi.ReadBatch.from_list(reads)
    opt, so = bpsw_hip.default_opt(), _opt(gold, "c2")
    ctx.ref_load(gold["g1_pac"], g.size)
    ctx.fmi_load(idx)
    fake = jnishim.load_fake_worker1()
    rc, cnt, longs, msg = jnishim.worker1_flat(fake, gold["g1_pac"], g.size, idx, opt, so, bpsw_hip.C2A_SORT_DEDUP | W1_PLAN | W1_CHAIN, rb)
    assert rc == 0, msg
    wcnt, wregs = ctx.chain2aln_batch(opt, _ref_chain_batch(gold, "c2", rb, g.size), zdrop_mode=bpsw_hip.ZDROP_BWA, flags=bpsw_hip.C2A_SORT_DEDUP)
    assert np.array_equal(cnt, wcnt) and longs.shape[0] == wregs.shape[0] > 0
    for k, f in enumerate(("rb", "re", "qb", "qe", "score", "truesc", "w", "seedcov")):
        assert np.array_equal(longs[:, k], wregs[f].astype(np.int64)), f


# ---- 8. reads to text ------------------------------------------------------------------------------------------------------------------------
def _regions(orc, gold, reads):
    """per read of the fixture the regions of its recorded chains after memSortAndDedup (C flavour): the reference's own mem_chain2aln
    where oracle/_ref is built, the oracle's memChainToAln with BWA's z-drop otherwise"""
    rb = fmi.ReadBatch.from_list(reads)
    b = _ref_chain_batch(gold, "c1", rb, int(gold["g1_l_pac"]))
    if po.Ref.available():
        cnt, regs = po.Ref().chain2aln_batch(orc.default_opt(), gold["g1_pac"], b)
    else:
        cnt, regs, _, _ = orc.chain2aln_batch(orc.default_opt(), gold["g1_pac"], b, po.ZDROP_BWA)
    out_cnt, out, at = [], [regs[0:0]], 0
    for c in cnt:
        r = orc.sort_dedup(regs[at:at + c], mode=po.RESCUE_C) if c else regs[0:0]
        at += c
        out_cnt.append(len(r)); out.append(r)
    return np.array(out_cnt, np.int32), np.concatenate(out)


def _pair_text(orc, pac, pairs):
    """mem_sam_pe without a rescue on `pairs`: the reference's text where oracle/_ref is built, the oracle's (C flavour) otherwise"""
    if po.Ref.available():
        return po.Ref().sam_pe_batch(orc.default_opt(), orc.default_tail_opt(), pac, pairs, no_rescue=True)
    return orc.sam_pe_batch(orc.default_opt(), orc.default_tail_opt(), pac, pairs, flavour=bpsw_hip.TAIL_C)[0]


def test_align_se_reads_to_text_with_both_flags(ctx, orc, gold, fixture_reads):
    """the text tests/test_sam_se_gpu.py expects for the fixture's reads: end 0 of pairs with a one-base mate, the pair's bits cleared"""
    g, idx, reads, quals, names = fixture_reads
    opt, so, topt = bpsw_hip.default_opt(), _opt(gold, "c1"), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    table = _contig_tables(g.size)[1]
    reg_cnt, regs = _regions(orc, gold, reads)
    pairs = _pairs_with_a_one_base_mate(g.size, reads, quals, names, reg_cnt, regs, table, 500)
    want = [_single_end_of(t) for t in _pair_text(orc, gold["g1_pac"], pairs)[0::2]]
    assert len(want) == len(reads) and sum(t.count(b"\n") for t in want) >= 107
    _load(ctx, gold["g1_pac"], g.size, table, idx)
    se = bpsw_hip.SeReadsSoA.from_lists(reads, names, quals, id0=1000, id_step=2)
    for w1 in (W1_PLAN, W1_PLAN | W1_CHAIN):
        for mode in TEXT_MODES:
            got = ctx.align_se_batch(opt, so, topt, se, zdrop_mode=bpsw_hip.ZDROP_BWA, w1_flags=w1, flags=mode)
            bad = [i for i in range(len(want)) if want[i] != got[i]]
            assert not bad, (w1, mode, len(bad), want[bad[0]], got[bad[0]])


def test_align_pe_reads_to_text_with_both_flags(ctx, orc, gold, fixture_reads):
    """the fixture's reads paired in PAIR_ORDER, every orientation failed (nothing to rescue): mem_sam_pe's text on the regions"""
    g, idx, reads, quals, names = fixture_reads
    opt, so, topt = bpsw_hip.default_opt(), _opt(gold, "c1"), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    table = _contig_tables(g.size)[1]
    pairs = _paired_fixture(fixture_reads, *_regions(orc, gold, reads), table, NO_PES)
    want = _pair_text(orc, gold["g1_pac"], pairs)
    assert len(want) == 104 and sum(t.count(b"\n") for t in want) >= 106
    _load(ctx, gold["g1_pac"], g.size, table, idx)
    bare = copy.copy(pairs)
    bare.reg_cnt, bare.regs, bare.pes = None, None, [(7, 7, 0, 7.0, 7.0)] * 4       # ignored
    for w1 in (W1_PLAN, W1_PLAN | W1_CHAIN):
        for mode in TEXT_MODES:
            got, got_pes = ctx.align_pe_batch(opt, so, topt, bare, pes0=NO_PES, zdrop_mode=bpsw_hip.ZDROP_BWA, w1_flags=w1, flags=mode)
            assert got_pes == [tuple(p) for p in NO_PES]
            bad = [i for i in range(len(want)) if want[i] != got[i]]
            assert not bad, (w1, mode, len(bad), want[bad[0]], got[bad[0]])


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, gold, genomes):
    g, sa, reads = genomes[0]
    idx, _ = fu.build_index(g, 8, sa_full=sa)
    so = bpsw_hip.default_seed_opt()
    ctx.fmi_load(idx)
    rb = fmi.ReadBatch.from_list(reads[:3])
    for flags in (2, PLAN | 2, 4, -1):
        with pytest.raises(bpsw_hip.BpswError, match=r"\(-1\)"):     # an unknown bit: BPSW_ERR_ARG
            ctx.seed_batch(so, rb, flags=flags)
    with pytest.raises(bpsw_hip.BpswError, match=r"\(-4\)"):         # 257 bases: BPSW_ERR_LIMIT
        ctx.seed_batch(so, fmi.ReadBatch.from_list([g[:257]]), flags=PLAN)
    icnt, iv, scnt, sv = ctx.seed_batch(so, fmi.ReadBatch.from_list([g[:256], g[:18], N_READ]), flags=PLAN)
    assert icnt[0] > 0 and scnt[0] > 0 and icnt[1] == 0 and scnt[1] == 0 and icnt[2] == 0 and scnt[2] == 0
    ctx.fmi_unload()
    with pytest.raises(bpsw_hip.BpswError, match=r"\(-1\)"):         # no index: BPSW_ERR_ARG
        ctx.seed_batch(so, rb, flags=PLAN)
    ctx.fmi_load(idx)
