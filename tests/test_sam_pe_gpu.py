"""Paired-end reads to SAM: bpsw_sam_pe_batch_ex (the paired tail with a flags argument) and bpsw_align_pe_batch (paired reads to
text in one call), each with the text written on the calling thread and by sam_len_kernel / sam_write_kernel with a mate
(BPSW_SAM_TEXT_DEVICE).  Every comparison of text is byte for byte unless stated.

THE PAIRED FIXTURE READS.  The committed goldens and tail_util.synthetic_group hold no SA:Z tag, no 0x800 line and no pair with both
ends unmapped, so the mate columns of those lines would go uncompared.  The seeding fixture's 105 reads (genome g1) paired in the
order PAIR_ORDER (52 pairs) give all of them.  Census of the reference's own C text on the reference's regions, two contigs, all
four orientations failed -- asserted below as minimums on the expected text alone:
  flag 0        106 lines; 4 SA:Z; 2 with 0x800, both beside an unmapped mate (0x8); 2 hard-clipped; 2 of a both-unmapped pair;
                2 unmapped reads whose mate has two lines; 32 with RNEXT naming another contig; 18 with RNEXT = and TLEN 0
  ALL           239 lines; one read of 101 lines; 133 with 0x100, 6 of them with 0x8; 4 pairs with both reads multi-line; 13
                hard-clipped; 143 naming another contig
  ALL|NO_MULTI  239 lines; no 0x800; 8 with 0x100 and 0x8
and with orientation 1 = (low 1, high 2000, avg 300, std 100): 14 lines at flag 0 carry 0x2."""
import copy
import ctypes as C

import numpy as np
import pytest

import bpsw_hip
import fmi_util as fu
import pyoracle as po
from bpsw_hip import fmi, synth
from tail_util import load_sam_pe_golden, synthetic_group
from test_sam_se_gpu import NO_PES, TEXT_MODES, _contig_tables, _lines, _load, _pool, _reference_regions, fixture_reads, gold  # noqa: F401
from test_worker1_gpu import _opt

pytestmark = pytest.mark.gpu

PAIR_ORDER = [18, 2, 4, 29, 26, 19, 9, 10] + [i for i in range(104) if i not in (18, 2, 4, 29, 26, 19, 9, 10)]
PES_FR = [NO_PES[0], (1, 2000, 0, 300.0, 100.0), NO_PES[0], NO_PES[0]]
ALL, NO_MULTI = bpsw_hip.MEM_F_ALL, bpsw_hip.MEM_F_NO_MULTI
FLAGS3 = (0, ALL, ALL | NO_MULTI)


def _group_of(l_pac, reads, quals, names, reg_cnt, regs, table, pes, id0=500, with_quals=True):
    """a TailGroupSoA of consecutive reads (2k, 2k + 1) with one name per pair; regs: one array per read"""
    ln = np.array([len(r) for r in reads], np.int32)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int64)
    name_off, name_pool = _pool(names)
    a_off, a_pool = _pool([s.encode() for s in table[2]])
    empty = np.zeros(0, bpsw_hip.ALNREG_DTYPE)
    return bpsw_hip.TailGroupSoA(group_size=len(reads) // 2, l_pac=l_pac, id0=id0, pes=list(pes), read_len=ln, read_off=off,
                                 read_pool=np.concatenate(list(reads) + [np.zeros(1, np.uint8)]),
                                 qual_pool=np.concatenate(list(quals) + [np.zeros(1, np.uint8)]) if with_quals else None,
                                 name_off=name_off, name_pool=name_pool, reg_cnt=np.array(reg_cnt, np.int32),
                                 regs=np.ascontiguousarray(np.concatenate(list(regs) + [empty])), ann_off=np.array(table[0], np.int64),
                                 ann_len=np.array(table[1], np.int32), ann_name_off=a_off, ann_name_pool=a_pool)


def _paired_fixture(fixture_reads, reg_cnt, regs, table, pes, order=PAIR_ORDER, id0=500, names=None, with_quals=True):
    """the fixture's reads in `order` as pairs; reg_cnt / regs: per fixture read, flat"""
    g, idx, reads, quals, nm = fixture_reads
    at = np.concatenate([[0], np.cumsum(reg_cnt)])
    names = names if names is not None else [b"pair%d/%s" % (k, nm[order[2 * k]]) for k in range(len(order) // 2)]
    return _group_of(g.size, [reads[i] for i in order], [quals[i] for i in order], names, [int(reg_cnt[i]) for i in order],
                     [regs[at[i]:at[i + 1]] for i in order], table, pes, id0, with_quals)


def _census(want):
    f = _lines(want)
    per_read = [t.count(b"\n") for t in want]
    fl = [int(l[1]) for l in f]
    return dict(lines=len(f), most_lines=max(per_read), sa=sum(any(x.startswith(b"SA:Z:") for x in l) for l in f),
                supp=sum(bool(x & 0x800) for x in fl), supp_mate_unmapped=sum(x & 0x808 == 0x808 for x in fl),
                sec=sum(bool(x & 0x100) for x in fl), sec_mate_unmapped=sum(x & 0x108 == 0x108 for x in fl),
                hard=sum(b"H" in l[5] for l in f), both_unmapped=sum(x & 0xc == 0xc for x in fl),
                unmapped_at_two_line_mate=sum(per_read[r] == 1 and int(_lines([want[r]])[0][1]) & 0xc == 0x4 and per_read[r ^ 1] == 2
                                              for r in range(len(want))),
                both_multi=sum(per_read[2 * k] > 1 and per_read[2 * k + 1] > 1 for k in range(len(want) // 2)),
                other_contig=sum(l[6] not in (b"=", b"*") for l in f), same_tlen0=sum(l[6] == b"=" and l[8] == b"0" for l in f),
                proper=sum(bool(x & 0x2) for x in fl), tlen_pos=sum(int(l[8]) > 0 for l in f), tlen_neg=sum(int(l[8]) < 0 for l in f),
                mate_unmapped=sum(bool(x & 0x8) for x in fl), at_mate=sum(x & 0xc == 0x4 for x in fl))


def _assert_census(c, flag, pes):
    if flag == 0 and pes is NO_PES:
        assert c["lines"] >= 106 and c["sa"] >= 4 and c["supp"] >= 2 and c["supp_mate_unmapped"] >= 2 and c["hard"] >= 2, c
        assert c["both_unmapped"] >= 2 and c["unmapped_at_two_line_mate"] >= 2 and c["other_contig"] >= 32 and c["same_tlen0"] >= 18, c
    elif pes is not NO_PES:
        assert flag != 0 or c["proper"] >= 14, c
    elif flag == ALL:
        assert c["lines"] >= 239 and c["most_lines"] >= 101 and c["sec"] >= 133 and c["sec_mate_unmapped"] >= 6 and c["both_multi"] >= 4, c
        assert c["hard"] >= 13 and c["other_contig"] >= 143, c
    else:
        assert c["lines"] >= 239 and c["supp"] == 0 and c["sec_mate_unmapped"] >= 8, c


def _both_modes(ctx, opt, topt, g):
    """(text on the thread, out_regs) after checking that the device text and its out_regs are the same"""
    host, regs_h = ctx.sam_pe_batch(opt, topt, g, flags=0)
    dev, regs_d = ctx.sam_pe_batch(opt, topt, g, flags=bpsw_hip.SAM_TEXT_DEVICE)
    bad = [i for i in range(len(host)) if host[i] != dev[i]]
    assert not bad, (len(bad), host[bad[0]], dev[bad[0]])
    assert regs_h.tobytes() == regs_d.tobytes()
    return host, regs_h


def _ex(ctx, opt, topt, g, mode):
    """always through bpsw_sam_pe_batch_ex, flags 0 included"""
    st, keep, regs = bpsw_hip._pairs_struct(g)
    n = 2 * g.group_size
    off, need = np.zeros(n + 1, np.int64), C.c_size_t(0)
    out_regs = np.zeros(max(regs.shape[0], 1), bpsw_hip.ALNREG_DTYPE)
    rc = ctx.lib.bpsw_sam_pe_batch_ex(ctx.h, C.byref(opt), C.byref(topt), C.byref(st), mode, None, 0, bpsw_hip._ptr(off), C.byref(need), bpsw_hip._ptr(out_regs))
    assert rc == -3
    buf = np.zeros(need.value + 1, np.uint8)
    rc = ctx.lib.bpsw_sam_pe_batch_ex(ctx.h, C.byref(opt), C.byref(topt), C.byref(st), mode, bpsw_hip._ptr(buf), need.value, bpsw_hip._ptr(off), C.byref(need),
                                      bpsw_hip._ptr(out_regs))
    assert rc == 0, bpsw_hip.load_library().bpsw_last_error()
    text = buf[: int(off[-1])].tobytes()
    return [text[int(off[i]):int(off[i + 1])] for i in range(n)], out_regs[: regs.shape[0]]


# ---- 1. the reference's goldens --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", TEXT_MODES)
@pytest.mark.parametrize("stem", ["mem_sam_pe", "mem_sam_pe_all", "mem_sam_pe_rg"])
def test_sam_pe_ex_vs_reference_golden_text(ctx, stem, mode):
    pac, g, flag, want = load_sam_pe_golden(stem)
    ctx.ref_load(pac, g.l_pac)
    names = [bytes(g.ann_name_pool[int(g.ann_name_off[i]):int(g.ann_name_off[i + 1])]).decode() for i in range(g.ann_off.shape[0])]
    ctx.bns_load(g.ann_off, g.ann_len, names)
    opt = bpsw_hip.default_opt()
    opt.flag = flag
    topt = bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    topt.rg_id = g.rg_id
    got, _ = _ex(ctx, opt, topt, g, mode)
    assert got == want          # the reference's mem_sam_pe output, byte for byte
    ms, n_jobs = ctx.last_tail_kernel()
    assert n_jobs > 0 and ms > 0


# ---- 2. the paired fixture reads against the reference's C ---------------------------------------------------------------------------------
def _reference_text(ref, orc, gold, fixture_reads, ref_regions, table, flag, pes):
    pairs = _paired_fixture(fixture_reads, *ref_regions, table, pes)
    oopt, otopt = orc.default_opt(), orc.default_tail_opt()
    oopt.flag = flag
    return ref.sam_pe_batch(oopt, otopt, gold["g1_pac"], pairs, no_rescue=True), pairs


def test_sam_pe_fixture_pairs_vs_reference_c(ctx, ref, orc, gold, fixture_reads):
    g = fixture_reads[0]
    topt = bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    ref_regions = _reference_regions(ref, orc, gold, fixture_reads[2])
    for table in _contig_tables(g.size):
        _load(ctx, gold["g1_pac"], g.size, table)
        for pes in (NO_PES, PES_FR):
            for flag in FLAGS3:
                want, pairs = _reference_text(ref, orc, gold, fixture_reads, ref_regions, table, flag, pes)
                c = _census(want)
                print(len(table[0]), flag, "failed" if pes is NO_PES else "FR", c)
                if len(table[0]) == 2:
                    _assert_census(c, flag, pes)
                opt = bpsw_hip.default_opt()
                opt.flag = flag
                for mode in TEXT_MODES:
                    got, _ = _ex(ctx, opt, topt, pairs, mode)
                    bad = [i for i in range(len(want)) if want[i] != got[i]]
                    assert not bad, (len(table[0]), flag, mode, len(bad), want[bad[0]], got[bad[0]])


# ---- 3. against the oracle, both flavours ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_regions(orc, gold, fixture_reads):
    """the oracle's memChainToAln (BWA's z-drop) on the fixture's filtered chains, memSortAndDedup in C mode per read"""
    from test_worker1_gpu import _ref_chain_batch
    rb = fmi.ReadBatch.from_list(fixture_reads[2])
    cnt, regs, _, _ = orc.chain2aln_batch(orc.default_opt(), gold["g1_pac"], _ref_chain_batch(gold, "c1", rb, int(gold["g1_l_pac"])), po.ZDROP_BWA)
    out_cnt, out, at = [], [regs[0:0]], 0
    for c in cnt:
        r = orc.sort_dedup(regs[at:at + c], mode=po.RESCUE_C) if c else regs[0:0]
        at += c
        out_cnt.append(len(r)); out.append(r)
    return np.array(out_cnt, np.int32), np.concatenate(out)


@pytest.mark.parametrize("flavour", [bpsw_hip.TAIL_SCALA, bpsw_hip.TAIL_C])
def test_sam_pe_fixture_pairs_vs_oracle(ctx, orc, gold, fixture_reads, oracle_regions, flavour):
    g = fixture_reads[0]
    table = _contig_tables(g.size)[1]
    _load(ctx, gold["g1_pac"], g.size, table)
    for pes in (NO_PES, PES_FR):
        pairs = _paired_fixture(fixture_reads, *oracle_regions, table, pes)
        for flag, rg in ((0, b""), (ALL, b"run12.lane3"), (ALL | NO_MULTI, b""), (bpsw_hip.MEM_F_NOPAIRING, b""), (ALL | bpsw_hip.MEM_F_NOPAIRING, b"")):
            opt, oopt = bpsw_hip.default_opt(), orc.default_opt()
            opt.flag = oopt.flag = flag
            otopt, topt = orc.default_tail_opt(), bpsw_hip.default_tail_opt(flavour)
            otopt.rg_id = topt.rg_id = rg
            want, want_regs, _ = orc.sam_pe_batch(oopt, otopt, gold["g1_pac"], pairs, flavour=flavour)
            if flavour == bpsw_hip.TAIL_C and flag in FLAGS3:
                _assert_census(_census(want), flag, pes)
            for mode in TEXT_MODES:
                got, got_regs = _ex(ctx, opt, topt, pairs, mode)
                bad = [i for i in range(len(want)) if want[i] != got[i]]
                assert not bad, (flag, mode, len(bad), want[bad[0]], got[bad[0]])
                assert want_regs.tobytes() == got_regs.tobytes()
            assert all((b"\tRG:Z:run12.lane3" in w) == bool(rg) for w in want)


@pytest.fixture(scope="module")
def groups(orc):
    """read length -> (pac, 200 synthetic pairs): the mem_pair branch"""
    return {L: synthetic_group(orc, 200, 6100 + L, read_len=L, sub_rate=0.05, indel_rate=0.02, p_span=0.05, p_hard=0.2, p_unmappable=0.05)
            for L in (150, 250)}


@pytest.mark.parametrize("flavour", [bpsw_hip.TAIL_SCALA, bpsw_hip.TAIL_C])
@pytest.mark.parametrize("L", [150, 250])
def test_sam_pe_synthetic_pairs_vs_oracle(ctx, orc, groups, L, flavour):
    """Census of the oracle's text at flag 0 (measured on the oracle alone; asserted as rounded-down minimums): of 400 lines 334 proper,
    TLEN positive and negative 159 to 162 each, 26 to 29 with the mate unmapped, 24 to 27 placed at their mate, 24 to 26 naming another
    contig, one pair with both ends unmapped."""
    pac, g = groups[L]
    names = [bytes(g.ann_name_pool[int(g.ann_name_off[i]):int(g.ann_name_off[i + 1])]).decode() for i in range(g.ann_off.shape[0])]
    _load(ctx, pac, g.l_pac, (g.ann_off, g.ann_len, names))
    for flag in (0, ALL, bpsw_hip.MEM_F_NOPAIRING):
        opt, oopt = bpsw_hip.default_opt(), orc.default_opt()
        opt.flag = oopt.flag = flag
        want, want_regs, _ = orc.sam_pe_batch(oopt, orc.default_tail_opt(), pac, g, flavour=flavour)
        if flag == 0:
            c = _census(want)
            print(L, flavour, c)
            assert c["lines"] >= 400 and c["proper"] >= 300 and c["tlen_pos"] >= 150 and c["tlen_neg"] >= 150, c
            assert c["mate_unmapped"] >= 20 and c["at_mate"] >= 20 and c["other_contig"] >= 15, c
        for mode in TEXT_MODES:
            got, got_regs = _ex(ctx, opt, bpsw_hip.default_tail_opt(flavour), g, mode)
            bad = [i for i in range(len(want)) if want[i] != got[i]]
            assert not bad, (flag, mode, len(bad), want[bad[0]], got[bad[0]])
            assert want_regs.tobytes() == got_regs.tobytes()


# ---- 4., 5.: the library's own regions for the fixture's reads (no reference needed) -----------------------------------------------------------
@pytest.fixture(scope="module")
def own_regions(ctx, gold, fixture_reads):
    g, idx, reads, quals, names = fixture_reads
    _load(ctx, gold["g1_pac"], g.size, _contig_tables(g.size)[1], idx)
    cnt, regs = ctx.worker1_batch(bpsw_hip.default_opt(), _opt(gold, "c1"), fmi.ReadBatch.from_list(reads), zdrop_mode=bpsw_hip.ZDROP_BWA,
                                  flags=bpsw_hip.C2A_SORT_DEDUP)
    return cnt.copy(), regs.copy()


def _ready(ctx, gold, fixture_reads, names=True):
    g, idx = fixture_reads[0], fixture_reads[1]
    _load(ctx, gold["g1_pac"], g.size, _contig_tables(g.size)[1], idx, names=names)
    return _contig_tables(g.size)[1]


def test_device_text_at_the_line_counts_around_a_wavefront(ctx, gold, fixture_reads, own_regions):
    """one line per lane, 64 lanes a block: one pair; 31, 32 and 33 single-line pairs (62, 64, 66 lines); 32 pairs with one two-line
    read (65 lines: the last lines' mates lie in the block before); no pair at all"""
    table = _ready(ctx, gold, fixture_reads)
    opt, topt = bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    everything = list(range(104))
    per_read = [t.count(b"\n") for t in _both_modes(ctx, opt, topt, _paired_fixture(fixture_reads, *own_regions, table, NO_PES, order=everything))[0]]
    one, two = [i for i in everything if per_read[i] == 1], [i for i in everything if per_read[i] == 2]
    assert len(one) >= 66 and two
    for order, total in ((one[:2], 2), (one[:62], 62), (one[:64], 64), (one[:66], 66), (one[:63] + two[:1], 65), (two[:1] + one[:63], 65)):
        text, _ = _both_modes(ctx, opt, topt, _paired_fixture(fixture_reads, *own_regions, table, NO_PES, order=order))
        assert sum(t.count(b"\n") for t in text) == total
    empty = _group_of(fixture_reads[0].size, [], [], [], [], [], table, NO_PES)
    for mode in TEXT_MODES:
        assert _ex_empty(ctx, opt, topt, empty, mode) == 0


def _ex_empty(ctx, opt, topt, g, mode):
    st, keep, regs = bpsw_hip._pairs_struct(g)
    off, need = np.full(1, -1, np.int64), C.c_size_t(99)
    rc = ctx.lib.bpsw_sam_pe_batch_ex(ctx.h, C.byref(opt), C.byref(topt), C.byref(st), mode, None, 0, bpsw_hip._ptr(off), C.byref(need), None)
    assert rc == 0 and off[0] == 0 and need.value == 0
    return rc


def test_device_text_of_the_pair_with_a_hundred_lines(ctx, gold, fixture_reads, own_regions):
    """the pair holding the 101-line read: the mate's first line lies in another wavefront than most of the lines that read it"""
    table = _ready(ctx, gold, fixture_reads)
    opt, topt = bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    opt.flag = ALL
    text, _ = _both_modes(ctx, opt, topt, _paired_fixture(fixture_reads, *own_regions, table, NO_PES))
    per_read = [t.count(b"\n") for t in text]
    big = int(np.argmax(per_read))
    assert per_read[big] >= 101
    pair = [PAIR_ORDER[big & ~1], PAIR_ORDER[big | 1]]
    for order in (pair, pair[::-1], [0, 1, 3, 5] + pair, pair + [0, 1]):
        for flavour in (bpsw_hip.TAIL_SCALA, bpsw_hip.TAIL_C):
            t, _ = _both_modes(ctx, opt, bpsw_hip.default_tail_opt(flavour), _paired_fixture(fixture_reads, *own_regions, table, NO_PES, order=order))
            assert max(x.count(b"\n") for x in t) >= 101


def test_device_text_of_short_and_long_ends_and_names(ctx, gold, fixture_reads):
    """a pair of a one-base end without regions and an end of 256 bases; names of 1 and of 254 bytes"""
    table = _ready(ctx, gold, fixture_reads)
    g = fixture_reads[0]
    opt, so = bpsw_hip.default_opt(), _opt(gold, "c1")
    reads = [g[77:78], g[5000:5256], (3 - g[6000:6256][::-1]).astype(np.uint8), g[300:450]]
    cnt, regs = ctx.worker1_batch(opt, so, fmi.ReadBatch.from_list(reads), zdrop_mode=bpsw_hip.ZDROP_BWA, flags=bpsw_hip.C2A_SORT_DEDUP)
    assert cnt[0] == 0 and cnt[1] >= 1 and cnt[2] >= 1 and cnt[3] >= 1
    at = np.concatenate([[0], np.cumsum(cnt)])
    rng = np.random.default_rng(9)
    quals = [rng.integers(33, 127, len(r)).astype(np.uint8) for r in reads]
    for flavour in (bpsw_hip.TAIL_SCALA, bpsw_hip.TAIL_C):
        grp = _group_of(g.size, reads, quals, [b"q", b"n" * 254], cnt, [regs[at[i]:at[i + 1]] for i in range(4)], table, PES_FR, id0=5)
        text, _ = _both_modes(ctx, opt, bpsw_hip.default_tail_opt(flavour), grp)
        f = [_lines([t])[0] for t in text]
        assert f[0][0] == b"q" and int(f[0][1]) & 0xc == 0x4 and f[0][2] == f[1][2] and f[0][3] == f[1][3] and len(f[0][9]) == 1     # placed at its mate
        assert int(f[1][1]) & 0x8 and f[1][6] == b"=" and f[1][7] == f[1][3] and len(f[1][9]) == 256
        assert len(f[2][0]) == 254 and len(f[2][10]) == 256 and f[3][0] == b"n" * 254


def test_device_text_without_qualities_and_without_contig_names(ctx, gold, fixture_reads, own_regions):
    table = _ready(ctx, gold, fixture_reads, names=False)
    opt, topt = bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_SCALA)
    opt.flag = ALL
    text, _ = _both_modes(ctx, opt, topt, _paired_fixture(fixture_reads, *own_regions, table, NO_PES, with_quals=False))
    f = _lines(text)
    assert all(l[10] == b"*" for l in f) and any(l[2] == b"ctg2" for l in f) and any(l[6] in (b"ctg1", b"ctg2") for l in f)


@pytest.mark.parametrize("mode", TEXT_MODES)
def test_sam_pe_ex_text_capacity(ctx, gold, fixture_reads, own_regions, mode):
    table = _ready(ctx, gold, fixture_reads)
    opt, topt = bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    opt.flag = ALL
    pairs = _paired_fixture(fixture_reads, *own_regions, table, NO_PES)
    want, _ = ctx.sam_pe_batch(opt, topt, pairs)
    full = b"".join(want)
    want_off = np.concatenate([[0], np.cumsum([len(t) for t in want])])
    st, keep, regs = bpsw_hip._pairs_struct(pairs)
    off = np.zeros(2 * pairs.group_size + 1, np.int64)
    need = C.c_size_t(0)
    for cap in (0, 1, 777, len(full) - 1):
        buf = np.full(cap + 64, 0xAB, np.uint8)
        off[:] = -1
        rc = ctx.lib.bpsw_sam_pe_batch_ex(ctx.h, C.byref(opt), C.byref(topt), C.byref(st), mode, bpsw_hip._ptr(buf), cap, bpsw_hip._ptr(off),
                                          C.byref(need), None)
        assert rc == -3 and need.value == len(full) and np.array_equal(off, want_off), (cap, rc, need.value)
        assert (buf[cap:] == 0xAB).all()                                  # the guard bytes behind the buffer
    buf = np.full(need.value + 1, 0xAB, np.uint8)
    rc = ctx.lib.bpsw_sam_pe_batch_ex(ctx.h, C.byref(opt), C.byref(topt), C.byref(st), mode, bpsw_hip._ptr(buf), need.value, bpsw_hip._ptr(off),
                                      C.byref(need), None)
    assert rc == 0 and buf[:-1].tobytes() == full and buf[-1] == 0xAB
    for unknown in (2, mode | 4, -2):
        rc = ctx.lib.bpsw_sam_pe_batch_ex(ctx.h, C.byref(opt), C.byref(topt), C.byref(st), unknown, bpsw_hip._ptr(buf), need.value, bpsw_hip._ptr(off),
                                          C.byref(need), None)
        assert rc == -1


# ---- 6. reads to text --------------------------------------------------------------------------------------------------------------------
def test_align_pe_fixture_pairs(ctx, ref, orc, gold, fixture_reads):
    """(a) the text of bpsw_align_pe_batch is the composition the caller writes today -- worker1_batch on the 2n reads, pe_stat,
    worker2_batch -- and, with pes0 all failed (nothing to rescue), the reference's mem_sam_pe on the reference's regions"""
    g, idx, reads, quals, names = fixture_reads
    table = _contig_tables(g.size)[1]
    _load(ctx, gold["g1_pac"], g.size, table, idx)
    opt, so, topt = bpsw_hip.default_opt(), _opt(gold, "c1"), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    want_ref, _ = _reference_text(ref, orc, gold, fixture_reads, _reference_regions(ref, orc, gold, reads), table, 0, NO_PES)
    ordered = [reads[i] for i in PAIR_ORDER]
    cnt, regs = ctx.worker1_batch(opt, so, fmi.ReadBatch.from_list(ordered), zdrop_mode=bpsw_hip.ZDROP_BWA, flags=bpsw_hip.C2A_SORT_DEDUP)
    pes = bpsw_hip.pe_stat(opt, topt, g.size, cnt, regs)
    at = np.concatenate([[0], np.cumsum(cnt)])
    ident = list(range(104))
    by_hand = _group_of(g.size, ordered, [quals[i] for i in PAIR_ORDER], [b"pair%d/%s" % (k, names[PAIR_ORDER[2 * k]]) for k in range(52)], cnt,
                        [regs[at[i]:at[i + 1]] for i in ident], table, pes)
    want, _, _ = ctx.worker2_batch(opt, topt, by_hand, bpsw_hip.RESCUE_C)
    bare = copy.copy(by_hand)
    bare.reg_cnt, bare.regs, bare.pes = None, None, [(7, 7, 0, 7.0, 7.0)] * 4       # ignored
    for w1 in (0, bpsw_hip.W1_CHAIN_DEVICE):
        for mode in TEXT_MODES:
            got, got_pes = ctx.align_pe_batch(opt, so, topt, bare, zdrop_mode=bpsw_hip.ZDROP_BWA, w1_flags=w1, flags=mode)
            assert got_pes == pes
            bad = [i for i in range(len(want)) if want[i] != got[i]]
            assert not bad, (w1, mode, len(bad), want[bad[0]], got[bad[0]])
            got, got_pes = ctx.align_pe_batch(opt, so, topt, bare, pes0=NO_PES, zdrop_mode=bpsw_hip.ZDROP_BWA, w1_flags=w1, flags=mode)
            assert got_pes == [tuple(p) for p in NO_PES]
            bad = [i for i in range(len(want_ref)) if want_ref[i] != got[i]]
            assert not bad, (w1, mode, len(bad), want_ref[bad[0]], got[bad[0]])
    t = bpsw_hip.last_sam_pe_times()
    assert t[4] > 0 and t[6] > 0 and t[7] > 0 and t[0] > 0 and t[1] > 0 and all(x >= 0 for x in t)


def test_align_pe_refusals_and_no_pairs(ctx, gold, fixture_reads):
    g, idx, reads, quals, names = fixture_reads
    table = _contig_tables(g.size)[1]
    _load(ctx, gold["g1_pac"], g.size, table, idx)
    opt, so, topt = bpsw_hip.default_opt(), _opt(gold, "c1"), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    none = np.zeros(0, bpsw_hip.ALNREG_DTYPE)
    empty = _group_of(g.size, [], [], [], [], [], table, NO_PES)
    for mode in TEXT_MODES:
        text, pes = ctx.align_pe_batch(opt, so, topt, empty, flags=mode)
        assert text == [] and all(p[2] == 1 for p in pes)
    pair = _group_of(g.size, [g[:257], g[300:450]], [np.full(257, 70, np.uint8), np.full(150, 70, np.uint8)], [b"long"], [0, 0], [none, none], table, NO_PES)
    with pytest.raises(bpsw_hip.BpswError, match=r"\(-4\)"):     # a read of 257 bases: worker1's limit
        ctx.align_pe_batch(opt, so, topt, pair)
    ok = _group_of(g.size, [g[100:250], g[300:450]], [np.full(150, 70, np.uint8)] * 2, [b"ok"], [0, 0], [none, none], table, NO_PES)
    with pytest.raises(bpsw_hip.BpswError, match=r"\(-1\)"):     # an unknown flag
        ctx.align_pe_batch(opt, so, topt, ok, flags=2)
    ctx.fmi_unload()
    with pytest.raises(bpsw_hip.BpswError, match=r"\(-1\)"):     # no index
        ctx.align_pe_batch(opt, so, topt, ok)
    ctx.fmi_load(idx)
    text, _ = ctx.align_pe_batch(opt, so, topt, ok, zdrop_mode=bpsw_hip.ZDROP_BWA)
    assert len(text) == 2 and all(t.startswith(b"ok\t") for t in text)


def true_pairs(n_pairs=72, seed=4110):
    """a genome of 15 000 bases in three contigs and FR pairs of 150 bases with inserts of 200 to 400, every twelfth pair with an end
    of random bases -> (bases, contig table, reads, quals, names)"""
    rng = np.random.default_rng(seed)
    ln = [6000, 5000, 4000]
    g = rng.integers(0, 4, sum(ln)).astype(np.uint8)
    off = [0, ln[0], ln[0] + ln[1]]
    reads, quals, names = [], [], []
    for k in range(n_pairs):
        c = int(rng.integers(0, 3))
        ins = int(rng.integers(200, 401))
        p = off[c] + int(rng.integers(0, ln[c] - ins))
        a, b = g[p:p + 150].copy(), (3 - g[p + ins - 150:p + ins][::-1]).astype(np.uint8)
        for r in (a, b):
            at = rng.integers(0, 150, 3)
            r[at] = (r[at] + 1 + rng.integers(0, 3, 3)) % 4
        if k % 12 == 5:
            b = rng.integers(0, 4, 150).astype(np.uint8)
        if rng.random() < 0.5:
            a, b = b, a
        reads += [a, b]
        quals += [rng.integers(35, 74, 150).astype(np.uint8), rng.integers(35, 74, 150).astype(np.uint8)]
        names.append(b"tp%d" % k)
    return g, (off, ln, ["c1", "c2", "c3"]), reads, quals, names


def reference_pipeline(ref, orc, g, table, reads, quals, names, so_fields=None):
    """the reference's own C from reads to text: mem_chain + mem_chain_flt, mem_chain2aln, mem_sort_and_dedup, mem_pestat, mem_sam_pe"""
    rs = fu.RefSeeding(po.REF_SO)
    idx, _ = fu.build_index(g, 8)
    bwt = fu.ref_bwt(idx)
    d = rs.default_seed_fields()
    d.pop("w")
    o = rs.opt(d)
    cc, sc, seeds = [], [], []
    for r in reads:
        _, (ac, as_) = rs.chains(bwt, o, g.size, r)
        cc.append(len(ac)); sc += list(ac); seeds.append(as_)
    rs.libc.free(o)
    seeds = np.concatenate(seeds)
    rb = fmi.ReadBatch.from_list(reads)
    pac = fu.pack_pac(g)
    cb = bpsw_hip.ChainBatchSoA(l_pac=g.size, read_len=rb.read_len, read_off=rb.read_off, read_pool=rb.read_pool, chain_cnt=np.array(cc, np.int32),
                                seed_cnt=np.array(sc, np.int32), seed_rbeg=np.ascontiguousarray(seeds["rbeg"]),
                                seed_qbeg=np.ascontiguousarray(seeds["qbeg"]), seed_len=np.ascontiguousarray(seeds["len"]))
    oopt, otopt = orc.default_opt(), orc.default_tail_opt()
    rcnt, rregs = ref.chain2aln_batch(oopt, pac, cb)
    lists, at = [], 0
    for c in rcnt:
        lists.append(ref.sort_dedup(rregs[at:at + c]) if c else rregs[0:0])
        at += c
    cnt, regs = np.array([len(x) for x in lists], np.int32), np.concatenate(lists + [rregs[0:0]])
    pes = ref.pestat(oopt, otopt, g.size, cnt, regs)
    grp = _group_of(g.size, reads, quals, names, cnt, lists, table, pes, id0=40)
    return idx, pac, d, cnt, regs, pes, grp, ref.sam_pe_batch(oopt, otopt, pac, grp, no_rescue=False)


def strip_mapq_xs(line):
    f = line.rstrip(b"\n").split(b"\t")
    return [x for k, x in enumerate(f) if k != 4 and not x.startswith(b"XS:i:")]


@pytest.mark.skipif(not po.Ref.available(), reason="oracle/_ref/libbwaref.so not built (reference tree absent): the yardstick is the live reference pipeline")
def test_align_pe_true_pairs_vs_reference_pipeline(ctx, ref, orc):
    """(b) 72 FR pairs on a generated genome of three contigs against the reference from reads to text.  Region lists and statistics
    identical; the text may differ in MAPQ and XS:i only, on at most 5 % of the reads (the standing rule of
    test_tail_gpu.py::test_chains_to_sam_end_to_end_vs_reference)."""
    g, table, reads, quals, names = true_pairs()
    assert g.size <= 16_000 and len(reads) >= 128
    idx, pac, d, cnt, regs, pes, grp, want = reference_pipeline(ref, orc, g, table, reads, quals, names)
    assert pes[1][2] == 0 and all(pes[r][2] for r in (0, 2, 3))            # FR estimated, the others failed
    _load(ctx, pac, g.size, table, idx)
    opt, so, topt = bpsw_hip.default_opt(), fu.sopt_from(d), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    got_cnt, got_regs = ctx.worker1_batch(opt, so, fmi.ReadBatch.from_list(reads), zdrop_mode=bpsw_hip.ZDROP_BWA, flags=bpsw_hip.C2A_SORT_DEDUP)
    assert np.array_equal(got_cnt, cnt) and got_regs.tobytes() == regs.tobytes()
    bare = copy.copy(grp)
    bare.reg_cnt, bare.regs, bare.pes = None, None, list(NO_PES)
    for mode in TEXT_MODES:
        got, got_pes = ctx.align_pe_batch(opt, so, topt, bare, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=mode)
        assert got_pes == pes
        diff = [i for i in range(len(want)) if want[i] != got[i]]
        print("reads whose text differs:", len(diff), "of", len(want))
        assert len(diff) <= 0.05 * len(want), len(diff)
        for i in diff:
            wl, gl = want[i].splitlines(), got[i].splitlines()
            assert len(wl) == len(gl) and all(strip_mapq_xs(a) == strip_mapq_xs(b) for a, b in zip(wl, gl)), (want[i], got[i])
    assert sum(bool(int(l[1]) & 0x2) for l in _lines(want)) >= 100 and sum(bool(int(l[1]) & 0x4) for l in _lines(want)) >= 4
