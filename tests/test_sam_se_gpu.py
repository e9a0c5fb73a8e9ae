"""Single-end reads to SAM: bpsw_sam_se_batch (singleEndBwaMemWorker2 for a batch) and bpsw_align_se_batch (reads to text in one
call), each with the text written on the calling thread and by sam_len_kernel / sam_write_kernel (BPSW_SAM_TEXT_DEVICE).

Every comparison is byte for byte.  The reference has no single-end entry in the shim, so its single-end text is derived from
mem_sam_pe on pairs whose second end is a one-base read without regions: the reference then prints end 0 through mem_reg2sam_se,
marked primary with id (id0 + k) << 1, and the single-end line is that line with the pair's flag bits (0x1 0x2 0x8 0x20 0x40 0x80)
cleared and the mate columns replaced by * 0 0 -- mem_aln2sam reads the mate for nothing else.  The same derivation on the
oracle's text gives the Scala flavour's expectation.  So the single-end call is made with id0 = 2 * pair_id0 and id_step = 2."""
import ctypes as C

import numpy as np
import pytest

import bpsw_hip
import fmi_util as fu
import pyoracle as po
from bpsw_hip import fmi
from tail_util import synthetic_group
from test_worker1_gpu import _opt, _ref_chain_batch

pytestmark = pytest.mark.gpu

PAIR_BITS = 0x1 | 0x2 | 0x8 | 0x20 | 0x40 | 0x80
NO_PES = [(0, 0, 1, 0.0, 0.0)] * 4
TEXT_MODES = [0, bpsw_hip.SAM_TEXT_DEVICE]


def _single_end_of(pair_text: bytes) -> bytes:
    out = []
    for line in pair_text.split(b"\n")[:-1]:
        f = line.split(b"\t")
        f[1] = str(int(f[1]) & ~PAIR_BITS).encode()
        f[6:9] = [b"*", b"0", b"0"]
        out.append(b"\t".join(f) + b"\n")
    return b"".join(out)


def _lines(texts):
    return [ln.split(b"\t") for t in texts for ln in t.split(b"\n")[:-1]]


def _pool(strs):
    off = np.zeros(len(strs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in strs])
    return off, np.frombuffer(b"".join(strs) + b"\0", np.uint8).copy()


@pytest.fixture(scope="module")
def gold():
    return np.load(fu.GOLDEN)


@pytest.fixture(scope="module")
def fixture_reads(gold):
    """genome g1 of the seeding fixture: bases, index (sa_intv 8), its 105 reads with names and qualities"""
    l_pac = int(gold["g1_l_pac"])
    g = fu.unpack_pac(gold["g1_pac"], l_pac)
    idx, _ = fu.build_index(g, 8)
    reads = fu.split(gold["g1_read_len"], gold["g1_read_pool"])
    rng = np.random.default_rng(105)
    quals = [rng.integers(35, 74, len(r)).astype(np.uint8) for r in reads]
    names = [b"frag%d/%s" % (i, b"x" * (i % 7)) for i in range(len(reads))]
    return g, idx, reads, quals, names


def _contig_tables(l_pac):
    return [([0], [l_pac], ["chrA"]), ([0, l_pac // 3], [l_pac // 3, l_pac - l_pac // 3], ["chrA", "chrB.second"])]


def _load(ctx, pac, l_pac, table, idx=None, names=True):
    ctx.ref_load(pac, l_pac)
    ctx.bns_load(np.array(table[0], np.int64), np.array(table[1], np.int32), table[2] if names else None)
    if idx is not None:
        ctx.fmi_load(idx)


def _reference_regions(ref, orc, gold, reads):
    """the reference's mem_chain2aln on the fixture's filtered chains, then memSortAndDedup per read (C flavour)"""
    rb = fmi.ReadBatch.from_list(reads)
    cnt, regs = ref.chain2aln_batch(orc.default_opt(), gold["g1_pac"], _ref_chain_batch(gold, "c1", rb, int(gold["g1_l_pac"])))
    out_cnt, out, at = [], [regs[0:0]], 0
    for c in cnt:
        r = orc.sort_dedup(regs[at:at + c], mode=po.RESCUE_C) if c else regs[0:0]
        at += c
        out_cnt.append(len(r)); out.append(r)
    return np.array(out_cnt, np.int32), np.concatenate(out)


def _pairs_with_a_one_base_mate(l_pac, reads, quals, names, reg_cnt, regs, table, pair_id0):
    two_r, two_q, cnt2 = [], [], []
    for i, r in enumerate(reads):
        two_r += [r, np.zeros(1, np.uint8)]
        two_q += [quals[i], np.full(1, 73, np.uint8)]
        cnt2 += [int(reg_cnt[i]), 0]
    ln = np.array([len(r) for r in two_r], np.int32)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int64)
    name_off, name_pool = _pool(names)
    a_off, a_pool = _pool([s.encode() for s in table[2]])
    return bpsw_hip.TailGroupSoA(group_size=len(reads), l_pac=l_pac, id0=pair_id0, pes=list(NO_PES), read_len=ln, read_off=off,
                                 read_pool=np.concatenate(two_r), qual_pool=np.concatenate(two_q), name_off=name_off, name_pool=name_pool,
                                 reg_cnt=np.array(cnt2, np.int32), regs=np.ascontiguousarray(regs), ann_off=np.array(table[0], np.int64),
                                 ann_len=np.array(table[1], np.int32), ann_name_off=a_off, ann_name_pool=a_pool)


def _expected_c(ref, orc, gold, fixture_reads, table, flag, pair_id0=500):
    """(the reference's single-end text per read, reg_cnt, regs) for the fixture's reads"""
    g, idx, reads, quals, names = fixture_reads
    reg_cnt, regs = _reference_regions(ref, orc, gold, reads)
    pairs = _pairs_with_a_one_base_mate(g.size, reads, quals, names, reg_cnt, regs, table, pair_id0)
    oopt, otopt = orc.default_opt(), orc.default_tail_opt()
    oopt.flag = flag
    text = ref.sam_pe_batch(oopt, otopt, gold["g1_pac"], pairs, no_rescue=True)
    mates = _lines(text[1::2])
    assert all(int(f[1]) & 0x4 and f[9] in (b"A", b"T") for f in mates)          # the one-base mates: unmapped, nothing else
    raw = _lines(text[0::2])
    assert {int(f[1]) & PAIR_BITS for f in raw} <= {73, 105}                        # what the derivation clears ...
    assert all((f[6], f[8]) in ((b"=", b"0"), (b"*", b"0")) for f in raw)           # ... and replaces
    return [_single_end_of(t) for t in text[0::2]], reg_cnt, regs


def _census(want):
    f = _lines(want)
    per_read = [t.count(b"\n") for t in want]
    return dict(lines=len(f), two_line_reads=sum(n == 2 for n in per_read), most_lines=max(per_read), sa=sum(any(x.startswith(b"SA:Z:") for x in l) for l in f),
                supp=sum(bool(int(l[1]) & 0x800) for l in f), sec=sum(bool(int(l[1]) & 0x100) for l in f), hard=sum(b"H" in l[5] for l in f),
                unmapped=sum(bool(int(l[1]) & 0x4) for l in f), reverse=sum(bool(int(l[1]) & 0x10) for l in f))


def _se(fixture_reads, reg_cnt, regs, id0=1000, id_step=2, which=None, names=None, quals=True):
    g, idx, reads, qs, nm = fixture_reads
    which = range(len(reads)) if which is None else which
    at = np.concatenate([[0], np.cumsum(reg_cnt)])
    names = names if names is not None else [nm[i] + b"." + str(k).encode() for k, i in enumerate(which)]
    sub = [regs[at[i]:at[i + 1]] for i in which]
    return bpsw_hip.SeReadsSoA.from_lists([reads[i] for i in which], names, [qs[i] for i in which] if quals else None,
                                          reg_cnt=np.array([len(s) for s in sub], np.int32), regs=np.concatenate(sub + [regs[0:0]]), id0=id0, id_step=id_step)


# ---- 1. against the reference's C -------------------------------------------------------------------------------------------------
def test_sam_se_vs_reference_c(ctx, ref, orc, gold, fixture_reads):
    """Census of the reference's own text (minimums, so that the input cannot quietly degenerate; measured on the reference alone):
    flag 0: 107 lines, 2 reads of two lines, 4 SA:Z tags, 2 lines with 0x800, 2 hard-clipped CIGARs, 9 unmapped reads, 46
    reverse-strand lines; MEM_F_ALL: 240 lines, 133 with 0x100, 13 hard-clipped, one read of 101 lines; MEM_F_NO_MULTI: 107 lines,
    2 with 0x100, none with 0x800."""
    g, idx, reads, quals, names = fixture_reads
    assert len(reads) == 105
    topt = bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    for table in _contig_tables(g.size):
        _load(ctx, gold["g1_pac"], g.size, table)
        for flag in (0, bpsw_hip.MEM_F_ALL, bpsw_hip.MEM_F_NO_MULTI):
            want, reg_cnt, regs = _expected_c(ref, orc, gold, fixture_reads, table, flag)
            c = _census(want)
            print(len(table[0]), flag, c)
            if flag == 0:
                assert c["lines"] >= 107 and c["two_line_reads"] >= 2 and c["sa"] >= 4 and c["supp"] >= 2 and c["hard"] >= 2, c
                assert c["unmapped"] >= 9 and c["reverse"] >= 46, c
            elif flag == bpsw_hip.MEM_F_ALL:
                assert c["lines"] >= 240 and c["sec"] >= 133 and c["hard"] >= 13 and c["most_lines"] >= 101, c
            else:
                assert c["lines"] >= 107 and c["sec"] >= 2 and c["supp"] == 0, c
            opt = bpsw_hip.default_opt()
            opt.flag = flag
            names2 = list(names)
            se = bpsw_hip.SeReadsSoA.from_lists(reads, names2, quals, reg_cnt=reg_cnt, regs=regs, id0=2 * 500, id_step=2)
            for mode in TEXT_MODES:
                got, _ = ctx.sam_se_batch(opt, topt, se, flags=mode)
                bad = [i for i in range(len(want)) if want[i] != got[i]]
                assert not bad, (len(table[0]), flag, mode, len(bad), want[bad[0]], got[bad[0]])
    ms, n_jobs = ctx.last_tail_kernel()
    assert n_jobs > 0 and ms > 0 and all(t >= 0 for t in ctx.last_tail_host_ms())


# ---- 2. against the oracle, both flavours -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def groups(orc):
    """read length -> (pac, group of 200 pairs with every odd end's regions dropped)"""
    out = {}
    for L, es, ei in ((150, 0.05, 0.02), (250, 0.05, 0.02)):
        pac, g = synthetic_group(orc, 200, 6100 + L, read_len=L, sub_rate=es, indel_rate=ei, p_span=0.05)
        at = np.concatenate([[0], np.cumsum(g.reg_cnt)])
        keep = [g.regs[at[r]:at[r + 1]] for r in range(0, 2 * g.group_size, 2)]
        g.reg_cnt = g.reg_cnt.copy()
        g.reg_cnt[1::2] = 0
        g.regs = np.ascontiguousarray(np.concatenate(keep))
        out[L] = (pac, g)
    return out


def _se_of_group(g, quals=True):
    names = g.name_pool
    return bpsw_hip.SeReadsSoA(read_len=np.ascontiguousarray(g.read_len[0::2]), read_off=np.ascontiguousarray(g.read_off[0::2]), read_pool=g.read_pool,
                               qual_pool=g.qual_pool if quals else None, name_off=g.name_off, name_pool=names,
                               reg_cnt=np.ascontiguousarray(g.reg_cnt[0::2]), regs=g.regs, id0=2 * g.id0, id_step=2)


@pytest.mark.parametrize("mode", TEXT_MODES)
@pytest.mark.parametrize("flavour", [bpsw_hip.TAIL_SCALA, bpsw_hip.TAIL_C])
@pytest.mark.parametrize("L", [150, 250])
def test_sam_se_vs_oracle(ctx, orc, groups, L, flavour, mode):
    pac, g = groups[L]
    names = [bytes(g.ann_name_pool[int(g.ann_name_off[i]):int(g.ann_name_off[i + 1])]).decode() for i in range(g.ann_off.shape[0])]
    _load(ctx, pac, g.l_pac, (g.ann_off, g.ann_len, names))
    for flag, rg in ((0, b""), (bpsw_hip.MEM_F_ALL, b"run12.lane3"), (bpsw_hip.MEM_F_ALL | bpsw_hip.MEM_F_NO_MULTI, b"")):
        opt, oopt = bpsw_hip.default_opt(), orc.default_opt()
        opt.flag = oopt.flag = flag
        otopt, topt = orc.default_tail_opt(), bpsw_hip.default_tail_opt(flavour)
        otopt.rg_id = topt.rg_id = rg
        pair_text, want_regs, _ = orc.sam_pe_batch(oopt, otopt, pac, g, flavour=flavour)
        want = [_single_end_of(t) for t in pair_text[0::2]]
        got, got_regs = ctx.sam_se_batch(opt, topt, _se_of_group(g), flags=mode)
        bad = [i for i in range(len(want)) if want[i] != got[i]]
        assert not bad, (flag, len(bad), want[bad[0]], got[bad[0]])
        assert all((b"\tRG:Z:run12.lane3" in w) == bool(rg) for w in want)
        assert want_regs.tobytes() == got_regs.tobytes()                 # out_regs: the oracle's end-0 lists after mark-primary
        assert len(_lines(want)) > len(want) or flag == 0


@pytest.mark.parametrize("mode", TEXT_MODES)
def test_sam_se_without_qualities_and_contig_names(ctx, orc, groups, mode):
    import copy
    pac, g = groups[150]
    g2 = copy.copy(g)
    g2.qual_pool = None
    g2.ann_name_off, g2.ann_name_pool = _pool([b"ctg%d" % (i + 1) for i in range(g.ann_off.shape[0])])
    _load(ctx, pac, g.l_pac, (g.ann_off, g.ann_len, None), names=False)
    opt, oopt = bpsw_hip.default_opt(), orc.default_opt()
    opt.flag = oopt.flag = bpsw_hip.MEM_F_ALL
    pair_text, _, _ = orc.sam_pe_batch(oopt, orc.default_tail_opt(), pac, g2, flavour=bpsw_hip.TAIL_SCALA)
    want = [_single_end_of(t) for t in pair_text[0::2]]
    got, _ = ctx.sam_se_batch(opt, bpsw_hip.default_tail_opt(bpsw_hip.TAIL_SCALA), _se_of_group(g2, quals=False), flags=mode)
    assert got == want
    f = _lines(want)
    assert any(l[2].startswith(b"ctg") for l in f) and all(l[10] == b"*" for l in f)


# ---- 3. reads to text ---------------------------------------------------------------------------------------------------------------
def test_align_se_reads_to_text(ctx, ref, orc, gold, fixture_reads):
    g, idx, reads, quals, names = fixture_reads
    opt, so, topt = bpsw_hip.default_opt(), _opt(gold, "c1"), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    table = _contig_tables(g.size)[1]
    want, _, _ = _expected_c(ref, orc, gold, fixture_reads, table, 0)
    _load(ctx, gold["g1_pac"], g.size, table, idx)
    se = bpsw_hip.SeReadsSoA.from_lists(reads, names, quals, id0=1000, id_step=2)
    for w1 in (0, bpsw_hip.W1_CHAIN_DEVICE):
        for mode in TEXT_MODES:
            got = ctx.align_se_batch(opt, so, topt, se, zdrop_mode=bpsw_hip.ZDROP_BWA, w1_flags=w1, flags=mode)
            bad = [i for i in range(len(want)) if want[i] != got[i]]
            assert not bad, (w1, mode, len(bad), want[bad[0]], got[bad[0]])
    t = bpsw_hip.last_sam_se_times()
    assert t[4] > 0 and t[5] > 0 and t[0] > 0 and t[1] > 0
    # the refusals are bpsw_worker1_batch's: a read of 257 bases, no index
    long_read = bpsw_hip.SeReadsSoA.from_lists([g[:257]], [b"long"], [np.full(257, 70, np.uint8)])
    with pytest.raises(bpsw_hip.BpswError, match=r"\(-4\)"):
        ctx.align_se_batch(opt, so, topt, long_read)
    ctx.fmi_unload()
    with pytest.raises(bpsw_hip.BpswError, match=r"\(-1\)"):
        ctx.align_se_batch(opt, so, topt, se)
    ctx.fmi_load(idx)


# ---- 4., 5.: the library's own regions for the fixture's reads (no reference needed) ------------------------------------------------
@pytest.fixture(scope="module")
def own_regions(ctx, gold, fixture_reads):
    g, idx, reads, quals, names = fixture_reads
    _load(ctx, gold["g1_pac"], g.size, _contig_tables(g.size)[1], idx)
    cnt, regs = ctx.worker1_batch(bpsw_hip.default_opt(), _opt(gold, "c1"), fmi.ReadBatch.from_list(reads), zdrop_mode=bpsw_hip.ZDROP_BWA,
                                  flags=bpsw_hip.C2A_SORT_DEDUP)
    return cnt.copy(), regs.copy()


def _ready(ctx, gold, fixture_reads):
    g, idx = fixture_reads[0], fixture_reads[1]
    _load(ctx, gold["g1_pac"], g.size, _contig_tables(g.size)[1], idx)


@pytest.mark.parametrize("mode", TEXT_MODES)
def test_sam_se_text_capacity(ctx, gold, fixture_reads, own_regions, mode):
    _ready(ctx, gold, fixture_reads)
    opt, topt = bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    opt.flag = bpsw_hip.MEM_F_ALL
    se = _se(fixture_reads, *own_regions)
    want, _ = ctx.sam_se_batch(opt, topt, se, flags=0)
    full = b"".join(want)
    want_off = np.concatenate([[0], np.cumsum([len(t) for t in want])])
    st, keep, _ = bpsw_hip._se_struct(se, True)
    off = np.zeros(se.n_reads + 1, np.int64)
    need = C.c_size_t(0)
    for cap in (0, len(full) // 2, len(full) - 1):
        buf = np.full(cap + 64, 0xAB, np.uint8)
        off[:] = -1
        rc = ctx.lib.bpsw_sam_se_batch(ctx.h, C.byref(opt), C.byref(topt), C.byref(st), mode, bpsw_hip._ptr(buf), cap, bpsw_hip._ptr(off),
                                       C.byref(need), None)
        assert rc == -3 and need.value == len(full) and np.array_equal(off, want_off), (cap, rc, need.value)
        assert (buf[cap:] == 0xAB).all()                                  # the sentinel bytes behind the buffer
    buf = np.full(need.value + 1, 0xAB, np.uint8)
    rc = ctx.lib.bpsw_sam_se_batch(ctx.h, C.byref(opt), C.byref(topt), C.byref(st), mode, bpsw_hip._ptr(buf), need.value, bpsw_hip._ptr(off),
                                   C.byref(need), None)
    assert rc == 0 and buf[:-1].tobytes() == full and buf[-1] == 0xAB


def _both(ctx, opt, topt, se):
    host, regs_h = ctx.sam_se_batch(opt, topt, se, flags=0)
    dev, regs_d = ctx.sam_se_batch(opt, topt, se, flags=bpsw_hip.SAM_TEXT_DEVICE)
    bad = [i for i in range(len(host)) if host[i] != dev[i]]
    assert not bad, (len(bad), host[bad[0]], dev[bad[0]])
    assert regs_h.tobytes() == regs_d.tobytes()
    return host


def test_device_text_at_the_line_counts_around_a_wavefront(ctx, gold, fixture_reads, own_regions):
    """one line per lane, 64 lanes a block: batches of 1, 63, 64, 65 and 129 lines in all; no reads at all"""
    _ready(ctx, gold, fixture_reads)
    opt, topt = bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    per_read = [t.count(b"\n") for t in _both(ctx, opt, topt, _se(fixture_reads, *own_regions))]
    one, two = [i for i, n in enumerate(per_read) if n == 1], [i for i, n in enumerate(per_read) if n == 2]
    assert len(one) >= 65 and two
    for total in (1, 63, 64, 65, 129):
        which = (one * 2)[: total - 2] + two[:1] if total > 2 else one[:total]      # (a two-line read last: its SA list crosses nothing)
        text = _both(ctx, opt, topt, _se(fixture_reads, *own_regions, which=which))
        assert sum(t.count(b"\n") for t in text) == total
    empty = bpsw_hip.SeReadsSoA.from_lists([], [], [], reg_cnt=np.zeros(0, np.int32), regs=own_regions[1][:0])
    for mode in TEXT_MODES:
        assert ctx.sam_se_batch(opt, topt, empty, flags=mode)[0] == []


def test_device_text_of_the_read_with_a_hundred_lines(ctx, gold, fixture_reads, own_regions):
    _ready(ctx, gold, fixture_reads)
    opt, topt = bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    opt.flag = bpsw_hip.MEM_F_ALL
    per_read = [t.count(b"\n") for t in _both(ctx, opt, topt, _se(fixture_reads, *own_regions))]
    big = int(np.argmax(per_read))
    assert per_read[big] >= 101
    alone = _both(ctx, opt, topt, _se(fixture_reads, *own_regions, which=[big]))
    assert alone[0].count(b"\n") == per_read[big]
    last = _both(ctx, opt, topt, _se(fixture_reads, *own_regions, which=[0, 1, 2, big]))
    assert last[3].count(b"\n") == per_read[big]
    # id_step 0 and 1 on one batch: each equals the host path's; they differ at most where the hash order does
    t0 = _both(ctx, opt, topt, _se(fixture_reads, *own_regions, id0=77, id_step=0))
    t1 = _both(ctx, opt, topt, _se(fixture_reads, *own_regions, id0=77, id_step=1))
    assert [t.count(b"\n") for t in t0] == [t.count(b"\n") for t in t1] and t0[0] == t1[0]      # (read 0 has id 77 both ways)


def test_device_text_of_short_and_long_reads_and_names(ctx, gold, fixture_reads):
    """a one-base read without regions, a read of 256 bases, names of 1 and of 200 bytes"""
    _ready(ctx, gold, fixture_reads)
    g = fixture_reads[0]
    opt, so = bpsw_hip.default_opt(), _opt(gold, "c1")
    reads = [g[77:78], g[5000:5256], (3 - g[6000:6256][::-1]).astype(np.uint8), g[300:450]]
    cnt, regs = ctx.worker1_batch(opt, so, fmi.ReadBatch.from_list(reads), zdrop_mode=bpsw_hip.ZDROP_BWA, flags=bpsw_hip.C2A_SORT_DEDUP)
    assert cnt[0] == 0 and cnt[1:].sum() >= 1
    rng = np.random.default_rng(9)
    quals = [rng.integers(33, 127, len(r)).astype(np.uint8) for r in reads]
    names = [b"q", b"n" * 200, b"w" * 200, b"z"]
    for flavour in (bpsw_hip.TAIL_SCALA, bpsw_hip.TAIL_C):
        se = bpsw_hip.SeReadsSoA.from_lists(reads, names, quals, reg_cnt=cnt, regs=regs, id0=5, id_step=2)
        text = _both(ctx, opt, bpsw_hip.default_tail_opt(flavour), se)
        f = [_lines([t])[0] for t in text]                                     # every read's first line
        assert f[0][0] == b"q" and int(f[0][1]) == 4 and f[0][9] in (b"A", b"C", b"G", b"T") and len(f[0][10]) == 1
        assert len(f[1][0]) == 200 and len(f[1][9]) == 256 and len(f[2][10]) == 256 and f[3][0] == b"z"
