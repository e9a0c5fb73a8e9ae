"""BASELINE.json configs[3]-sized coordinate space: a reference of 3 100 000 019 bases (GRCh38-sized; 0.78 GB as 2-bit .pac,
resident in HBM), so that forward coordinates pass 2^31 and reverse-strand coordinates -- [l_pac, 2 l_pac) = [3.1e9, 6.2e9) --
pass 2^32 (util/BNTSeqUtil.scala:37-79, worker2/MemSamPe.scala:1834-1850 work in that doubled space with Long arithmetic).
Every device path that takes reference coordinates is compared with the oracle on reads placed beyond 2^31, beyond 2^32 and
at the ends of both strands: bpsw_ref_fetch (bnsGetSeq), the coordinate-mode group rescue and the device round loop.

Worker2's tail and the writers behind it run here on the same resident reference under two contig tables -- one whose first contig
has ann_len's maximum of 2^31 - 1 bases, one of 3 002 contigs -- on pairs pinned where their arithmetic turns (tests/tail_util.py:
big_group; the census of what the pins reach is asserted on the reference's own text in tests/test_tail_oracle.py): reg2aln_kernel,
the pairing and mapQ host code, sam_len_kernel / sam_write_kernel, bam_len_kernel / bam_write_kernel and bpsw_worker2_batch, each
against the oracle, byte for byte."""
import copy
import dataclasses

import numpy as np
import pytest

import bpsw_hip
from bpsw_hip import synth
import bam_plain as bp
import pyoracle as po
import tail_util as tu
from conftest import region_fields_equal
from test_bam_gpu import _check, _ref_id, payload
from test_reg2aln_edges_gpu import _resident_waves
from test_sam_se_gpu import _se_of_group, _single_end_of

pytestmark = pytest.mark.gpu
L_PAC = 3_100_000_019


@pytest.fixture(scope="module")
def big():
    pac = tu.big_pac()        # rng(20261101)'s bytes, with one stretch of 1 500 bases copied (tail_util.BIG_DUP) for reads of two loci
    assert tu.BIG_L_PAC == L_PAC
    ctx = bpsw_hip.Context(0)
    ctx.ref_load(pac, L_PAC)
    yield ctx, pac, synth.PacBases(pac, L_PAC)
    ctx.ref_unload()
    ctx.close()


def test_ref_fetch_beyond_2_31_and_at_the_strand_ends(big):
    ctx, pac, _ = big
    assert ctx.ref_length() == L_PAC
    orc = po.Oracle()
    rng = np.random.default_rng(7)
    edges = [0, 2 ** 31, 2 ** 32, L_PAC, 2 * L_PAC]
    beg, end = [], []
    for e in edges:                               # windows before, across and after every interesting coordinate
        for d in (-700, -300, -1, 0, 1, 250):
            b = e + d
            beg.append(b); end.append(b + int(rng.integers(1, 600)))
    for _ in range(200):                          # and anywhere in the doubled space, sometimes swapped (bnsGetSeq swaps)
        b = int(rng.integers(0, 2 * L_PAC - 700))
        e = b + int(rng.integers(1, 700))
        if rng.random() < 0.2:
            b, e = e, b
        beg.append(b); end.append(e)
    got, _ = ctx.ref_fetch(np.array(beg, np.int64), np.array(end, np.int64))
    n_beyond = 0
    for b, e, g in zip(beg, end, got):
        want = orc.bns_get_seq(L_PAC, pac, b, e)
        assert np.array_equal(g, want), (b, e)
        n_beyond += int(len(want) > 0 and max(b, e) > 2 ** 32)
    assert n_beyond > 20


def test_group_rescue_by_coordinates_beyond_2_31(big):
    ctx, pac, bases = big
    orc = po.Oracle()
    # forward starts: right behind the start of the strand, either side of 2^31, right before the end of the strand (whose
    # mates then sit at the START of the reverse strand, coordinates just above l_pac); the mates of the first ones sit at
    # the END of the doubled space, just below 2 l_pac = 6.2e9
    pos = [2000, 2100, 2 ** 31 - 700, 2 ** 31 - 100, 2 ** 31 + 5, L_PAC - 3100, L_PAC - 3001] * 6
    g = synth.rescue_group(240, seed=20261102, l_pac=L_PAC, p_resc=0.5, ref_bases=bases, positions=pos)
    assert int((g.regs["rb"] > 2 ** 32).sum()) > 50 and int(((g.regs["rb"] > 2 ** 31) & (g.regs["rb"] < L_PAC)).sum()) > 20
    for mode in (bpsw_hip.RESCUE_C, bpsw_hip.RESCUE_SCALA):
        want_cnt, want, n_sw, _ = orc.matesw_group(orc.default_opt(), g, mode)           # windows as bytes
        gc = dataclasses.replace(g, ref_pool=None, ref_len=None, ref_off=None)            # coordinates only
        got_cnt, got = ctx.matesw_group(bpsw_hip.default_opt(), gc, mode)
        assert np.array_equal(got_cnt, want_cnt)
        region_fields_equal(got, want)
        assert n_sw > 80 and got.shape[0] > g.regs.shape[0]                               # mates were rescued from the resident reference
    assert int((got["rb"] > 2 ** 32).sum()) > int((g.regs["rb"] > 2 ** 32).sum())       # ... also beyond 2^32


def test_round_loop_on_reads_beyond_2_31(big):
    ctx, pac, bases = big
    orc = po.Oracle()
    L = 150
    pos = [600, 2 ** 31 - 80, 2 ** 31 + 3, L_PAC - L - 661, L_PAC + 600, 2 ** 32 - 75, 2 ** 32 + 9, 2 * L_PAC - L - 661] * 5
    b = synth.read_chains(400, bases, L_PAC, read_len=L, sub_rate=0.02, indel_rate=0.004, seed=20261103, positions=pos)
    assert int((b.seed_rbeg > 2 ** 32).sum()) > 100
    for zmode in (po.ZDROP_SCALA, po.ZDROP_BWA):
        want_cnt, want, _, _ = orc.chain2aln_batch(orc.default_opt(), pac, b, zmode)
        got_cnt, got = ctx.chain2aln_batch(bpsw_hip.default_opt(), b, zdrop_mode=zmode)
        assert np.array_equal(got_cnt, want_cnt)
        region_fields_equal(got, want)
    assert int((got["rb"] > 2 ** 32).sum()) > 50


# ---- worker2's tail and the SAM / BAM writers ---------------------------------------------------------------------------------------------
FLAVOURS = [bpsw_hip.TAIL_SCALA, bpsw_hip.TAIL_C]
ALL, NO_MULTI = bpsw_hip.MEM_F_ALL, bpsw_hip.MEM_F_NO_MULTI
CASES = ((0, b""), (ALL, b"run12.lane3"), (ALL | NO_MULTI, b""), (0, b"g7"))     # the three flag sets, the read group on and off
DEV = bpsw_hip.SAM_TEXT_DEVICE
_orc_memo = {}


def _bns(ctx, table, with_names=True):
    _, _, off, ln, names = tu.big_reference(table)
    ctx.bns_load(off, ln, names if with_names else None)
    return off, ln, names


def _opts(orc, flavour, flag=0, rg=b""):
    opt, oopt, topt, otopt = bpsw_hip.default_opt(), orc.default_opt(), bpsw_hip.default_tail_opt(flavour), orc.default_tail_opt()
    opt.flag = oopt.flag = flag
    topt.rg_id = otopt.rg_id = rg
    return opt, oopt, topt, otopt


def _orc_reg2aln(orc, table, flavour):
    """the oracle's memRegToAln on the genome-scale jobs, once per (table, flavour)"""
    key = ("reg2aln", table, flavour)
    if key not in _orc_memo:
        _, _, off, ln, _ = tu.big_reference(table)
        rl, ro, pool, regs, _ = tu.big_reg2aln_jobs(orc, table)
        _orc_memo[key] = orc.reg2aln_batch(orc.default_opt(), orc.default_tail_opt(), tu.big_pac(), L_PAC, off, ln, rl, ro, pool, regs,
                                           flavour=flavour, cigar_cap=64, md_cap=512)
    return _orc_memo[key]


def _reg2aln_same(ctx, want, jobs, sel, flavour, what):
    """the jobs `sel` (indices, possibly repeated) through bpsw_reg2aln_batch: every field, the CIGAR words and the MD bytes a job has"""
    rl, ro, pool, regs, _ = jobs
    sel = np.asarray(sel)
    got = ctx.reg2aln_batch(bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(flavour), rl[sel], ro[sel], pool, regs[sel], max_cigar=64, max_md=512)
    a = want[0][sel]
    for f in a.dtype.names:
        bad = np.nonzero(a[f] != got[0][f])[0]
        assert bad.size == 0, (what, flavour, f, [(int(sel[i]), regs[sel[i]].tolist(), int(a[f][i]), int(got[0][f][i])) for i in bad[:4]])
    nc = np.where((a["status"] == bpsw_hip.ALN_XREF) | (a["n_cigar"] > 64), 0, a["n_cigar"])
    nm = np.where(a["status"] == bpsw_hip.ALN_XREF, 0, np.minimum(a["md_len"], 512))
    for k, n, rows_w, rows_g in ((64, nc, want[1][sel], got[1]), (512, nm, want[2][sel], got[2])):
        live = np.arange(k)[None, :] < n[:, None]                        # behind them the library leaves the zeros it was given
        bad = np.nonzero(((rows_w != rows_g) & live).any(axis=1) | ((rows_g != 0) & ~live).any(axis=1))[0]
        assert bad.size == 0, (what, flavour, k, [(int(sel[i]), regs[sel[i]].tolist()) for i in bad[:4]])
    return got


@pytest.mark.parametrize("flavour", FLAVOURS, ids=["scala", "c"])
@pytest.mark.parametrize("table", ["long", "many"])
def test_reg2aln_at_genome_scale(big, table, flavour):
    """reg2aln_kernel: rb / re rebuilt from two 32-bit halves, pos2rid over 4 and over 3 002 contigs, the contig-end cut and pac_base
    beyond 2^31 and 2^32, o.pos in a contig of 2^31 - 1 bases.  The jobs are counted in test_tail_oracle.py (915 / 1 178: every region
    of the pinned groups and the hand-built ones at 2^31 -+ 75, 2^32 -+ 75, l_pac and 2 l_pac); here also 1, 63, 64 and 65 of them and
    more than the launch has resident waves."""
    ctx, pac, _ = big
    orc = po.Oracle()
    _bns(ctx, table)
    jobs = tu.big_reg2aln_jobs(orc, table)
    want = _orc_reg2aln(orc, table, flavour)
    n = len(jobs[0])
    _reg2aln_same(ctx, want, jobs, np.arange(n), flavour, "all")
    regs, a = jobs[3], want[0]
    assert int((regs["rb"] > 2 ** 32).sum()) >= 190 and int(((regs["rb"] > 2 ** 31) & (regs["re"] <= L_PAC)).sum()) >= 20
    assert int((regs["re"] == 2 * L_PAC).sum()) >= 3 and int((regs["rb"] == L_PAC).sum()) >= 3 and int((a["status"] == bpsw_hip.ALN_XREF).sum()) >= 1
    assert int((a["pos"] >= 10 ** 9).sum()) >= 170                    # ... and, "long", positions at the end of a contig of 2^31 - 1 bases
    assert int(((a["rid"] == 0) & (a["pos"] + 160 >= 2 ** 31 - 1)).sum()) >= (40 if table == "long" else 0)
    assert n - jobs[4] >= 65                                          # the hand-built jobs are the last ones
    for k in (1, 63, 64, 65):
        _reg2aln_same(ctx, want, jobs, np.arange(n - k, n), flavour, k)
    resident = _resident_waves(ctx.num_cu(), int(jobs[0].max()), int((regs["re"] - regs["rb"]).max()))
    many = resident + 129
    assert many > n                                                   # (else the run over all of them was that case already)
    _reg2aln_same(ctx, want, jobs, (np.arange(many) * 7 + 3) % n, flavour, "more than resident")


def _names_pool(names):
    off = np.zeros(len(names) + 1, np.int64)
    bs = [s.encode() for s in names]
    off[1:] = np.cumsum([len(b) for b in bs])
    return off, np.frombuffer(b"".join(bs) + b"\0", np.uint8).copy()


def _end0_only(g):
    """the group with every second end's regions dropped: what the single-end derivation of test_sam_se_gpu.py starts from"""
    return tu.without_regions_of(g, range(1, 2 * g.group_size, 2))


def _first_diff(want, got):
    bad = [i for i in range(len(want)) if want[i] != got[i]]
    return (len(bad), want[bad[0]], got[bad[0]]) if bad else None


def _sam_cases(ctx, orc, pac, table, flavour):
    """every case of the text tests: the contig table loaded with and without names, the three flag sets, the read group on and off
    -> (group, its end-0-only twin, opt, topt, the oracle's text and regions for either), the contig table being loaded for the case"""
    g = tu.big_group(orc, table, 150)[2]
    for with_names in (True, False):
        off, ln, names = _bns(ctx, table, with_names)
        gn = copy.copy(g)
        if not with_names:
            gn.ann_name_off, gn.ann_name_pool = _names_pool(["ctg%d" % (k + 1) for k in range(len(ln))])
        g1 = _end0_only(gn)
        for flag, rg in CASES:
            opt, oopt, topt, otopt = _opts(orc, flavour, flag, rg)
            key = ("sam", table, flavour, with_names, flag, rg)
            if key not in _orc_memo:
                want, want_regs, _ = orc.sam_pe_batch(oopt, otopt, pac, gn, flavour=flavour)
                pair1, want_regs1, _ = orc.sam_pe_batch(oopt, otopt, pac, g1, flavour=flavour)
                assert all((b"\tRG:Z:" + rg in w) == bool(rg) for w in want)
                if flag == ALL:                                        # (the minimums of test_tail_oracle.py's census, C flavour or not)
                    tiny = (b"tiny20" if table == "long" else b"s1500") if with_names else b"ctg%d" % (2 if table == "long" else 1501)
                    c = tu.big_census(want, gn, tiny)
                    assert c["pos10"] >= 69 and c["pnext10"] >= 71 and c["sa_pos10"] >= 8 and c["secondary"] >= 13 and c["tiny"] >= 3, c
                    assert c["tlen_2e9"] >= (10 if table == "long" else 0) and c["contigs"] >= (4 if table == "long" else 487), c
                    assert table == "long" or sum(b"\tctg2001\t" in w for w in want) >= 4
                _orc_memo[key] = (want, want_regs, [_single_end_of(t) for t in pair1[0::2]], want_regs1)
            yield (table, with_names, flag, rg), gn, g1, opt, topt, _orc_memo[key]


@pytest.mark.parametrize("flavour", FLAVOURS, ids=["scala", "c"])
@pytest.mark.parametrize("table", ["long", "many"])
def test_sam_pe_host_text_at_genome_scale(big, table, flavour):
    """bpsw_sam_pe_batch with the text written by the calling thread: the pairing and mapQ host code and bwa_fix_xref2's host twin on
    coordinates up to 6.2e9, ten-digit POS / PNEXT / SA:Z positions, TLEN of -+2.1e9, 3 002 contig names (one of them empty: ctg2001)
    and no names at all.  Byte for byte against the oracle, out_regs included; what the text holds is counted in test_tail_oracle.py."""
    ctx, pac, _ = big
    orc = po.Oracle()
    for case, gn, _, opt, topt, (want, want_regs, _, _) in _sam_cases(ctx, orc, pac, table, flavour):
        got, got_regs = ctx.sam_pe_batch(opt, topt, gn)
        assert _first_diff(want, got) is None, (case, _first_diff(want, got))
        assert got_regs.tobytes() == want_regs.tobytes()


# The tests below carry `device_resident` in their names: tests/test_host_sanitizers.py plays this file on a fake device that has no
# text, BAM or header entry (they live beside their kernels), and leaves out by that word what it cannot play.
@pytest.mark.parametrize("flavour", FLAVOURS, ids=["scala", "c"])
@pytest.mark.parametrize("table", ["long", "many"])
def test_sam_text_of_the_device_resident_writers_at_genome_scale(big, table, flavour):
    """The same cases with the text written by sam_len_kernel / sam_write_kernel (csrc/bpsw_sam_core.h on the device: put_num, put_contig
    and ctg_at over thousands of names), for pairs and -- by test_sam_se_gpu.py's derivation -- for single ends, whose host text is
    compared too."""
    ctx, pac, _ = big
    orc = po.Oracle()
    for case, gn, g1, opt, topt, (want, want_regs, want1, want_regs1) in _sam_cases(ctx, orc, pac, table, flavour):
        got, got_regs = ctx.sam_pe_batch(opt, topt, gn, flags=DEV)
        assert _first_diff(want, got) is None, (case, _first_diff(want, got))
        assert got_regs.tobytes() == want_regs.tobytes()
        for mode in (0, DEV):
            got1, got_regs1 = ctx.sam_se_batch(opt, topt, _se_of_group(g1), flags=mode)
            assert _first_diff(want1, got1) is None, (case, mode, _first_diff(want1, got1))
            assert got_regs1.tobytes() == want_regs1.tobytes()
        assert sum(t.count(b"\n") for t in want1) > len(want1)       # (supplementary or secondary lines among the single ends)


@pytest.mark.parametrize("rescue_mode,flavour", [(bpsw_hip.RESCUE_C, bpsw_hip.TAIL_C), (bpsw_hip.RESCUE_SCALA, bpsw_hip.TAIL_SCALA)], ids=["c", "scala"])
def test_worker2_at_genome_scale(big, rescue_mode, flavour):
    """bpsw_worker2_batch on the "long" table's pairs with every third read's regions taken away: the rescue cuts its windows from the
    resident reference at coordinates up to 6.2e9 and finds them again; against the oracle's pipeline with windows cut as bytes."""
    ctx, pac, bases = big
    orc = po.Oracle()
    _bns(ctx, "long")
    g0 = tu.big_group(orc, "long", 150)[2]
    g = tu.without_regions_of(g0, range(1, 2 * g0.group_size, 3))
    opt, oopt, topt, otopt = _opts(orc, flavour)
    cnt_o, regs_o, n_sw, _ = orc.matesw_group(oopt, tu.rescue_group_of(g, bases, oopt), rescue_mode)
    assert n_sw >= 150 and regs_o.shape[0] >= g.regs.shape[0] + 90
    assert int((regs_o["rb"] > 2 ** 32).sum()) >= int((g.regs["rb"] > 2 ** 32).sum()) + 20        # the rescue added regions beyond 2^32
    g2 = copy.copy(g)
    g2.reg_cnt, g2.regs = cnt_o, regs_o
    want, want_regs, _ = orc.sam_pe_batch(oopt, otopt, pac, g2, flavour=flavour)
    got, cnt, regs = ctx.worker2_batch(opt, topt, g, rescue_mode)
    assert np.array_equal(cnt, cnt_o)
    assert _first_diff(want, got) is None, _first_diff(want, got)
    assert regs.tobytes() == want_regs.tobytes()
    assert int((regs["rb"] > 2 ** 32).sum()) >= int((g.regs["rb"] > 2 ** 32).sum()) + 20


@pytest.mark.parametrize("table,read_len", [("long", 150), ("many", 150), ("long", 300)])
def test_bam_of_the_device_resident_writers_at_genome_scale(big, table, read_len):
    """bpsw_bam_pe_batch / bpsw_bam_se_batch (bam_len_kernel, bam_write_kernel over csrc/bpsw_bam_core.h): reg2bin on every level, bins
    beyond the 16-bit field, pos / next_pos / tlen near 2^31 and, with reads of 300 bases, integer tags of two bytes -- against
    bam_plain.sam_to_bam of the twin text (itself compared with the oracle above), with the member framing, CRC and closed-form size
    of test_bam_gpu.py's _check, at the default payload and at 256 bytes."""
    ctx, pac, _ = big
    orc = po.Oracle()
    off, ln, names = _bns(ctx, table)
    ids = _ref_id(names)
    g = tu.big_group(orc, table, read_len)[2]
    g1 = _end0_only(g)
    levels, over, tag_s = [0] * 6, 0, 0
    for flavour, flag, rg, p in ((bpsw_hip.TAIL_C, 0, b"", 0), (bpsw_hip.TAIL_SCALA, ALL, b"run12.lane3", 256)):
        opt, oopt, topt, otopt = _opts(orc, flavour, flag, rg)
        text, regs_t = ctx.sam_pe_batch(opt, topt, g, flags=DEV)
        want, _, _ = orc.sam_pe_batch(oopt, otopt, pac, g, flavour=flavour)
        assert _first_diff(want, text) is None, _first_diff(want, text)
        text1, regs_t1 = ctx.sam_se_batch(opt, topt, _se_of_group(g1), flags=DEV)
        with payload(p) as size:
            bam, regs_b = ctx.bam_pe_batch(opt, topt, g)
            bam1, regs_b1 = ctx.bam_se_batch(opt, topt, _se_of_group(g1))
        assert regs_t.tobytes() == regs_b.tobytes() and regs_t1.tobytes() == regs_b1.tobytes()
        _check(bam, text, ids, size)
        _check(bam1, text1, ids, size)
        c = tu.big_census(text, g)
        levels = [a + b for a, b in zip(levels, c["levels"])]
        over += c["bin_over_16_bits"]; tag_s += c["tag_S"]
        assert c["tlen_2e9"] >= (10 if table == "long" else 0) and c["pos10"] >= 60 and c["pnext10"] >= 60, c
    assert all(n >= 4 for n in levels) and over >= 140 and (tag_s >= 298 or read_len < 256), (levels, over, tag_s)


def test_device_resident_contig_table_as_headers_of_three_thousand_contigs(big):
    ctx, _, _ = big
    off, ln, names = _bns(ctx, "many")
    extra = b"@PG\tID:bpsw\n"
    text = bp.sam_header_text(names, ln, extra)
    assert ctx.sam_header(extra) == text and b"@SQ\tSN:ctg2001\tLN:" in text and text.count(b"@SQ") == 3002
    with payload(4096):
        data = ctx.bam_header(extra)
    stream = bp.bgzf_inflate(data)
    assert len(bp.bgzf_members(data)) == -(-len(stream) // 4096) > 10
    assert bp.parse_bam_header(stream) == (text, [(n.encode(), int(l)) for n, l in zip(tu.printed_names(names), ln)], len(stream))
    _bns(ctx, "many", with_names=False)
    assert ctx.sam_header() == bp.sam_header_text([""] * 3002, ln)
