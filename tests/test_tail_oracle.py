"""Pins the oracle's restatement of worker2's tail (oracle/bpsw_oracle_tail.c) on the reference: committed golden vectors made
by the reference's own mem_sam_pe / mem_reg2aln (tests/golden/make_golden.py) and, where oracle/_ref exists, live runs of
mem_mark_primary_se / mem_pair / mem_approx_mapq_se / mem_reg2aln / mem_sam_pe on larger seeded samples.  CPU only."""
import os

import numpy as np
import pytest

import pyoracle as po
import tail_util as tu
from tail_util import G, load_sam_pe_golden, synthetic_group


@pytest.mark.parametrize("stem", ["mem_sam_pe", "mem_sam_pe_all", "mem_sam_pe_rg"])
def test_sam_pe_vs_golden_text(orc, stem):
    pac, g, flag, want = load_sam_pe_golden(stem)
    opt, topt = orc.default_opt(), orc.default_tail_opt()
    opt.flag = flag
    topt.rg_id = g.rg_id                    # "mem_sam_pe_rg": the reference ran with a read group (bwa_rg_id): RG:Z on every line
    assert all((b"\tRG:Z:" + g.rg_id in w) if g.rg_id else (b"\tRG:Z:" not in w) for w in want)
    got, _, n_jobs = orc.sam_pe_batch(opt, topt, pac, g, flavour=po.TAIL_C)
    assert got == want                      # byte for byte, every field of every SAM line
    assert n_jobs >= g.group_size           # memRegToAln ran for (almost) every read
    kinds = {int(w.split(b"\t")[1]) & 0x2 for w in want}
    assert kinds == {0, 2}                  # both properly paired and unpaired outcomes are present
    assert any(b"I" in w.split(b"\t")[5] or b"D" in w.split(b"\t")[5] for w in want)   # gapped CIGARs (the DP path)
    if stem != "mem_sam_pe_rg":             # (the smaller fixture need not hold every kind)
        assert any(w.split(b"\t")[1] in (b"77", b"141", b"69", b"133", b"73", b"137", b"89", b"153") for w in want)  # unmapped ends


def test_reg2aln_vs_golden(orc):
    z = np.load(os.path.join(G, "mem_reg2aln.npz"))
    opt, topt = orc.default_opt(), orc.default_tail_opt()
    regs = z["regs"].astype(po.ALNREG_DTYPE)
    alns, cig, md = orc.reg2aln_batch(opt, topt, z["pac"], int(z["l_pac"]), z["ann_off"], z["ann_len"], z["read_len"], z["read_off"],
                                      z["read_pool"], regs, flavour=po.TAIL_C, cigar_cap=32, md_cap=160)
    want = z["alns"]
    assert int((alns["status"] != 0).sum()) == 0
    for f in ("pos", "rid", "flag", "is_rev", "mapq", "NM", "n_cigar", "score", "sub", "md_len"):
        assert np.array_equal(alns[f], want[f]), f
    assert np.array_equal(cig, z["cigar"]) and np.array_equal(md, z["md"])
    assert int((want["rid"] < 0).sum()) == 1 and int((want["flag"] & 0x100 != 0).sum()) > 0
    # the fixture reaches bwaFixXref2's repair: some region was cut at a contig boundary, so its CIGAR carries a clip that the
    # region's own qb/qe do not explain
    explained = (regs["qb"][:-1] != 0) | (regs["qe"][:-1] != z["read_len"][:-1])
    has_clip = np.array([any((int(c) & 0xf) == 3 for c in cig[j, :want["n_cigar"][j]]) for j in range(len(want) - 1)])
    assert int((has_clip & ~explained).sum()) > 0


def test_scala_flavour_differences_are_the_documented_ones(orc):
    """T1..T4: the Scala text and the C agree except where the transcription changed the arithmetic."""
    opt, topt = orc.default_opt(), orc.default_tail_opt()
    # T2: mapQ at l == mapQCoefLen
    r = np.zeros(1, po.ALNREG_DTYPE)[0]
    r["qb"], r["qe"], r["rb"], r["re"], r["score"], r["seedcov"] = 0, 50, 1000, 1050, 30, 25
    assert orc.approx_mapq(opt, topt, r, po.TAIL_C) != orc.approx_mapq(opt, topt, r, po.TAIL_SCALA)
    r["qe"], r["re"] = 51, 1051
    assert orc.approx_mapq(opt, topt, r, po.TAIL_C) == orc.approx_mapq(opt, topt, r, po.TAIL_SCALA)
    # T4: the parent index of a secondary hit (three overlapping hits and one disjoint primary)
    regs = np.zeros(4, po.ALNREG_DTYPE)
    for i, (qb, qe, sc) in enumerate(((0, 100, 90), (0, 100, 85), (110, 150, 75), (5, 95, 70))):
        regs[i]["qb"], regs[i]["qe"], regs[i]["rb"], regs[i]["re"], regs[i]["score"] = qb, qe, 5000 * (i + 1), 5000 * (i + 1) + qe - qb, sc
    c = orc.mark_primary(opt, topt, regs, 10, po.TAIL_C)
    s = orc.mark_primary(opt, topt, regs, 10, po.TAIL_SCALA)
    assert list(c["score"]) == [90, 85, 75, 70] and list(c["secondary"]) == [-1, 0, -1, 0]
    assert list(s["secondary"]) == [-1, 0, -1, 2]    # z(k) read after k was stepped (MemMarkPrimarySe.scala:93-101)
    assert list(c["sub"]) == list(s["sub"]) == [85, 0, 0, 0] and list(c["sub_n"]) == [1, 0, 0, 0]


# ---- genome-scale coordinates (tests/tail_util.py: big_group, big_census) -------------------------------------------------------------------
ALL, NO_MULTI = po.MEM_F_ALL, po.MEM_F_NO_MULTI


def _big_vs_reference(orc, ref, table, read_len, cases, tiny):
    """the oracle's text equals the reference's byte for byte under every (flag, read group) of `cases` -> the census of each"""
    pac, _, g = tu.big_group(orc, table, read_len)
    out = []
    for flag, rg in cases:
        o, topt = orc.default_opt(), orc.default_tail_opt()
        o.flag, topt.rg_id = flag, rg
        want = ref.sam_pe_batch(o, topt, pac, g)
        c = tu.big_census(want, g, tiny)           # on the reference's text alone, before it is compared with anything
        print(table, read_len, flag, rg, c)
        out.append(c)
        got, _, _ = orc.sam_pe_batch(o, topt, pac, g, flavour=po.TAIL_C)
        bad = [i for i in range(len(want)) if want[i] != got[i]]
        assert not bad, (table, flag, rg, len(bad), want[bad[0]], got[bad[0]])
        assert all((b"\tRG:Z:" + rg in w) if rg else (b"\tRG:Z:" not in w) for w in want)
    return g, out


BIG_CASES = ((0, b""), (ALL, b""), (ALL | NO_MULTI, b""), (0, b"run12.lane3"))


def test_genome_scale_long_table_vs_reference(orc, ref):
    """168 pairs of 2 x 150 bp on 3 100 000 019 bases under the contig table [2^31 - 1, 20, 1, the rest].  Census of the reference's
    text, as minimums (measured on the reference alone).  Flag 0: 346 lines, of them on reg2bin's levels 303 / 4 / 4 / 4 / 2 / 12,
    112 with a bin beyond 16 bits, 110 with a ten-digit POS, 117 with a ten-digit PNEXT, 20 SA:Z tags of which 18 hold a ten-digit
    position, 10 with |TLEN| > 2e9, 42 cut at a contig end, 12 on the 20-base contig, 10 hard-clipped supplementary lines, 81 with the
    mate on another contig, 167 on the reverse strand, 17 unmapped.  MEM_F_ALL: 362 lines, 16 secondary ones; with MEM_F_NO_MULTI 26
    and no hard clip."""
    g, (c0, c_all, c_nm, c_rg) = _big_vs_reference(orc, ref, "long", 150, BIG_CASES, b"tiny20")
    assert g.group_size == 168 and int(g.ann_len[0]) == 2 ** 31 - 1 and list(g.ann_len[1:3]) == [20, 1]
    assert int((g.regs["rb"] > 2 ** 32).sum()) >= 90 and int(((g.regs["rb"] > 2 ** 31) & (g.regs["rb"] < g.l_pac)).sum()) >= 20
    assert c0["lines"] >= 346 and all(n >= m for n, m in zip(c0["levels"], (303, 4, 4, 4, 2, 12))), c0
    assert c0["bin_over_16_bits"] >= 112 and c0["pos10"] >= 110 and c0["pnext10"] >= 117 and c0["sa"] >= 20 and c0["sa_pos10"] >= 18, c0
    assert c0["tlen_2e9"] >= 10 and c0["contig_end_cut"] >= 42 and c0["tiny"] >= 12 and c0["supp_hard"] >= 10, c0
    assert c0["other_contig_mate"] >= 81 and c0["reverse"] >= 167 and c0["unmapped"] >= 17 and c0["contigs"] == 4, c0
    assert c_all["lines"] >= 362 and c_all["secondary"] >= 16 and c_nm["secondary"] >= 26 and c_nm["supp_hard"] == 0, (c_all, c_nm)
    assert c_rg["lines"] == c0["lines"]


def test_genome_scale_many_contigs_vs_reference(orc, ref):
    """469 pairs of 2 x 150 bp under a table of 3 002 contigs (3 000 of 150-5 000 bases, a 20-base and a 1-base one among them,
    between two large ones; names of seven different lengths, one printed as ctg2001).  Census of the reference's text, as
    minimums.  Flag 0: 948 lines on 487 distinct contigs, 4 and more on every reg2bin level, 71 bins beyond 16 bits, 69 ten-digit POS,
    71 ten-digit PNEXT, 20 SA:Z tags (8 with a ten-digit position), 98 lines cut at a contig end, 3 on the 20-base contig, 269 with
    the mate on another contig, 10 hard-clipped supplementary lines; MEM_F_ALL: 13 secondary lines, with MEM_F_NO_MULTI 23."""
    g, (c0, c_all, c_nm, c_rg) = _big_vs_reference(orc, ref, "many", 150, BIG_CASES, b"s1500")
    assert g.ann_len.shape[0] == 3002 and list(g.ann_len[1500:1502]) == [20, 1]
    names = [bytes(g.ann_name_pool[int(g.ann_name_off[i]):int(g.ann_name_off[i + 1])]) for i in range(3002)]
    assert names[1500] == b"s1500" and names[2000] == b"ctg2001" and len({len(n) for n in names}) >= 7
    assert c0["lines"] >= 948 and c0["contigs"] >= 487 and all(n >= 4 for n in c0["levels"]) and c0["bin_over_16_bits"] >= 71, c0
    assert c0["sa"] >= 20 and c0["sa_pos10"] >= 8 and c0["contig_end_cut"] >= 98 and c0["other_contig_mate"] >= 269 and c0["supp_hard"] >= 10, c0
    assert c0["pos10"] >= 69 and c0["pnext10"] >= 71 and c0["tiny"] >= 3, c0
    assert c_all["secondary"] >= 13 and c_nm["secondary"] >= 23 and c_rg["lines"] == c0["lines"], (c_all, c_nm)


def test_genome_scale_300bp_reads_vs_reference(orc, ref):
    """No tag of a 150-base read passes 255, so BAM's two-byte integer tag needs longer reads: the "long" table's pins as 2 x 300 bp.
    Census (minimums): 298 integer tags of 256 and more (AS, XS), 346 lines, 12 with |TLEN| > 2e9, 20 SA:Z tags."""
    g, (c0, c_all) = _big_vs_reference(orc, ref, "long", 300, ((0, b""), (ALL, b"g7")), b"tiny20")
    assert c0["tag_S"] >= 298 and c0["lines"] >= 346 and c0["tlen_2e9"] >= 12 and c0["sa"] >= 20 and c_all["secondary"] >= 13, (c0, c_all)


def _reg2aln_vs_reference(orc, ref, table):
    pac = tu.big_pac()
    _, _, off, ln, _ = tu.big_reference(table)
    rl, ro, pool, regs, n_group = tu.big_reg2aln_jobs(orc, table)
    opt, topt = orc.default_opt(), orc.default_tail_opt()
    got = orc.reg2aln_batch(opt, topt, pac, tu.BIG_L_PAC, off, ln, rl, ro, pool, regs, flavour=po.TAIL_C, cigar_cap=64, md_cap=512)
    ok = np.nonzero(got[0]["status"] == 0)[0]   # (the reference's mem_reg2aln EXITS where the oracle reports BPSW_ALN_XREF: bwamem.c:968-971)
    want = ref.reg2aln_batch(opt, topt, pac, tu.BIG_L_PAC, off, ln, rl[ok], ro[ok], pool, regs[ok], cigar_cap=64, md_cap=512)
    return want, got, ok, regs


def _genome_scale_reg2aln(orc, ref, table):
    want, got, ok, regs = _reg2aln_vs_reference(orc, ref, table)
    for f in ("pos", "rid", "flag", "is_rev", "mapq", "NM", "n_cigar", "score", "sub", "md_len"):
        assert np.array_equal(got[0][f][ok], want[0][f]), (table, f)
    for k, j in enumerate(ok):
        n, m = int(want[0]["n_cigar"][k]), int(want[0]["md_len"][k])
        assert np.array_equal(got[1][j][:n], want[1][k][:n]) and np.array_equal(got[2][j][:m], want[2][k][:m]), (table, j)
    a = got[0]
    refused = int((a["status"] != 0).sum())
    cut = int(((a["status"] == 0) & (a["rid"] >= 0) & (regs["qb"] == 0) & (regs["qe"] == tu.big_reg2aln_jobs(orc, table)[0])
               & np.array([any((int(c) & 0xf) in (3, 4) for c in got[1][j][:a["n_cigar"][j]]) for j in range(len(a))])).sum())
    print(table, "reg2aln jobs:", len(a), "refused:", refused, "cut at a contig end:", cut, "beyond 2^32:", int((regs["rb"] > 2 ** 32).sum()),
          "ten-digit pos:", int((a["pos"] >= 10 ** 9).sum()))
    return len(a), refused, cut, int((regs["rb"] > 2 ** 32).sum()), int((a["pos"] >= 10 ** 9).sum())


def test_genome_scale_reg2aln_long_table_vs_reference(orc, ref):
    """memRegToAln on every region of the 2 x 150 and the 2 x 250 group and on the hand-built regions at 2^31, 2^32, l_pac and 2 l_pac
    (tests/tail_util.py: big_hand_jobs), field by field, CIGAR words and MD bytes.  Measured (asserted as minimums): 915 jobs, 1
    refused (the bridge over l_pac), 157 cut at a contig end, 196 regions beginning beyond 2^32, 340 positions of ten digits."""
    n, refused, cut, beyond, pos10 = _genome_scale_reg2aln(orc, ref, "long")
    assert n >= 915 and refused >= 1 and cut >= 157 and beyond >= 196 and pos10 >= 340


def test_genome_scale_reg2aln_many_contigs_vs_reference(orc, ref):
    """... and under the table of 3 002 contigs (2 x 150 bp and the hand-built regions).  Measured: 1 178 jobs, 1 refused, 132 cut at
    a contig end, 508 regions beginning beyond 2^32, 177 positions of ten digits."""
    n, refused, cut, beyond, pos10 = _genome_scale_reg2aln(orc, ref, "many")
    assert n >= 1178 and refused >= 1 and cut >= 132 and beyond >= 508 and pos10 >= 177


def test_tail_vs_reference_live(orc, ref):
    opt, topt = orc.default_opt(), orc.default_tail_opt()
    total = 0
    for k, (es, ei, flag) in enumerate(((0.01, 0.002, 0), (0.04, 0.015, 0), (0.02, 0.005, po.MEM_F_ALL),
                                        (0.03, 0.01, po.MEM_F_NO_MULTI | po.MEM_F_ALL), (0.01, 0.002, po.MEM_F_NOPAIRING))):
        pac, g = synthetic_group(orc, 300, 900 + 10 * k, zdrop_mode=po.ZDROP_BWA, sub_rate=es, indel_rate=ei, p_span=0.06)
        o = orc.default_opt()
        o.flag = flag
        want = ref.sam_pe_batch(o, topt, pac, g)
        got, _, _ = orc.sam_pe_batch(o, topt, pac, g, flavour=po.TAIL_C)
        assert got == want
        total += len(want)
        # the pieces, one by one
        at = 0
        for r in range(2 * g.group_size):
            c = int(g.reg_cnt[r])
            if c:
                a = orc.mark_primary(opt, topt, g.regs[at:at + c], 2 * (g.id0 + r // 2) | (r & 1), po.TAIL_C)
                b = ref.mark_primary(opt, topt, g.regs[at:at + c], 2 * (g.id0 + r // 2) | (r & 1))
                assert a.tobytes() == b.tobytes()
                for reg in a[:2]:
                    assert orc.approx_mapq(opt, topt, reg, po.TAIL_C) == ref.approx_mapq(opt, topt, reg)
            at += c
        at = 0
        for p in range(g.group_size):
            c0, c1 = int(g.reg_cnt[2 * p]), int(g.reg_cnt[2 * p + 1])
            if c0 and c1:
                a0, a1 = g.regs[at:at + c0], g.regs[at + c0:at + c0 + c1]
                assert orc.mem_pair(opt, g.l_pac, g.pes, a0, a1, g.id0 + p, po.TAIL_C) == ref.mem_pair(opt, g.l_pac, g.pes, a0, a1, g.id0 + p)
            at += c0 + c1
    assert total == 3000
