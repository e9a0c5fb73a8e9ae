"""Helpers shared by the worker2-tail tests: golden-file loaders and the synthetic pipeline reads -> regions -> group."""
import os

import numpy as np

import bpsw_hip
import pyoracle as po
from bpsw_hip import synth

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_sam_pe_golden(stem):
    z = np.load(os.path.join(G, stem + ".npz"))
    pes = [(int(r[0]), int(r[1]), int(r[2]), float(r[3]), float(r[4])) for r in z["pes"]]
    g = bpsw_hip.TailGroupSoA(group_size=int(z["read_len"].shape[0]) // 2, l_pac=int(z["l_pac"]), id0=int(z["id0"]), pes=pes,
                              read_len=z["read_len"], read_off=z["read_off"], read_pool=z["read_pool"], qual_pool=z["qual_pool"],
                              name_off=z["name_off"], name_pool=z["name_pool"], reg_cnt=z["reg_cnt"],
                              regs=z["regs"].astype(po.ALNREG_DTYPE), ann_off=z["ann_off"], ann_len=z["ann_len"],
                              ann_name_off=z["ann_name_off"], ann_name_pool=z["ann_name_pool"])
    text, off = z["text"].tobytes(), z["text_off"]
    want = [text[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
    g.rg_id = z["rg_id"].tobytes() if "rg_id" in z.files else b""   # the -R read-group ID the reference ran with
    return z["pac"], g, int(z["flag"]), want


def synthetic_group(orc, n_pairs, seed, contigs=(70_000, 50_000, 30_000, 50_000), zdrop_mode=po.ZDROP_SCALA, dedup_mode=po.RESCUE_C,
                    id0=77, **kw):
    """pairs -> chains -> regions (the ORACLE's memChainToAln + memSortAndDedup) -> TailGroupSoA; returns (pac, group)"""
    pac, bases, off, ln, names, dups = synth.contig_reference(list(contigs), seed=seed)
    tb, rn, quals, pes = synth.tail_pairs(n_pairs, bases, off, ln, dups, seed=seed + 1, **kw)
    cnt, regs, _, _ = orc.chain2aln_batch(orc.default_opt(), pac, tb, zdrop_mode)
    out_cnt, out, at = [], [], 0
    for c in cnt:
        r = orc.sort_dedup(regs[at:at + c], mode=dedup_mode) if c else regs[0:0]
        at += c
        out_cnt.append(len(r)); out.append(r)
    g = bpsw_hip.make_tail_group(tb, rn, quals, pes, np.array(out_cnt, np.int32), np.concatenate(out), off, ln, names, id0=id0)
    return pac, g


def rescue_group_of(g, bases, opt):
    """The arguments of mateSWJNI for a TailGroupSoA whose regs are the lists BEFORE the rescue: the test-side mirror of
    memSamPeGroupJNIPrepare (MemSamPe.scala:1895-2000) with getAlnRegRefJNI's windows (:1810-1878) cut as bytes."""
    l_pac = g.l_pac
    ref_cnt, rb_l, re_l, len_l, off_l, chunks = [], [], [], [], [], []
    at, pool_at = 0, 0
    for e in range(2 * g.group_size):
        n = int(g.reg_cnt[e])
        a = g.regs[at:at + n]
        mate_len = int(g.read_len[e ^ 1])
        cnt = 0
        for j in range(n):
            if cnt >= opt.max_matesw:
                break
            if not (a[j]["score"] >= a[0]["score"] - opt.pen_unpaired):
                continue
            for r in range(4):
                lo, hi, failed = g.pes[r][0], g.pes[r][1], g.pes[r][2]
                if failed:
                    rb_l.append(-1); re_l.append(-1); len_l.append(0); off_l.append(0)
                    continue
                is_rev, is_larger = (r >> 1) != (r & 1), (r >> 1) == 0
                arb = int(a[j]["rb"])
                if not is_rev:
                    rb = arb + lo if is_larger else arb - hi
                    re = (arb + hi if is_larger else arb - lo) + mate_len
                else:
                    rb = (arb + lo if is_larger else arb - hi) - mate_len
                    re = arb + hi if is_larger else arb - lo
                rb, re = max(rb, 0), min(re, 2 * l_pac)
                w = synth.window_bases(bases, l_pac, rb, re)
                rb_l.append(rb); re_l.append(re); len_l.append(len(w)); off_l.append(pool_at)
                chunks.append(w)
                pad = (-len(w)) % 16
                if pad:
                    chunks.append(np.zeros(pad, np.uint8))
                pool_at += len(w) + pad
            cnt += 1
        ref_cnt.append(cnt)
        at += n
    i64 = lambda v: np.array(v, np.int64)
    return bpsw_hip.RescueGroupSoA(group_size=g.group_size, l_pac=l_pac, pes=g.pes, seq_len=np.ascontiguousarray(g.read_len),
                                   seq_off=np.ascontiguousarray(g.read_off), seq_pool=np.ascontiguousarray(g.read_pool),
                                   reg_cnt=np.ascontiguousarray(g.reg_cnt), regs=np.ascontiguousarray(g.regs),
                                   ref_cnt=np.array(ref_cnt, np.int32), ref_rb=i64(rb_l), ref_re=i64(re_l), ref_len=i64(len_l),
                                   ref_off=i64(off_l), ref_pool=np.concatenate(chunks) if chunks else np.zeros(16, np.uint8))


def synthetic_group_with_bases(orc, n_pairs, seed, contigs=(70_000, 50_000, 30_000, 50_000), zdrop_mode=po.ZDROP_SCALA,
                               dedup_mode=po.RESCUE_C, id0=77, **kw):
    """like synthetic_group, also returning the unpacked reference (for cutting rescue windows)"""
    pac, bases, off, ln, names, dups = synth.contig_reference(list(contigs), seed=seed)
    tb, rn, quals, pes = synth.tail_pairs(n_pairs, bases, off, ln, dups, seed=seed + 1, **kw)
    cnt, regs, _, _ = orc.chain2aln_batch(orc.default_opt(), pac, tb, zdrop_mode)
    out_cnt, out, at = [], [], 0
    for c in cnt:
        r = orc.sort_dedup(regs[at:at + c], mode=dedup_mode) if c else regs[0:0]
        at += c
        out_cnt.append(len(r)); out.append(r)
    g = bpsw_hip.make_tail_group(tb, rn, quals, pes, np.array(out_cnt, np.int32), np.concatenate(out), off, ln, names, id0=id0)
    return pac, bases, g


# ---------------------------------------------------------------------------------------------------------------------
# Genome-scale coordinates: the reference of tests/test_large_genome_gpu.py (3 100 000 019 bases, forward coordinates beyond 2^31,
# reverse-strand ones beyond 2^32) under two contig tables, with pairs PINNED at the coordinates where the tail's arithmetic turns:
# random placement reaches none of them (600 random lines: one reg2bin level, no SA:Z, no |TLEN| > 65 535).
BIG_L_PAC = 3_100_000_019
BIG_DUP = (1_200_000_000, 2_600_000_000, 1500)      # (src, dst, len): byte-aligned, inside a large contig of either table
BIG_E0 = 2 ** 31 - 1                                # "long": the first contig has ann_len's maximum
BIG_BIN_EDGES = (9 << 14, 9 << 17, 9 << 20, 9 << 23, 1 << 26, 1 << 29, 1 << 30, 10 ** 9)   # one per reg2bin level, 2^30 and ten digits
_big = {}


def big_pac():
    """the 2-bit reference, once per process; BIG_DUP's stretch copied before anybody loads it"""
    if "pac" not in _big:
        rng = np.random.default_rng(20261101)
        pac = rng.integers(0, 256, (BIG_L_PAC + 3) // 4, dtype=np.uint8)
        src, dst, n = BIG_DUP
        assert src % 4 == 0 and dst % 4 == 0 and n % 4 == 0
        pac[dst >> 2:(dst + n) >> 2] = pac[src >> 2:(src + n) >> 2]
        pac.setflags(write=False)
        _big["pac"] = pac
    return _big["pac"]


def _big_table(table):
    if table == "long":       # ann_len's maximum, a contig shorter than a read, a contig of one base, the rest
        lens = [BIG_E0, 20, 1]
        lens.append(BIG_L_PAC - sum(lens))
        names = ["chr1", "tiny20", "", "chrUn_rest.v2"]
    else:                     # "many": 3 000 contigs of 150-5 000 bases (a 20-base and a 1-base one among them) between two large ones
        rng = np.random.default_rng(20261104)
        small = [int(x) for x in rng.integers(150, 5001, 3000)]
        small[1499], small[1500] = 20, 1          # contigs 1500 and 1501
        lens = [1_400_000_000] + small
        lens.append(BIG_L_PAC - sum(lens))
        names = ["chr1"] + [("s%d" % c) if c % 3 == 0 else ("scaffold_%05d_random" % c) if c % 3 == 1 else ("KI%06d.%dv1_alt" % (c * 7, c % 10))
                            for c in range(1, 3001)] + ["chrZ"]
        names[2000] = ""
    ln = np.array(lens, np.int32)
    off = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)[:-1]]).astype(np.int64)
    assert int(off[-1] + ln[-1]) == BIG_L_PAC and len(set(names)) == len(names)
    return off, ln, names


def big_reference(table):
    """(pac, PacBases, ann_off, ann_len, names) of the "long" or the "many" table; names[k] == "" prints as ctg<k + 1>"""
    if table not in _big:
        _big[table] = _big_table(table)
    pac = big_pac()
    return (pac, synth.PacBases(pac, BIG_L_PAC)) + _big[table]


def printed_names(names):
    return [n or "ctg%d" % (k + 1) for k, n in enumerate(names)]


def big_pins(table, L):
    """-> (core, spread): each a dict(positions, mate_positions, anchor_rev, chimeric) with one entry per pair"""
    _, _, off, ln, _ = big_reference(table)
    pos, mate, rev, chim = [], [], [], []

    def add(p, p2=None, r=False, c=None):
        pos.append(p); mate.append(p2); rev.append(r); chim.append(c)

    def both(p):
        add(p); add(p, r=True)

    def cut():
        nonlocal pos, mate, rev, chim
        d = dict(positions=pos, mate_positions=mate, anchor_rev=rev, chimeric=chim)
        pos, mate, rev, chim = [], [], [], []
        return d
    src, dst, _ = BIG_DUP
    edges = [b for b in BIG_BIN_EDGES if b < int(ln[0])] + ([BIG_E0] if table == "long" else [])
    for b in edges:                                   # a read over every bin edge, on both strands
        both(b - 70)
    add(0); add(BIG_L_PAC)                            # the ends of the strand (the second is clamped to l_pac - ins - 70)
    for p in (src + 100, dst + 300, dst + 900):       # the duplicated stretch: two loci; with the mate elsewhere the ends are
        both(p)                                       # printed one by one, secondaries under MEM_F_ALL included
        add(p, 700_000_000 + p % 1000); add(640_000_000 + p % 1000, p)
    two = 2 * BIG_L_PAC
    last = int(off[-1])
    for a, b in ((1_500_000_000, 1_600_000_000), (1_700_000_123, last + 500_000_000), (two - 1_800_000_000, 1_100_000_000),
                 (1_250_000_000, two - 1_050_000_000), (two - 1_000_000_500, two - 1_900_000_000)):
        add(min(a, two - a) - 200, c=(a, b))          # chimeric ends: halves beyond 10^9 on one contig and on two, either strand
    if table == "long":
        for x in (int(off[1]), int(off[3])):          # either side of each contig boundary, and across it
            for d in (-L, 0, -L // 2, -10, 10 - L):
                both(x + d)
        both(int(off[1]) - (L - 20) // 2)             # the 20-base contig in the middle of a read: a region swallows it whole
        both(int(off[1]) + 10 - L // 2)               # ... and the middle of the read inside it
        for p, p2 in ((100, BIG_E0 - 1200), (BIG_E0 - 800, 300), (5000, BIG_E0 - 2000)):
            add(p, p2)                                # improper pairs a first contig apart: |TLEN| about 2.1e9
    else:
        both(int(off[1500]) - (L - 20) // 2)
        both(int(off[1]) - L // 2); both(int(off[3001]) - L // 2)
        add(100, 1_399_990_000); add(1_399_995_000, 300)
    core = cut()
    if table == "many":
        for c in list(range(1, 3001, 9)) + [2, 3000, 2999, 1499, 1500, 1501, 1502, 2000, 2001]:
            x, n = int(off[c]), int(ln[c])            # spread over the small contigs: inside, at the start, at the end, across
            p = (x + max(0, n // 2 - L // 2), x, x + n - L, x - L // 2)[c % 4]
            add(p, r=bool(c % 3 == 0))
    return core, cut()


def big_group(orc, table, read_len=150, n_random=40, **kw):
    """(pac, bases, group) over `table`: the core pins of big_pins twice (other errors, clips, decoys and order of the ends), the
    spread ones once and n_random pairs placed at random; regions by the oracle's memChainToAln + memSortAndDedup (C flavour).
    kw: further arguments of synth.tail_pairs (p_hard: ends without a seed, for the rescue).  Cached per process."""
    key = (table, read_len, n_random) + tuple(sorted(kw.items()))
    if key not in _big:
        pac, bases, off, ln, names = big_reference(table)
        core, spread = big_pins(table, read_len)
        pins = {k: v + v + spread[k] + [None] * n_random for k, v in core.items()}
        tb, rn, quals, pes = synth.tail_pairs(len(pins["positions"]), bases, off, ln, [BIG_DUP], read_len=read_len, seed=20261105 + read_len,
                                              **{**dict(sub_rate=0.012, indel_rate=0.003, p_span=0.0, p_dup=0.0, p_far=0.03), **kw, **pins})
        cnt, regs, _, _ = orc.chain2aln_batch(orc.default_opt(), pac, tb, po.ZDROP_BWA)
        out_cnt, out, at = [], [regs[0:0]], 0
        for c in cnt:
            r = orc.sort_dedup(regs[at:at + c], mode=po.RESCUE_C) if c else regs[0:0]
            at += c
            out_cnt.append(len(r)); out.append(r)
        g = bpsw_hip.make_tail_group(tb, rn, quals, pes, np.array(out_cnt, np.int32), np.concatenate(out), off, ln, printed_names(names), id0=4100)
        _big[key] = (pac, bases, g)
    return _big[key]


def bin_level(beg, end):
    """the level of reg2bin's bin for [beg, end): 0 for the 16 kb bins ... 5 for bin 0 (SAM specification 5.3)"""
    for k, sh in enumerate((14, 17, 20, 23, 26)):
        if beg >> sh == (end - 1) >> sh:
            return k
    return 5


def big_census(texts, g, tiny=b"tiny20"):
    """What the pinned pairs are there for, counted on SAM text alone (and, for the contig-end cut, the regions it was printed from);
    tiny: the name of the table's 20-base contig"""
    import bam_plain as bp
    c = dict(lines=0, levels=[0] * 6, bin_over_16_bits=0, pos10=0, pnext10=0, sa_pos10=0, sa=0, tlen_2e9=0, contig_end_cut=0, tiny=0,
             supp_hard=0, secondary=0, other_contig_mate=0, contigs=set(), tag_S=0, reverse=0, unmapped=0)
    at = np.concatenate([[0], np.cumsum(g.reg_cnt)])
    for r, t in enumerate(texts):
        whole = at[r + 1] > at[r] and all(x["qb"] == 0 and x["qe"] == g.read_len[r] for x in g.regs[at[r]:at[r + 1]])
        for line in t.split(b"\n")[:-1]:
            f = line.split(b"\t")
            flag, pos = int(f[1]), int(f[3])
            c["lines"] += 1
            c["pnext10"] += int(f[7]) >= 10 ** 9
            c["tlen_2e9"] += abs(int(f[8])) > 2 * 10 ** 9
            c["other_contig_mate"] += f[6] not in (b"=", b"*")
            for x in f[11:]:
                if x.startswith(b"SA:Z:"):
                    c["sa"] += 1
                    c["sa_pos10"] += any(int(a.split(b",")[1]) >= 10 ** 9 for a in x[5:].split(b";") if a)
                elif x[3:5] == b"i:":
                    c["tag_S"] += 256 <= int(x[5:]) <= 65535
            if flag & 4:
                c["unmapped"] += 1
                continue
            ops = bp.parse_cigar(f[5])
            ref_len = sum(n for n, op in ops if op in (0, 2, 3, 7, 8))
            lv = bin_level(pos - 1, pos - 1 + max(ref_len, 1))
            c["levels"][lv] += 1
            c["bin_over_16_bits"] += bp.reg2bin(pos - 1, pos - 1 + max(ref_len, 1)) > 0xffff
            c["pos10"] += pos >= 10 ** 9
            c["contigs"].add(f[2])
            c["tiny"] += f[2] == tiny
            c["reverse"] += bool(flag & 16)
            c["supp_hard"] += bool(flag & 0x800) and b"H" in f[5]
            c["secondary"] += bool(flag & 0x100)
            c["contig_end_cut"] += whole and not flag & 0x900 and any(op in (4, 5) for _, op in ops)
    c["contigs"] = len(c["contigs"])
    return c


def region_jobs(g):
    """every region of a group as a memRegToAln job -> (read_len, read_off, regs); the read pool is the group's"""
    rl = np.repeat(g.read_len, g.reg_cnt).astype(np.int32)
    ro = np.repeat(g.read_off, g.reg_cnt).astype(np.int64)
    return rl, ro, np.ascontiguousarray(g.regs)


def big_hand_jobs(table):
    """Regions built by hand in the manner of test_reg2aln_edges_gpu.py's families -- exact, a leading and a trailing deletion,
    clips, each also flipped to the reverse strand -- at the coordinates where 32 bits end: forward starts 2^31 -+ 75, doubled-space
    starts 2^32 -+ 75 (reverse strand), the first contig's end, the last contig's end (l_pac; flipped: the first base of the reverse
    strand), the start of the strand (flipped: a region ending exactly at 2 l_pac) and the bridge over l_pac.
    -> (read_len, read_off, read_pool, regs, families)"""
    from test_reg2aln_edges_gpu import O, _arrays, _flip, _job
    _, b, off, ln, _ = big_reference(table)
    l_pac, L = BIG_L_PAC, 150
    rng = np.random.default_rng(20261106)
    e1 = int(off[1])                                  # the first contig's end
    at = {"2^31-75": 2 ** 31 - 75, "2^31+75": 2 ** 31 + 75, "2^32-75": 2 * l_pac - (2 ** 32 - 75) - L, "2^32+75": 2 * l_pac - (2 ** 32 + 75) - L,
          "end1": e1 - L, "over_end1": e1 - 100, "from_end1": e1 - 50, "l_pac": l_pac - L, "start": 0}
    out = []
    for where, x in at.items():
        read = b[x:x + L]
        fam = [_job("exact@" + where, read, x, x + L, 0, L, L)]
        if x >= 5:
            fam.append(_job("lead_del@" + where, read, x - 5, x + L, 0, L, L - O - 5))
        if x + L + 3 <= l_pac:
            fam.append(_job("trail_del@" + where, read, x, x + L + 3, 0, L, L - O - 3))
        clipped = np.concatenate([rng.integers(0, 4, 12).astype(np.uint8), read[12:L - 9], rng.integers(0, 4, 9).astype(np.uint8)])
        fam.append(_job("clip@" + where, clipped, x + 12, x + L - 9, 12, L - 9, L - 21))
        sub = read.copy(); sub[[20, 75, 140]] = (sub[[20, 75, 140]] + 1) & 3
        fam.append(_job("subst@" + where, np.delete(sub, 60), x, x + L, 0, L - 1, L - 1 - O - 1 - 12))   # a deletion in the read: the DP runs
        out += fam + [_flip(j, l_pac) for j in fam]
    assert any(j["rb"] == 2 ** 32 - 75 for j in out) and any(j["rb"] == 2 ** 32 + 75 for j in out)
    assert any(j["re"] == 2 * l_pac for j in out) and any(j["rb"] == l_pac for j in out) and any(j["re"] == l_pac for j in out)
    out.append(_job("bridge", rng.integers(0, 4, L), l_pac - 50, l_pac + 100, 0, L, L))
    return _arrays(out) + ([j["family"] for j in out],)


def big_reg2aln_jobs(orc, table):
    """the memRegToAln jobs at genome scale: every region of the 2 x 150 and ("long") the 2 x 250 group, then big_hand_jobs
    -> (read_len, read_off, read_pool, regs, number of jobs that came from groups)"""
    key = ("jobs", table)
    if key not in _big:
        parts = [big_group(orc, table, 150)[2]] + ([big_group(orc, "long", 250)[2]] if table == "long" else [])
        rl, ro, pool, regs, base = [], [], [], [], 0
        for g in parts:
            a, o, r = region_jobs(g)
            rl.append(a); ro.append(o + base); regs.append(r); pool.append(np.asarray(g.read_pool, np.uint8))
            base += pool[-1].size
        hl, ho, hp, hr, _ = big_hand_jobs(table)
        n_group = int(sum(len(r) for r in regs))
        _big[key] = (np.concatenate(rl + [hl]), np.concatenate(ro + [ho + base]), np.concatenate(pool + [hp]),
                     np.concatenate(regs + [hr.astype(regs[0].dtype)]), n_group)
    return _big[key]


def without_regions_of(g, reads):
    """a copy of the group in which the reads `reads` (indices in (pair, end) order) have no region: ends for the rescue to find"""
    import copy
    at = np.concatenate([[0], np.cumsum(g.reg_cnt)])
    drop = set(int(r) for r in reads)
    g2 = copy.copy(g)
    g2.reg_cnt = np.array([0 if r in drop else int(c) for r, c in enumerate(g.reg_cnt)], np.int32)
    g2.regs = np.ascontiguousarray(np.concatenate([g.regs[0:0]] + [g.regs[at[r]:at[r + 1]] for r in range(len(g.reg_cnt)) if r not in drop]))
    return g2
