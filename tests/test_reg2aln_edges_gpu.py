"""memRegToAln on the device (bpsw_reg2aln.hip) on regions built by hand, one family per branch of the kernel's control flow, against
Oracle.reg2aln_batch in both flavours: every field, every CIGAR word, every MD byte.  Each family is COUNTED -- from its construction
or from the oracle's outputs -- so that a drift of the generator cannot empty it silently."""
import numpy as np
import pytest

import bpsw_hip
import pyoracle as po
from bpsw_hip import synth
from tail_util import synthetic_group

pytestmark = pytest.mark.gpu

CONTIGS = [30_000, 20, 20_000, 25_000]          # (the second one is shorter than a read: a region can swallow it)
FLAVOURS = (bpsw_hip.TAIL_SCALA, bpsw_hip.TAIL_C)
A, O, E, OPT_W = 1, 6, 1, 100                   # default scoring: match 1, gap open 6, extend 1; opt.w


def _reference():
    pac, bases, off, ln, names, _ = synth.contig_reference(CONTIGS, seed=20261201)
    return pac, np.asarray(bases[: sum(CONTIGS)], np.uint8), off, ln, names


def infer_bw(l1, l2, score, a=A, q=O, r=E):      # inferBw, MemRegToADAMSAM.scala:127-140
    if l1 == l2 and l1 * a - score < (q + r - a) << 1:
        return 0
    return max(int((min(l1, l2) * a - score - q) / r + 2.), abs(l1 - l2))


def _job(family, read, rb, re, qb, qe, truesc, w=OPT_W):
    return dict(family=family, read=np.asarray(read, np.uint8), rb=int(rb), re=int(re), qb=int(qb), qe=int(qe), truesc=int(truesc), w=int(w))


def _flip(j, l_pac):
    """the same hit on the reverse strand: the read reverse-complemented, the window mirrored"""
    r = j["read"][::-1]
    L = len(r)
    return dict(j, family=j["family"] + "/rev", read=np.where(r < 4, 3 - r, 4).astype(np.uint8), rb=2 * l_pac - j["re"], re=2 * l_pac - j["rb"],
                qb=L - j["qe"], qe=L - j["qb"])


def _families(b, off, l_pac):
    rng = np.random.default_rng(20261202)
    out, p = [], 1000

    def nxt():
        nonlocal p
        p += 700
        return p

    def other(x):                                # bases that match nothing at their place
        return ((x + 1 + rng.integers(0, 3, len(x))) & 3).astype(np.uint8)

    for L in (150, 64, 251):                     # exact hit, truesc = a * len: inferBw gives 0, no DP
        x = nxt(); out.append(_job("exact", b[x:x + L], x, x + L, 0, L, L))
        x = nxt(); r = b[x:x + L].copy(); r[L // 2] = 4
        out.append(_job("exact_N", r, x, x + L, 0, L, L - 2))
    for gap, fam in ((20, "retry2"), (30, "retry3")):   # an insertion and a deletion of `gap` bases, 100 bases apart, net length 0;
        for _ in range(3):                              # the region claims a score 15 below perfect: first band 11
            x = nxt()
            read = np.concatenate([b[x:x + 50], other(b[x + 50:x + 50 + gap]), b[x + 50:x + 150], b[x + 150 + gap:x + 210 + gap]])
            n = len(read)
            out.append(_job(fam, read, x, x + n, 0, n, n - 15))
    for _ in range(3):                           # the score repeats: a one-base deletion and five substitutions under a claim of
        x = nxt(); r = np.delete(b[x:x + 150], 75)     # len - 1; the second round has the same band (|d| + 3) and the same score
        for k in (10, 40, 70, 100, 130):
            r[k] = (r[k] + 1) & 3
        out.append(_job("repeat_stop", r, x, x + 150, 0, 149, 149))
    for wreg in (50, 12):                        # truesc so low that inferBw exceeds opt.w: clamped by the region's own w
        x = nxt(); out.append(_job("clamp", b[x:x + 150], x, x + 150, 0, 150, 20, w=wreg))
    for k in (5, 1):                             # the window starts / ends k bases off the read: a leading / trailing deletion
        x = nxt(); out.append(_job("lead_del", b[x:x + 150], x - k, x + 150, 0, 150, 150 - O - k))
        x = nxt(); out.append(_job("trail_del", b[x:x + 150], x, x + 150 + k, 0, 150, 150 - O - k))
    e3 = int(off[3])                             # over a contig end: the middle decides the contig, the rest is cut and clipped
    out.append(_job("contig_end_right", b[e3 - 100:e3 + 50], e3 - 100, e3 + 50, 0, 150, 150))
    out.append(_job("contig_end_left", b[e3 - 50:e3 + 100], e3 - 50, e3 + 100, 0, 150, 150))
    s = int(off[1])                              # the 20-base contig lies inside a 30-base deletion of the read: qb == qe after the cut
    out.append(_job("collapse", np.concatenate([b[s - 105:s - 5], b[s + 25:s + 125]]), s - 105, s + 125, 0, 200, 200 - O - 30))
    for qb_, tail in ((10, 0), (0, 15), (10, 15), (0, 0)):
        x = nxt()
        read = np.concatenate([other(b[x - qb_:x]), b[x:x + 100], other(b[x + 100:x + 100 + tail])])
        out.append(_job("clip%d%d" % (qb_ > 0, tail > 0), read, x, x + 100, qb_, qb_ + 100, 100))
    out += [_flip(j, l_pac) for j in out]
    out.append(_job("bridge", rng.integers(0, 4, 150), l_pac - 50, l_pac + 100, 0, 150, 150))   # a region bridging the two strands
    return out


def _arrays(jobs):
    rl = np.array([len(j["read"]) for j in jobs], np.int32)
    ro = np.concatenate([[0], np.cumsum(rl)[:-1]]).astype(np.int64)
    pool = np.concatenate([j["read"] for j in jobs] + [np.zeros(16, np.uint8)])
    regs = np.zeros(len(jobs), bpsw_hip.ALNREG_DTYPE)
    for i, j in enumerate(jobs):
        regs[i] = (j["rb"], j["re"], j["qb"], j["qe"], j["truesc"], j["truesc"], 0, 0, 0, j["w"], j["qe"] - j["qb"], -1, 0)
    return rl, ro, pool, regs


def _both(ctx, orc, ref, jobs, flavour, cap=64, md=512):
    pac, _, off, ln, _ = ref
    rl, ro, pool, regs = _arrays(jobs)
    want = orc.reg2aln_batch(orc.default_opt(), orc.default_tail_opt(), pac, sum(CONTIGS), off, ln, rl, ro, pool, regs, flavour=flavour,
                             cigar_cap=cap, md_cap=md)
    got = ctx.reg2aln_batch(bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(flavour), rl, ro, pool, regs, max_cigar=cap, max_md=md)
    for f in want[0].dtype.names:
        bad = np.nonzero(want[0][f] != got[0][f])[0]
        assert bad.size == 0, (flavour, f, [(jobs[i]["family"], int(want[0][f][i]), int(got[0][f][i])) for i in bad[:5]])
    # the words / bytes a job has (n_cigar, md_len: compared above), all of them; behind them the library leaves the zeros it was given,
    # while the oracle's row may keep the tail of a longer MD text that an earlier, narrower round of the band retry wrote there
    for what, k, cnt in (("cigar", 1, "n_cigar"), ("md", 2, "md_len")):
        for i in range(len(jobs)):
            n, room = int(want[0][cnt][i]), want[k].shape[1]
            n = 0 if want[0]["status"][i] == bpsw_hip.ALN_XREF or (what == "cigar" and n > room) else min(n, room)
            assert np.array_equal(want[k][i][:n], got[k][i][:n]) and not got[k][i][n:].any(), \
                (flavour, what, jobs[i]["family"], want[k][i][:n].tobytes(), got[k][i][:n + 8].tobytes())
    return want


def _load(ctx, ref):
    pac, _, off, ln, names = ref
    ctx.ref_load(pac, sum(CONTIGS))
    ctx.bns_load(off, ln, names)


def _ops(cig_row, n):
    return [(int(c) >> 4, int(c) & 15) for c in cig_row[:n]]


@pytest.mark.parametrize("flavour", FLAVOURS, ids=["scala", "c"])
def test_hand_built_families_vs_oracle(ctx, orc, flavour):
    ref = _reference()
    _, b, off, ln, _ = ref
    l_pac = sum(CONTIGS)
    jobs = _families(b, off, l_pac)
    _load(ctx, ref)
    alns, cig, md = _both(ctx, orc, ref, jobs, flavour)
    count = {}
    for i, j in enumerate(jobs):
        fam, a, ops = j["family"].split("/")[0], alns[i], _ops(cig[i], alns[i]["n_cigar"])
        rev = j["family"].endswith("/rev")
        lq, lr = j["qe"] - j["qb"], j["re"] - j["rb"]
        w1 = infer_bw(lq, lr, j["truesc"])
        took = False
        if fam in ("exact", "exact_N"):
            took = w1 == 0 and lq == lr and ops == [(lq, 0)] and a["NM"] == (fam == "exact_N") and a["status"] == 0
        elif fam in ("retry2", "retry3"):          # the gaps are longer than the first band (retry3: than the second, too), and are found
            gap = 20 if fam == "retry2" else 30
            took = 0 < w1 < gap and (fam == "retry2") == (2 * w1 >= gap) and 4 * w1 >= gap and (gap, 1) in ops and (gap, 2) in ops
        elif fam == "repeat_stop":                 # the alignment stays more than `a` below the claim, and its band cannot grow past |d| + 3
            took = 0 < w1 and 2 * w1 <= abs(lr - lq) + 3 and a["NM"] >= 6 and a["status"] == 0
        elif fam == "clamp":
            took = w1 > OPT_W > j["w"] and ops == [(150, 0)]
        elif fam in ("lead_del", "trail_del"):     # the deletion is dropped from the CIGAR and, where it leads, moves the position
            k = lr - lq
            start = (j["rb"] if not rev else 2 * l_pac - j["re"]) + (k if fam == "lead_del" else 0)   # (forward coordinates)
            took = ops == [(150, 0)] and a["pos"] == start and a["NM"] == 0 and a["md_len"] == 3
        elif fam in ("contig_end_right", "contig_end_left"):
            took = a["status"] == 0 and sorted(ops) == [(50, 3), (100, 0)] and a["rid"] == (2 if fam == "contig_end_right" else 3)
        elif fam == "collapse":
            took = a["status"] == bpsw_hip.ALN_XREF
        elif fam == "bridge":
            took = a["status"] == bpsw_hip.ALN_XREF and j["rb"] < l_pac < j["re"]
        elif fam.startswith("clip"):
            c5, c3 = (j["qb"], len(j["read"]) - j["qe"]) if not rev else (len(j["read"]) - j["qe"], j["qb"])
            took = ops == [(c5, 3)] * (c5 > 0) + [(100, 0)] + [(c3, 3)] * (c3 > 0)
        assert took, (j["family"], dict(zip(a.dtype.names, a.tolist())), ops, w1)
        assert bool(a["is_rev"]) == rev or a["status"] != 0, j["family"]
        count[j["family"]] = count.get(j["family"], 0) + 1
    want = {"exact": 3, "exact_N": 3, "retry2": 3, "retry3": 3, "repeat_stop": 3, "clamp": 2, "lead_del": 2, "trail_del": 2, "contig_end_right": 1,
            "contig_end_left": 1, "collapse": 1, "clip10": 1, "clip01": 1, "clip11": 1, "clip00": 1}
    assert count == {**want, **{k + "/rev": v for k, v in want.items()}, "bridge": 1}, count
    print("reg2aln families, flavour", flavour, ":", count)


def _lds_per_wave(qcap, rcap):                   # reg2aln_lds_per_wave with md_cap = 2 qcap + rcap + 32 (bpsw_tail.cpp, bpsw_reg2aln.hip)
    return (8 * (qcap + 2) + 4 * 512 + 5 * qcap + qcap + rcap + (2 * qcap + rcap + 32) + 15) & ~15


def _resident_waves(num_cu, max_read, max_region):
    lds = _lds_per_wave((max_read + 31) & ~31, (max_region + 31) & ~31) * 4
    return num_cu * min(8, max(1, (160 * 1024) // lds)) * 4


@pytest.mark.parametrize("read_len,region,next_read,next_region", [(864, 224, 864, 225), (352, 4096, 353, 4096)])
def test_lds_limit_from_the_formula(ctx, orc, read_len, region, next_read, next_region):
    """include/bpsw.h: a launch passes when 8 Q + R <= 7144 (Q, R = longest read / region rounded up to 32).  The largest pair that
    passes runs and equals the oracle; the next one is refused with BPSW_ERR_LIMIT."""
    assert _lds_per_wave((read_len + 31) & ~31, (region + 31) & ~31) * 4 <= 64 * 1024 < _lds_per_wave((next_read + 31) & ~31, (next_region + 31) & ~31) * 4
    ref = _reference()
    _, b, off, ln, _ = ref
    _load(ctx, ref)
    rng = np.random.default_rng(5)

    def job(rl, rg):
        lq = min(rl, 224)                                                     # the aligned part of the read; the rest is clipped
        x, qb = 3000, (rl - lq) // 2
        read = rng.integers(0, 4, rl).astype(np.uint8)
        read[qb:qb + lq] = b[x:x + lq]
        return _job("limit", read, x, x + rg, qb, qb + lq, lq - O - (rg - lq))
    for flavour in FLAVOURS:
        _both(ctx, orc, ref, [job(read_len, region)], flavour)
    rl, ro, pool, regs = _arrays([job(next_read, next_region)])
    with pytest.raises(bpsw_hip.BpswError, match=r"\(-4\)"):
        ctx.reg2aln_batch(bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(), rl, ro, pool, regs)


@pytest.mark.parametrize("order,flavour", [("long_to_short", bpsw_hip.TAIL_SCALA), ("short_to_long", bpsw_hip.TAIL_C), ("shuffled", bpsw_hip.TAIL_SCALA)])
def test_more_jobs_than_resident_waves(ctx, orc, order, flavour):
    """Grid-stride reuse in reg2aln_kernel: more jobs than the launch has waves, reads of 40-300 bases on both strands, so a wave's
    staged sequences, profile, CIGAR and MD stage serve a second job of another length"""
    ref = _reference()
    _, b, off, ln, _ = ref
    l_pac = sum(CONTIGS)
    rng = np.random.default_rng(20261203)
    jobs = []
    for k in range(6400):
        L = int(rng.integers(40, 301))
        x = int(rng.integers(400, 29_000 - L))
        read, ref_len = b[x:x + L].copy(), L
        kind = k % 4
        if kind == 1:                                                          # substitutions
            for q in rng.integers(0, L, 3):
                read[q] = (read[q] + 1) & 3
        elif kind == 2:                                                        # a deletion of 1-8 bases
            d = int(rng.integers(1, 9)); read = np.delete(read, slice(L // 2, L // 2 + d)); L -= d
        elif kind == 3:                                                        # an insertion of 1-8 bases
            d = int(rng.integers(1, 9)); read = np.insert(read, L // 3, rng.integers(0, 4, d)); L += d
        gaps = abs(L - ref_len)
        j = _job("many", read, x, x + ref_len, 0, L, min(L, ref_len) - (O + gaps if gaps else 0) - (15 if kind == 1 else 0))
        jobs.append(_flip(j, l_pac) if k % 3 == 0 else j)
    by_len = sorted(range(len(jobs)), key=lambda i: len(jobs[i]["read"]))
    jobs = {"long_to_short": [jobs[i] for i in reversed(by_len)], "short_to_long": [jobs[i] for i in by_len], "shuffled": jobs}[order]
    resident = _resident_waves(ctx.num_cu(), max(len(j["read"]) for j in jobs),
                               max(j["re"] - j["rb"] for j in jobs))
    print(f"reg2aln many/{order}: n = {len(jobs)} jobs, resident waves = {resident}")
    assert len(jobs) > resident, (len(jobs), resident)                        # else the test proves nothing
    _load(ctx, ref)
    alns, _, _ = _both(ctx, orc, ref, jobs, flavour, cap=16, md=64)
    assert (alns["status"] == 0).all() and (alns["n_cigar"] <= 16).all() and int(alns["is_rev"].sum()) > 2000


@pytest.mark.parametrize("flavour", FLAVOURS, ids=["scala", "c"])
def test_resubmission_ladder_is_climbed(ctx, orc, flavour):
    """Reads of 250 bases at 10 % substitutions and 3 % indels through bpsw_sam_pe_batch (single-end mode, every hit printed): some
    alignments need more than the 16 operations / 64 MD bytes of the first launch and are launched again with 128 / 512.  The text
    equals the oracle's, and the number of resubmitted jobs equals what the oracle's memRegToAln says of the same jobs."""
    pac, g = synthetic_group(orc, 120, 20261204, read_len=250, sub_rate=0.10, indel_rate=0.03)
    ctx.ref_load(pac, g.l_pac)
    ctx.bns_load(g.ann_off, g.ann_len, [bytes(g.ann_name_pool[int(g.ann_name_off[i]):int(g.ann_name_off[i + 1])]).decode() for i in range(len(g.ann_len))])
    opt, oopt = bpsw_hip.default_opt(), orc.default_opt()
    opt.flag = oopt.flag = bpsw_hip.MEM_F_NOPAIRING | bpsw_hip.MEM_F_ALL
    want, regs, _ = orc.sam_pe_batch(oopt, orc.default_tail_opt(), pac, g, flavour)
    # the jobs of that mode (bpsw_tail.cpp, the no-pairing plan): every region of score >= T that is primary or at least half its parent
    rl, ro, sel, at = [], [], [], 0
    for r in range(2 * g.group_size):
        a = regs[at:at + int(g.reg_cnt[r])]
        for k in range(len(a)):
            if a[k]["score"] >= opt.T and a[k]["rb"] >= 0 and not (a[k]["secondary"] >= 0 and a[k]["score"] < a[int(a[k]["secondary"])]["score"] * .5):
                rl.append(int(g.read_len[r])); ro.append(int(g.read_off[r])); sel.append(at + k)
        at += int(g.reg_cnt[r])
    alns, _, _ = orc.reg2aln_batch(oopt, orc.default_tail_opt(), pac, g.l_pac, g.ann_off, g.ann_len, rl, ro, g.read_pool, regs[sel], flavour=flavour,
                                   cigar_cap=600, md_cap=4096)
    first = (alns["n_cigar"] > 16) | (alns["md_len"] > 64)
    second = (alns["n_cigar"] > 128) | (alns["md_len"] > 512)
    got, _ = ctx.sam_pe_batch(opt, bpsw_hip.default_tail_opt(flavour), g)
    resub = ctx.last_tail_resubmitted()
    print(f"resubmission, flavour {flavour}: {len(sel)} jobs, {int(first.sum())} outgrew 16 operations / 64 MD bytes, {int(second.sum())} outgrew 128 / 512; "
          f"the library resubmitted {resub}")
    assert got == want
    assert int(first.sum()) >= 20 and resub == int(first.sum()) + int(second.sum())
    assert ctx.last_tail_kernel()[1] == len(sel)
