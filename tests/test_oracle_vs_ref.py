"""Cross-checks the oracle against the reference's own C compiled in place (oracle/_ref), live, on larger
seeded samples than the committed fixtures.  Skipped where oracle/_ref/libbwaref.so is absent."""
import numpy as np

import chain_cases
import global_cases
import pyoracle as po
from bpsw_hip import synth
from conftest import region_fields_equal

MAT = po.default_mat()


def test_sw_extend_on_synthetic_tasks(orc, ref):
    for L, sub, ind, tail in ((150, 0.01, 0.001, 0.0), (250, 0.1, 0.02, 0.2)):
        soa = synth.ext_tasks(600, read_len=L, sub_rate=sub, indel_rate=ind, tail_frac=tail, seed=31 + L)
        calls = 0
        for i in range(soa.n):
            for side in ("left", "right"):
                ql, rl = int(getattr(soa, side + "_qlen")[i]), int(getattr(soa, side + "_rlen")[i])
                if ql == 0:
                    continue
                q = soa.pool[getattr(soa, side + "_q_off")[i]:][:ql]
                t = soa.pool[getattr(soa, side + "_r_off")[i]:][:rl]
                for w in (100, 200):
                    got, _ = orc.sw_extend(q, t, MAT, 6, 1, 6, 1, w, 5, 100, int(soa.h0[i]), po.ZDROP_BWA)
                    assert np.array_equal(got, ref.ksw_extend2(q, t, MAT, 6, 1, 6, 1, w, 5, 100, int(soa.h0[i])))
                    calls += 1
        assert calls > 1000


def test_sw_align2_on_synthetic_jobs(orc, ref):
    opt = orc.default_opt()
    for L in (100, 150, 250):
        jobs = synth.sw_jobs(150, read_len=L, seed=9 + L)
        xtra = po.KSW_XSUBO | po.KSW_XSTART | (po.KSW_XBYTE if L < 250 else 0) | 19
        got, _ = orc.sw_align2_jobs(opt, xtra, **jobs)
        for i in range(len(got)):
            q = jobs["q_pool"][jobs["q_off"][i]:][:jobs["q_len"][i]]
            if jobs["q_rev"][i]:
                q = np.where(q[::-1] < 4, 3 - q[::-1], 4).astype(np.uint8)
            want = ref.ksw_align2(q, jobs["t_pool"][jobs["t_off"][i]:][:jobs["t_len"][i]], MAT, 6, 1, 6, 1, xtra)
            assert np.array_equal(got[i][[0, 1, 2, 5, 6]], want[[0, 1, 2, 5, 6]])


def test_group_rescue_c_mode(orc, ref):
    opt = orc.default_opt()
    for allo, n, p in ((False, 200, 0.4), (True, 60, 0.5)):
        g = synth.rescue_group(n, seed=55 + n, p_resc=p, all_orientations=allo, p_multi_anchor=0.4)
        cnt, regs, n_sw, _ = orc.matesw_group(opt, g, po.RESCUE_C)
        rcnt, rregs = ref.matesw_group(opt, g)
        assert n_sw > 0 and np.array_equal(cnt, rcnt)
        region_fields_equal(regs, rregs, skip=("csub",))


def test_bns_get_seq_live(orc, ref):
    rng = np.random.default_rng(5)
    l_pac = 200_003
    pac = rng.integers(0, 256, (l_pac + 3) // 4, dtype=np.uint8)
    for t in range(2000):
        b = int(rng.integers(-100, 2 * l_pac))
        e = b + int(rng.integers(0, 1200))
        if t % 5 == 0:
            b = l_pac - int(rng.integers(0, 600)); e = b + int(rng.integers(0, 1200))
        if t % 9 == 0:
            b, e = e, b
        assert np.array_equal(orc.bns_get_seq(l_pac, pac, b, e), ref.bns_get_seq(l_pac, pac, b, e))


def test_chain2aln_live(orc, ref):
    l_pac = 400_009
    pac, bases = synth.random_pac(l_pac, seed=61)
    for L, es, ei, tail in ((150, 0.01, 0.001, 0.0), (250, 0.08, 0.02, 0.05), (100, 0.04, 0.01, 0.2)):
        b = synth.read_chains(1500, bases, l_pac, read_len=L, sub_rate=es, indel_rate=ei, tail_frac=tail, seed=62 + L)
        cnt, regs, n_ext, _ = orc.chain2aln_batch(orc.default_opt(), pac, b, po.ZDROP_BWA)
        rcnt, rregs = ref.chain2aln_batch(orc.default_opt(), pac, b)
        assert np.array_equal(cnt, rcnt)
        for f in regs.dtype.names:
            assert np.array_equal(regs[f], rregs[f]), (L, f)
        assert n_ext > 1000


def _global_both(orc, ref, job, s):
    got = orc.sw_global(job.q, job.t, s.mat, s.o_del, s.e_del, s.o_ins, s.e_ins, job.w)
    want = ref.ksw_global2(job.q, job.t, s.mat, s.o_del, s.e_del, s.o_ins, s.e_ins, job.w)
    return got, want


def test_sw_global_on_generated_cases(orc, ref):
    """Every group of tests/global_cases.py but `many` (chunk-edge lengths and bands, up to 12 edits with indels of 40, tie-rich input,
    CIGARs of 500-700 operations) under its five scorings: the oracle's SWGlobal against the reference's ksw_global2, score and every
    CIGAR word.  (test_sw_global_on_the_fixture_subset below is the part of it that became tests/golden/ksw_global2_edges.npz.)"""
    compared = 0
    for name, make in global_cases.GROUPS.items():
        jobs = make()
        for s in global_cases.SCORINGS:
            for i, job in enumerate(jobs):
                assert job.w >= abs(len(job.t) - len(job.q)), (name, i)      # in-domain, all of them: nothing is filtered
                (gs, gc), (ws, wc) = _global_both(orc, ref, job, s)
                assert gs == ws and gs > global_cases.MINUS_INF // 2, (name, s.name, i, gs, ws)
                assert np.array_equal(gc, wc), (name, s.name, i, gc, wc)
                compared += 1
    print(f"sw_global vs ksw_global2: {compared} jobs compared")
    assert compared >= 5 * 2000


def test_sw_global_on_the_fixture_subset(orc, ref):
    """the jobs of tests/golden/ksw_global2_edges.npz (a fifth of them, to keep the recording small) through the same comparison"""
    picked = global_cases.fixture_subset()[::5]
    for job, si in picked:
        (gs, gc), (ws, wc) = _global_both(orc, ref, job, global_cases.SCORINGS[si])
        assert gs == ws and np.array_equal(gc, wc), (si, len(job.q), len(job.t), job.w)
    assert len(picked) >= 250


def test_sw_global_below_the_band_rule_agrees_on_the_score_only(orc, ref):
    """w < |tLen - qLen|: the last cell is outside the band.  Reference and oracle both answer -2^30; the CIGAR either leaves is an
    accident of its backtrack (they differ in about one job of eight, and the reference's own differs from run to run) and is NOT
    compared.  For that reason this test has no recording and runs where the reference is built only.  bpsw_global_batch refuses
    such jobs."""
    jobs = global_cases.below_band()
    for s in global_cases.SCORINGS:
        for i, job in enumerate(jobs):
            (gs, _), (ws, _) = _global_both(orc, ref, job, s)
            assert gs == ws == global_cases.MINUS_INF, (s.name, i, gs, ws)
    assert len(jobs) >= 400


def _chain_both(orc, ref, o, w, b):
    pac = chain_cases.reference()[0]
    cnt, regs, _, _ = orc.chain2aln_batch(chain_cases.apply(orc.default_opt(), o, w), pac, b, po.ZDROP_BWA)
    rcnt, rregs = ref.chain2aln_batch(chain_cases.apply(orc.default_opt(), o, w), pac, b)
    return cnt, regs, rcnt, rregs


def test_chain2aln_on_generated_cases(orc, ref):
    """Every family of tests/chain_cases.py (requeue reduced to its heavy reads and their neighbours) under its five option sets, at
    the band widths the family names (2, 3, 100, 127, 254): the oracle's round loop in the BWA z-drop parse against the reference's
    mem_chain2aln, counts and every field of every region, nothing filtered; and each family's promise on the oracle's output."""
    reads = regions = calls = 0
    for name, make in chain_cases.GROUPS.items():
        fam = make()
        for oi, o in enumerate(chain_cases.OPTIONS):
            results = []
            for w, b in fam.batches:
                assert w >= 2
                cnt, regs, rcnt, rregs = _chain_both(orc, ref, o, w, b)
                assert np.array_equal(cnt, rcnt), (name, o.name, w)
                for f in regs.dtype.names:
                    assert np.array_equal(regs[f], rregs[f]), (name, o.name, w, f)
                results.append((cnt, regs))
                reads += len(cnt); regions += len(regs); calls += 1
            print(f"{name} / {o.name}: {fam.promise(oi, results)}")
    print(f"chain2aln vs mem_chain2aln: {reads} reads, {regions} regions, {calls} reference calls compared")
    assert calls == 5 * 11 and regions > 20000


def _only_where_the_c_tried_again(regs, rregs, where):
    """rows of two region lists that differ in any field have w = 2 in the reference's; returns how many, and how many beyond w"""
    assert regs.shape == rregs.shape, where
    any_diff = np.zeros(len(regs), bool)
    for f in regs.dtype.names:
        any_diff |= regs[f] != rregs[f]
    assert np.all(rregs["w"][any_diff] == 2) and np.all(regs["w"][any_diff] <= 2), where
    return any_diff, int((any_diff & ((regs["score"] != rregs["score"]) | (regs["rb"] != rregs["rb"]))).sum())


def test_chain2aln_at_w1_differs_where_the_c_tries_again(orc, ref):
    """At w = 1 the reference C and the Scala disagree, and the oracle (like the kernel) follows the Scala.
    bwamem.c:629/641 starts the left side's band loop with prev = a->score = -1, MemChainToAlignBatched.scala:558/800/811 with
    prev = regScore = seed length * a.  A left try that leaves the score unchanged therefore ends the Scala's loop (w stays 1) and
    not the C's, whose other exit, max_off < (w >> 1) + (w >> 2) = 0, cannot fire at w = 1: the C tries again at band 2, reports
    w = 2, and reports that try's alignment -- usually the same one, sometimes a better one the band of 1 did not hold (85 of the
    1 095 seed_lanes regions).  From w = 2 on that exit fires whenever the score is unchanged (max_off is 0 then) and the two
    agree (the test above).  Asserted here: the region counts agree, a region differs in ANY field only where the C reports
    w = 2, and, where a region can be traced to its seed, only where the first left try left the score unchanged (and there
    always, unless the oracle's right side went to band 2 as well and the left alignment is the same at both bands).  A difference between the two references is nothing a recording should pin down as expected output, so this test
    has none and runs where the reference is built only ("C and Scala at w = 1")."""
    o = chain_cases.OPTIONS[0]
    differ = more = compared = 0
    for name in ("region_cache", "seed_lanes", "overlap", "ends", "bases", "requeue"):
        for w0, b in chain_cases.GROUPS[name]().batches:
            cnt, regs, rcnt, rregs = _chain_both(orc, ref, o, 1, b)
            assert np.array_equal(cnt, rcnt), name
            d, m = _only_where_the_c_tried_again(regs, rregs, name)
            differ += int(d.sum()); more += m; compared += len(regs)
    # ... and where a region can be traced to its seed (every chain holds one seed and every seed made a region)
    b, seeds = chain_cases.w1_single()
    cnt, regs, rcnt, rregs = _chain_both(orc, ref, o, 1, b)
    assert np.array_equal(cnt, rcnt) and list(cnt) == [len(s) for s in seeds]
    d, m = _only_where_the_c_tried_again(regs, rregs, "w1_single")
    differ += int(d.sum()); more += m
    at = unchanged_left = 0
    for r, ss in enumerate(seeds):
        read = b.read_pool[b.read_off[r]:][:b.read_len[r]]
        for rb, qb, ln in ss:
            left_unchanged = False
            if qb > 0:
                r0, _ = chain_cases.max_span(o, 1, len(read), [(rb, qb, ln)])
                got, _ = orc.sw_extend(read[:qb][::-1], chain_cases.win(r0, rb)[::-1], o.mat, o.o_del, o.e_del, o.o_ins, o.e_ins, 1,
                                       o.pen_clip5, o.zdrop, ln * o.a, po.ZDROP_BWA)
                left_unchanged = int(got[0]) == ln * o.a
            if d[at]:
                assert left_unchanged, (r, rb, qb, ln)
            elif left_unchanged:       # the same region from both: the oracle's RIGHT side took its second try
                assert regs["w"][at] == 2, (r, rb, qb, ln)
            unchanged_left += left_unchanged
            at += 1
    print(f"w = 1: {compared + len(regs)} regions compared, {differ} differ (the C's w is 2 in all), {more} of them in score or rb too; "
          f"{unchanged_left} of {len(regs)} traced seeds left the left score unchanged")
    assert differ > 50 and unchanged_left > 50
