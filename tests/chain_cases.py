"""Generated batches for the chain-to-region round loop (memChainToAlnBatched == mem_chain2aln per chain): one generator for the
oracle-versus-reference tests on the CPU (tests/test_oracle_vs_ref.py), the reference fixture (tests/golden/make_golden.py ->
mem_chain2aln_edges.npz) and the kernel-versus-oracle tests (tests/test_chain2aln_edges_gpu.py).  Plain numpy from fixed seeds:
no GPU, no oracle.

Every family is built around one constant or one branch of csrc/bpsw_chain2aln.hip: the 64 regions a read keeps in LDS
(C2A_RCAP), the `i += 64` seed loops and their wave reductions, the srt rank with its `lj == li && j < i` tie-break,
checkOverlapping's boundaries, the second band try, the staged target rows (C2A_TCAP), window cropping at 0 / l_pac / 2 l_pac,
and a wave taking a second read.  A family is a list of (w, ChainBatchSoA) over ONE reference (reference()) and a `promise`:
a function of the ORACLE's results that raises when the batch stopped reaching the branch it was written for, so that a later
edit here cannot quietly turn a test into a restatement of the easy case.

Many seeds here are "dishonest": they name a reference position the read does not match.  The round loop never looks at whether
a seed matches; it is the geometry (containment, diagonals, lengths, ranks) that steers it, and dishonest seeds are the only way
to reach some of it (a window set by one seed alone, 200 distinct regions in one 256-base read).

Two things the issue's list asked for do not exist and are therefore not generated:
  * a longer-ranked seed ti with tl < 0.95 sl: srt is sorted by (len, index) and checkOverlapping walks i > k only, so tl >= sl
    for every ti it meets -- `tl >= 0.95 sl` is always true there (in the kernel, the oracle, the Scala and the C alike);
  * a 256-base flank: a seed has at least one base and a read at most 256, so the longest flank is 255 bases and the staged
    length min(rLen, qLen + 2w + 2) tops out at 765 of the 768 rows of C2A_TCAP.
"""
import functools
from collections import namedtuple

import numpy as np

from bpsw_hip import ChainBatchSoA, synth

L_PAC = 20_003            # not a multiple of 4: the last .pac byte is partly filled
A = 10_000                # the locus most reads are cut from; bases[A:A+256] is planted again 300 before and 300 after
PLANT = 300
RCAP = 64                 # C2A_RCAP
WAVE = 64

Options = namedtuple("Options", "name a b o_del e_del o_ins e_ins pen_clip5 pen_clip3 zdrop mat")
Family = namedtuple("Family", "batches promise")


def mat(a, b):
    m = np.full((5, 5), -1, np.int8)
    for i in range(4):
        for j in range(4):
            m[i, j] = a if i == j else -b
    return m.reshape(25)


# the general matrix of test_swalign_gpu.py::test_custom_scoring
GENERAL = np.array([1, -2, -3, -4, -1, -2, 2, -4, -3, 0, -3, -4, 1, -2, -1, -4, -3, -2, 2, -2, -1, 0, -1, -2, -1], np.int8)

OPTIONS = (
    Options("default", 1, 4, 6, 1, 6, 1, 5, 5, 100, mat(1, 4)),
    Options("m2x3_g5241", 2, 3, 5, 2, 4, 1, 5, 5, 100, mat(2, 3)),
    Options("clip0", 1, 4, 6, 1, 6, 1, 0, 0, 100, mat(1, 4)),
    Options("clip20_z10", 1, 4, 6, 1, 6, 1, 20, 20, 10, mat(1, 4)),
    Options("general_z0", 2, 4, 6, 1, 6, 1, 5, 5, 0, GENERAL),
)


def apply(opt, o: Options, w: int):
    """fill a bpsw_hip.Opt / pyoracle.Opt (same layout) from an option set and a band width; returns opt"""
    for f in ("a", "b", "o_del", "e_del", "o_ins", "e_ins", "pen_clip5", "pen_clip3", "zdrop"):
        setattr(opt, f, getattr(o, f))
    opt.w = w
    for k in range(25):
        opt.mat[k] = int(o.mat[k])
    return opt


@functools.lru_cache(None)
def reference():
    """(pac, bases): a random reference with bases[A:A+256] planted again at A-300 and A+300"""
    _, bases = synth.random_pac(L_PAC, seed=20261018)
    bases = bases.copy()
    bases[A - PLANT:A - PLANT + 256] = bases[A:A + 256]
    bases[A + PLANT:A + PLANT + 256] = bases[A:A + 256]
    padded = np.zeros(((L_PAC + 3) // 4) * 4, np.uint8)
    padded[:L_PAC] = bases
    q = padded.reshape(-1, 4)
    pac = ((q[:, 0] << 6) | (q[:, 1] << 4) | (q[:, 2] << 2) | q[:, 3]).astype(np.uint8)
    bases.setflags(write=False); pac.setflags(write=False)
    return pac, bases


def win(rb, re):
    """bases of [rb, re) in the 2 l_pac coordinates of both strands"""
    return synth.window_bases(reference()[1], L_PAC, rb, re)


class _Batch:
    def __init__(self):
        self.reads = []       # (bases, [[(rbeg, qbeg, len), ...] per chain])

    def add(self, seq, chains):
        seq = np.asarray(seq, np.uint8)
        assert 1 <= len(seq) <= 256
        for ch in chains:
            for rb, qb, ln in ch:
                assert ln >= 1 and 0 <= qb and qb + ln <= len(seq) and 0 <= rb and rb + ln <= 2 * L_PAC, (rb, qb, ln, len(seq))
                assert (rb < L_PAC) == (ch[0][0] < L_PAC) and (rb >= L_PAC or rb + ln <= L_PAC), (rb, ln)
        self.reads.append((seq, [list(ch) for ch in chains]))
        return len(self.reads) - 1

    def soa(self):
        seeds = [s for _, chains in self.reads for ch in chains for s in ch]
        lens = np.array([len(s) for s, _ in self.reads], np.int64)
        off = np.zeros(len(lens), np.int64)
        off[1:] = np.cumsum(lens)[:-1]
        pool = np.concatenate([s for s, _ in self.reads] + [np.zeros(16, np.uint8)])
        col = lambda k, dt: np.array([s[k] for s in seeds], dt).reshape(-1)
        return ChainBatchSoA(l_pac=L_PAC, read_len=lens.astype(np.int32), read_off=off, read_pool=pool,
                             chain_cnt=np.array([len(c) for _, c in self.reads], np.int32),
                             seed_cnt=np.array([len(ch) for _, c in self.reads for ch in c], np.int32),
                             seed_rbeg=col(0, np.int64), seed_qbeg=col(1, np.int32), seed_len=col(2, np.int32))


def per_read(cnt, regs):
    at = np.zeros(len(cnt) + 1, np.int64)
    at[1:] = np.cumsum(cnt)
    return [regs[at[i]:at[i + 1]] for i in range(len(cnt))]


def cal_max_gap(o: Options, w, qlen):      # MemChainToAlignBatched.scala:625-643
    ld = int((qlen * o.a - o.o_del) / o.e_del + 1.0)
    li = int((qlen * o.a - o.o_ins) / o.e_ins + 1.0)
    return min(max(ld, li, 1), w << 1)


def max_span(o: Options, w, qlen, seeds):  # getMaxSpan, :648-676
    r0 = min(rb - (qb + cal_max_gap(o, w, qb)) for rb, qb, ln in seeds)
    r1 = max(rb + ln + (qlen - qb - ln) + cal_max_gap(o, w, qlen - qb - ln) for rb, qb, ln in seeds)
    r0, r1 = max(r0, 0), min(r1, 2 * L_PAC)
    if r0 < L_PAC < r1:
        if seeds[0][0] < L_PAC:
            r1 = L_PAC
        else:
            r0 = L_PAC
    return r0, r1


def _need(cond, what):
    if not cond:
        raise AssertionError("chain_cases promise broken: " + what)


# ---------------------------------------------------------------------------------------------------------- region_cache
RC_COUNTS = (63, 64, 65, 90, 130)
RC_DECOY_C = 10           # the decoy (index < 64) whose region holds seed (c)


def _decoy(i):
    """single-seed chain i of a region_cache read: its own locus, alternating strands, 140 apart"""
    p = 200 + 140 * (i // 2)
    return [((p if i % 2 == 0 else L_PAC + p), (i * 7) % 200, 19 + i % 5)]


def region_cache_read(n):
    """250 bases cut at A.  n single-seed chains at distinct loci (n regions), then one chain: S0 whose region (index n: in LDS
    for n = 63, read back from global memory from n = 64 on) is the whole read; (a) 20 bases inside it on its diagonal -> skipped;
    (b) inside it 150 off the diagonal -> extended; (c) inside decoy 10's region only -> skipped"""
    chains = [_decoy(i) for i in range(n)]
    drb, dqb, dln = _decoy(RC_DECOY_C)[0]
    chains.append([(A + 10, 10, 60), (A + 30, 30, 20), (A + 50, 200, 20), (drb + 2, dqb + 2, dln - 4)])
    return win(A, A + 250), chains


@functools.lru_cache(None)
def region_cache():
    b = _Batch()
    for n in RC_COUNTS:
        b.add(*region_cache_read(n))

    def promise(oi, results, bwa=True):
        (cnt, regs), = results
        _need(int(cnt.max()) > RCAP, "no read with more than 64 regions")
        for n, rr in zip(RC_COUNTS, per_read(cnt, regs)):
            _rc_promise(n, rr)
        return f"{len(RC_COUNTS)} reads, {int(cnt.max())} regions in the largest"
    return Family([(100, b.soa())], promise)


def _rc_promise(n, rr):
    _need(len(rr) == n + 2, f"region_cache({n}): {len(rr)} regions, want the {n} decoys + S0 + (b); (a) or (c) was extended")
    s0, sb = rr[n], rr[n + 1]
    _need((s0["qb"], s0["qe"], s0["rb"], s0["re"]) == (0, 250, A, A + 250), f"region_cache({n}): S0 is not the whole read")
    _need(sb["rb"] <= A + 50 and sb["re"] >= A + 70 and sb["qb"] <= 200 and sb["qe"] >= 220 and sb["re"] - sb["rb"] < 250,
          f"region_cache({n}): region {n + 1} is not seed (b)'s")


# ------------------------------------------------------------------------------------------------------------ seed_lanes
SL_NS = (1, 63, 64, 65, 128, 129, 200)


def _lane_seeds(ns, diag, mode):
    out = []
    for i in range(ns):
        ln = 30 if mode == "equal" else 20 + (i // 8) % 5 if mode == "runs" else 25 + i % 7
        if mode == "late" and i == ns - 1:
            ln = 56                                   # the longest seed last: at index >= 64 from ns = 65 on
        out.append((A + i + ((i * 7) % 11 if diag == "fan" else 0), i, ln))
    return out


def seed_lanes_read(ns, diag, mode):
    """256 bases cut at A with four chains: a decoy, an EMPTY chain, the big one (seed i at query i; on one diagonal, or fanned
    over the eleven diagonals 0..10 off it: contained in the first region, kept alive by checkOverlapping or not "around" it,
    so the ranks decide the ORDER of many different regions), and one seed on the planted copy at A + 300"""
    return win(A, A + 256), [_decoy(3), [], _lane_seeds(ns, diag, mode), [(A + PLANT + 40, 40, 25)]]


def _span_read(hi):
    """65 seeds; the first 64 on the diagonal of A huddle at one end of the read, seed 64 sits on the planted copy on the other
    side: rmax1 (hi) / rmax0 (lo) comes from seed 64 alone, and its region reaches where the first 64 seeds' window would end"""
    first = [(A + q, q, 20) for q in ((200 + i % 30 if hi else i % 30) for i in range(64))]
    last = (A + (PLANT if hi else -PLANT) + 100, 100, 40)
    return win(A, A + 256), [[(A + 7, 7, 19)], first + [last], []]


SL_MANY = {(200, "fan", "equal"), (129, "fan", "equal"), (128, "fan", "late")}      # more than 64 regions in the one chain
SL_READS = tuple((ns, d, ("equal", "runs", "late")[(k + j) % 3]) for k, ns in enumerate(SL_NS) for j, d in enumerate(("one", "fan"))) + \
    ((200, "fan", "equal"), (129, "fan", "runs"), (65, "fan", "late"), (128, "one", "late"), (200, "one", "runs"))


@functools.lru_cache(None)
def seed_lanes():
    b = _Batch()
    for ns, d, mode in SL_READS:
        b.add(*seed_lanes_read(ns, d, mode))
    r_hi, r_lo = b.add(*_span_read(True)), b.add(*_span_read(False))

    def promise(oi, results, bwa=True):
        (cnt, regs), = results
        rr = per_read(cnt, regs)
        o = OPTIONS[oi]
        cov_hits = late_hits = 0
        for (ns, d, mode), g in zip(SL_READS, rr):
            seeds = _lane_seeds(ns, d, mode)
            if d == "one":      # the whole chain is one region, and every seed of it counts into seedcov
                _need(len(g) == 3, f"seed_lanes({ns},{d},{mode}): {len(g)} regions, want decoy + 1 + planted")
                _need(g[1]["seedcov"] == sum(s[2] for s in seeds), f"seed_lanes({ns},{d},{mode}): seedcov misses seeds")
                cov_hits += g[1]["seedcov"] > sum(s[2] for s in seeds[:WAVE])
            else:
                _need(ns < 63 or len(g) > 12, f"seed_lanes({ns},{d},{mode}): only {len(g)} regions, the off-diagonal seeds were skipped")
                if (ns, d, mode) in SL_MANY:
                    _need(len(g) > RCAP + 3 and len(set(g.tobytes()[k:k + 64] for k in range(0, 64 * len(g), 64))) > 10, f"seed_lanes({ns},{d},{mode}): no 64 regions in one chain")
            if mode == "late" and ns > WAVE:
                rb, qb, ln = seeds[-1]
                f = g[1]
                _need(f["rb"] <= rb and f["re"] >= rb + ln and f["qb"] <= qb and f["qe"] >= qb + ln and f["score"] >= ln * o.a,
                      f"seed_lanes({ns},{d},{mode}): the first region is not the longest seed's (index {ns - 1})")
                late_hits += 1
        _need(cov_hits >= 4 and late_hits >= 2, "seed_lanes: too few reads with seeds past lane 63")
        for r, hi in ((r_hi, True), (r_lo, False)):
            _, chains = b.reads[r]
            r0, r1 = max_span(o, 100, 256, chains[1][:WAVE])
            f0, f1 = max_span(o, 100, 256, chains[1])
            g = rr[r]
            _need(len(g) >= 2, f"seed_lanes(span {'hi' if hi else 'lo'}): {len(g)} regions")     # g[1]: seed 64's, the longest of its chain
            if hi:
                _need(f1 > r1 and g[1]["re"] > r1, "seed_lanes(span hi): no region past the first 64 seeds' rmax1")
            else:
                _need(f0 < r0 and g[1]["rb"] < r0, "seed_lanes(span lo): no region before the first 64 seeds' rmax0")
        return f"{len(rr)} reads, up to {int(cnt.max())} regions"
    return Family([(100, b.soa())], promise)


# --------------------------------------------------------------------------------------------------------------- overlap
@functools.lru_cache(None)
def overlap():
    """200 bases cut at A.  M = 60 bases at query 110 makes region 0 (the whole read).  s (sl bases at query 40, on M's diagonal)
    is contained in it; T, ranked after s (tl > sl, or tl == sl with the larger index), sits on the planted copy, is extended
    (so unmarked) and disagrees with s about the diagonal.  Whether s is extended is then the overlap rule alone."""
    b, want = _Batch(), []
    read = win(A, A + 200)
    sqb = 40
    M = (A + 110, 110, 60)

    def case(chain, regions, what):
        want.append((b.add(read, [chain]), regions, what))

    for sl in (20, 21, 40, 41):
        q4 = sl >> 2
        s = (A + sqb, sqb, sl)
        for tl in (sl, sl + 1):
            T = lambda tq: (A + PLANT + tq, tq, tl)
            case([M, s, T(sqb + sl - q4)], 3, f"sl={sl} tl={tl} sqb<=tq, overlap == sl>>2")
            case([M, s, T(sqb + sl - q4 + 1)], 2, f"sl={sl} tl={tl} sqb<=tq, overlap one short")
            case([M, s, T(sqb - tl + q4)], 3, f"sl={sl} tl={tl} tq<=sqb, overlap == sl>>2")
            case([M, s, T(sqb - tl + q4 - 1)], 2, f"sl={sl} tl={tl} tq<=sqb, overlap one short")
            case([M, s, T(sqb)], 3, f"sl={sl} tl={tl} tq == sqb")
        case([M, (A + PLANT + sqb, sqb, sl), s], 2, f"sl={sl}: equal length, T has the SMALLER index, so s is tried before T")
        case([(A + 20, 20, 60), s], 1, f"sl={sl}: the overlapping longer seed is on s's diagonal")
        case([(A + PLANT + 20, 20, 60), (A + PLANT + 30, 30, 50), s, M], 3, f"sl={sl}: two unmarked, both disagree")
        # the only seed that disagrees with s (T, 3 off s's diagonal, overlapping) is itself contained and already MARKED
        case([M, (A + 35, 35, sl + 5), (A + sqb + 3, sqb, sl)], 1, f"sl={sl}: the only disagreeing seed is marked")

    def promise(oi, results, bwa=True):
        (cnt, regs), = results
        for r, n, what in want:
            _need(cnt[r] == n, f"overlap [{what}]: {cnt[r]} regions, want {n}")
        return f"{len(want)} reads, {sum(n == 3 for _, n, _ in want)} kept alive by checkOverlapping"
    return Family([(100, b.soa())], promise)


# ------------------------------------------------------------------------------------------------------------------ band
BAND_WS = (2, 3, 100, 127, 254)
BAND_P = 15_000


def _gapped_flank(rng, p, m1, dels=(), ins=0, total=237):
    """a flank of `total` read bases that follows the reference from p: m1 matches, then `ins` foreign bases, then for every
    (matches, deleted) pair of `dels` `deleted` reference bases left out and `matches` bases copied; the rest copied"""
    out, at = [win(p, p + m1)], p + m1
    if ins:
        out.append(((win(at, at + ins) + 1 + rng.integers(0, 3, ins)) & 3).astype(np.uint8))   # differs from the reference base for base
    for k, (m, g) in enumerate(dels):
        at += g
        out.append(win(at, at + m)); at += m
    have = sum(len(x) for x in out)
    out.append(win(at, at + total - have))
    f = np.concatenate(out)
    assert len(f) == total
    return f


def _band_reads(w):
    """[(read, chains, want_w or None)]: 256-base reads, the seed at one end, one gap of g bases in the flank.

    The seed is 19 bases (a 237-base flank) for w = 2, 3 and 254 and 120 bases for w = 100 and 127: SWExtend's first row and
    column are positive for h0 - o - e cells only and its column range grows by at most one a row, so the extension of a 19-base
    seed never leaves the 13 diagonals next to the main one and max_off could not come near 0.75 w."""
    rng = np.random.default_rng(1000 + w)
    thr = (w >> 1) + (w >> 2)
    out = []
    p = BAND_P
    sl = 120 if w in (100, 127) else 19
    fl = 256 - sl
    m1 = 10 if sl == 120 else 70

    def right(flank, want):
        out.append((np.concatenate([win(p, p + sl), flank]), [[(p, 0, sl)]], want))

    def left(flank_fwd, want):
        # the mirror image on the reverse strand: the reverse complement of a right-flank read has its seed at its END
        read = np.concatenate([win(p, p + sl), flank_fwd])
        out.append(((3 - read[::-1]).astype(np.uint8), [[(2 * L_PAC - p - sl, fl, sl)]], want))

    for g in sorted({g for g in (thr - 1, thr, w, w + 1) if g >= 0}):
        # a deletion of g: the first try sees it iff g <= w; max_off == g decides the second try; the score cannot change at 2w
        feasible = sl + m1 > 6 + g and fl - m1 > 6 + g and g < sl - 7
        want = None if not feasible else (2 * w if thr <= g <= w else w)
        for put in (right, left):
            put(win(p + sl, p + 256) if g == 0 else _gapped_flank(rng, p + sl, m1, dels=((fl - m1, g),), total=fl), want)
    if w in (2, 3):
        for g in (1, w):            # an insertion of g foreign bases
            right(_gapped_flank(rng, p + sl, m1, ins=g, total=fl), 2 * w)
            left(_gapped_flank(rng, p + sl, m1, ins=g, total=fl), 2 * w)
    if w == 100:
        # two deletions, 75 then 30: the first try crosses the first (max_off 75) and not the second; the second try scores more
        right(_gapped_flank(rng, p + sl, 10, dels=((85, 75), (41, 30)), total=fl), 2 * w)
        left(_gapped_flank(rng, p + sl, 10, dels=((85, 75), (41, 30)), total=fl), 2 * w)
    if w in (2, 3, 100):
        # both flanks, a second try on ONE side only: the region's w is the larger of the two sides
        s2, f2, c2 = (100, 130, 26) if w == 100 else (19, 200, 37)      # seed, gapped flank, clean flank: 256 in all
        lf = _gapped_flank(rng, p + s2, m1, dels=((f2 - m1, thr),), total=f2)
        fwd = np.concatenate([win(p, p + s2), lf])
        rc = (3 - fwd[::-1]).astype(np.uint8)            # the seed at query f2 of the reverse-strand read, the gap on its LEFT
        out.append((np.concatenate([rc, win(2 * L_PAC - p, 2 * L_PAC - p + c2)]), [[(2 * L_PAC - p - s2, f2, s2)]], 2 * w))
        out.append((np.concatenate([win(p - c2, p), fwd]), [[(p, c2, s2)]], 2 * w))    # ... and on its right
    if w == 254:
        # 255- and 254-base flanks with a helper seed that widens the window: min(rLen, qLen + 2w + 2) reaches 765 / 764
        for k in (1, 2):
            out.append((win(p, p + 256), [[(p + 256 - k, 256 - k, k), (p - 300, 250, 3)]], None))
            out.append((win(p, p + 256), [[(p, 0, k), (p + 300, 3, 3)]], None))
    return out


def staged_rows(o, w, read_len, chain, seed):
    """(left, right): the target rows chain2aln_kernel stages for a seed's two sides, min(rLen, qLen + 2w + 2)"""
    r0, r1 = max_span(o, w, read_len, chain)
    rb, qb, ln = seed
    lq, rq = qb, read_len - qb - ln
    return (min(max(rb - r0, 0), lq + 2 * w + 2) if lq else 0), (min(max(r1 - rb - ln, 0), rq + 2 * w + 2) if rq else 0)


@functools.lru_cache(None)
def band():
    batches, wants = [], []
    for w in BAND_WS:
        b, want = _Batch(), []
        for read, chains, ww in _band_reads(w):
            want.append((b.add(read, chains), ww))
        batches.append((w, b.soa())); wants.append((b, want))

    def promise(oi, results, bwa=True):
        notes = []
        for (w, _), (b, want), (cnt, regs) in zip(batches, wants, results):
            rr = per_read(cnt, regs)
            if w == 254:
                rows = [max(staged_rows(OPTIONS[oi], w, len(rd), ch[0], ch[0][0])) for rd, ch in b.reads]
                _need(max(rows) == 765 and 764 in rows, f"band(w=254): staged rows {rows}, want 765 and 764")
                _need(all(g["w"].min() >= 254 for g in rr), "band(w=254): a region with w < 254")
                notes.append(f"w=254: staged rows up to {max(rows)}")
                continue
            if oi != 0 or not bwa:   # the gaps are sized for the default scoring, and the Scala z-drop parse ends a row walk 48 bases
                continue             # into a deletion: elsewhere the comparison alone counts
            wide = narrow = 0
            for r, ww in want:
                _need(len(rr[r]) == 1, f"band(w={w}) read {r}: {len(rr[r])} regions")
                got = int(rr[r][0]["w"])
                _need(ww is None or got == ww, f"band(w={w}) read {r}: w = {got}, want {ww}")
                wide += got == 2 * w; narrow += got == w
            _need(wide >= 2 and narrow >= 2, f"band(w={w}): {wide} regions at 2w and {narrow} at w")
            notes.append(f"w={w}: {wide} at 2w, {narrow} at w")
        return "; ".join(notes)
    return Family(batches, promise)


# ------------------------------------------------------------------------------------------------------------------ ends
@functools.lru_cache(None)
def ends():
    b, L = _Batch(), L_PAC
    pad = lambda n, v=1: np.full(n, v, np.uint8)
    bare_left, bare_right, inside = [], [], []          # reads whose left / right side has qLen > 0 and rLen == 0; all reads

    def add(read, seed, bl=False, br=False):
        r = b.add(read, [[seed]])
        inside.append(r)
        if bl:
            bare_left.append((r, seed))
        if br:
            bare_right.append((r, seed))

    add(win(0, 100), (0, 0, 30))                                                  # rbeg = 0, nothing on the left
    add(np.concatenate([pad(20), win(0, 80)]), (0, 20, 30), bl=True)              # rbeg = 0 with 20 read bases left of it: rLen == 0
    add(np.concatenate([pad(30, 2), win(5, 75)]), (5, 30, 20))                    # clipped at 0: rLen = 5 < qLen = 30
    add(win(L - 100, L), (L - 30, 70, 30))                                        # ends at l_pac
    add(np.concatenate([win(L - 70, L), pad(30)]), (L - 30, 40, 30), br=True)     # ends at l_pac, 30 read bases after it: rLen == 0
    add(win(L, L + 100), (L, 0, 30))                                              # starts at l_pac (reverse strand)
    add(np.concatenate([pad(20, 3), win(L, L + 80)]), (L, 20, 30), bl=True)       # starts at l_pac: the window is cropped there
    add(win(2 * L - 100, 2 * L), (2 * L - 30, 70, 30))                            # ends at 2 l_pac
    add(np.concatenate([win(2 * L - 70, 2 * L), pad(30, 0)]), (2 * L - 30, 40, 30), br=True)
    add(np.concatenate([win(2 * L - 60, 2 * L - 5), pad(45, 2)]), (2 * L - 25, 35, 20))   # clipped at 2 l_pac: rLen = 5 < qLen = 45
    add(np.concatenate([win(L - 80, L), pad(20)]), (L - 60, 20, 30))                                    # the span crosses l_pac, seed 0 forward
    add(np.concatenate([pad(20, 2), win(L, L + 80)]), (L + 20, 40, 30))                                    # ... seed 0 on the reverse strand
    # two seeds, the span crosses l_pac; seed 0 decides the side (the other seed is on the same strand, as the entry requires)
    b.add(win(L - 150, L - 50), [[(L - 140, 10, 25), (L - 90, 60, 30)]])
    b.add(win(L + 50, L + 150), [[(L + 60, 10, 25), (L + 110, 60, 30)]])

    def promise(oi, results, bwa=True):
        (cnt, regs), = results
        rr = per_read(cnt, regs)
        for g in rr:
            _need(len(g) >= 1 and g["rb"].min() >= 0 and g["re"].max() <= 2 * L, "ends: a region outside the reference")
            _need(all((x["rb"] < L) == (x["re"] <= L) for x in g), "ends: a region across l_pac")
        for r, (rb, qb, ln) in bare_left:       # no target on the left: SWExtend returns at once, the region starts at the seed
            _need(rr[r][0]["rb"] == rb and rr[r][0]["qb"] == qb, f"ends read {r}: extended to the left of an empty window")
        for r, (rb, qb, ln) in bare_right:
            _need(rr[r][0]["re"] == rb + ln and rr[r][0]["qe"] == qb + ln, f"ends read {r}: extended to the right of an empty window")
        o = OPTIONS[oi]
        short = 0
        for r in inside:
            rd, ch = b.reads[r]
            lrow, rrow = staged_rows(o, 100, len(rd), ch[0], ch[0][0])
            short += (0 < lrow < ch[0][0][1]) + (0 < rrow < len(rd) - ch[0][0][1] - ch[0][0][2])
        _need(short >= 2, "ends: no side with 0 < rLen < qLen")
        return f"{len(rr)} reads, {len(bare_left) + len(bare_right)} empty windows, {short} shorter than the flank"
    return Family([(100, b.soa())], promise)


# ----------------------------------------------------------------------------------------------------------------- bases
@functools.lru_cache(None)
def bases():
    b = _Batch()
    p = 12_000
    clean = win(p, p + 120)
    seed = (p + 50, 50, 25)
    twins = []
    for at in ([0], [119], [0, 119], [49], [75], [49, 75], [20, 21, 22], [100, 110], list(range(0, 50, 7)) + list(range(80, 120, 9))):
        rd = clean.copy()
        rd[at] = 4
        twins.append(b.add(rd, [[seed]]))
    r_clean = b.add(clean, [[seed]])
    r_one = b.add(win(p + 7, p + 8), [[(p + 7, 0, 1)]])            # a 1-base read with a 1-base seed
    r_whole = b.add(win(p, p + 77), [[(p, 0, 77)]])                # a seed spanning the whole read
    r_none = b.add(win(p, p + 50), [])                             # a read with no chain
    r_n_all = b.add(np.full(60, 4, np.uint8), [[(p, 20, 19)]])     # nothing but N around a (dishonest) seed

    def promise(oi, results, bwa=True):
        (cnt, regs), = results
        rr = per_read(cnt, regs)
        o = OPTIONS[oi]
        _need(cnt[r_none] == 0 and cnt[r_one] == 1 and cnt[r_whole] == 1, "bases: counts of the degenerate reads")
        _need(tuple(rr[r_one][0][["qb", "qe", "score"]]) == (0, 1, o.a) and rr[r_whole][0]["score"] == 77 * o.a, "bases: degenerate regions")
        _need(all(rr[t][0]["truesc"] < rr[r_clean][0]["truesc"] for t in twins), "bases: an N that costs nothing")
        _need(tuple(rr[r_n_all][0][["qb", "qe"]]) == (20, 39), "bases: extended into N")
        return f"{len(rr)} reads, {len(twins)} with N"
    return Family([(100, b.soa())], promise)


# --------------------------------------------------------------------------------------------------------------- requeue
RQ_EVERY = 97
RQ_HEAVY = (("rc", 65), ("sl", (200, "fan", "equal")), ("rc", 90), ("sl", (129, "one", "runs")))


@functools.lru_cache(None)
def requeue(resident_waves, reduced=False):
    """3 * resident_waves + 5 reads, so that every wave of the capped launch takes a second and a third read.  Light reads are
    30-40 bases cut at A + o (o < 100) with one 19-base seed at query 5: had the wave's previous read been a heavy one
    (region_cache / seed_lanes reads, every 97th) and its region count or LDS region cache survived, the seed would be
    "contained" in that read's whole-read region at A and skipped.  reduced: the heavy reads and their two neighbours only."""
    n = 3 * resident_waves + 5
    b, kinds = _Batch(), []
    heavy = 0
    for j in range(n):
        is_heavy = j % RQ_EVERY == 48
        if reduced and not (is_heavy or (j - 1) % RQ_EVERY == 48 or (j + 1) % RQ_EVERY == 48):
            heavy += is_heavy
            continue
        if is_heavy:
            kind, arg = RQ_HEAVY[heavy % len(RQ_HEAVY)]
            heavy += 1
            b.add(*(region_cache_read(arg) if kind == "rc" else seed_lanes_read(*arg)))
            kinds.append((kind, arg))
        else:
            o, ln = (j * 13) % 100, 30 + j % 11
            b.add(win(A + o, A + o + ln), [[(A + o + 5, 5, 19)]])
            kinds.append(None)

    def promise(oi, results, bwa=True):
        (cnt, regs), = results
        rr = per_read(cnt, regs)
        nh = 0
        for k, g in zip(kinds, rr):
            if k is None:
                _need(len(g) == 1, f"requeue: a light read with {len(g)} regions")
            elif k[0] == "rc":
                _rc_promise(k[1], g); nh += 1
            else:
                _need(len(g) == 3 if k[1][1] == "one" else len(g) > RCAP, f"requeue: heavy {k} has {len(g)} regions"); nh += 1
        _need(nh >= 2 and (reduced or len(rr) == n), "requeue: heavy reads missing")
        return f"{len(rr)} reads, {nh} heavy"
    return Family([(100, b.soa())], promise)


RQ_CPU_WAVES = 1024      # the size the CPU comparison and the fixture reduce requeue from (3 077 reads, 32 heavy)

GROUPS = {
    "region_cache": region_cache,
    "seed_lanes": seed_lanes,
    "overlap": overlap,
    "band": band,
    "ends": ends,
    "bases": bases,
    "requeue": lambda: requeue(RQ_CPU_WAVES, True),     # the GPU test calls requeue(resident waves of its device) instead
}

FIXTURE_OPTIONS = (0, 1)


def fixture_batches():
    """[(family, w, ChainBatchSoA)] of tests/golden/mem_chain2aln_edges.npz; requeue reduced from 256 resident waves"""
    out = []
    for name, make in GROUPS.items():
        fam = requeue(256, True) if name == "requeue" else make()
        out += [(name, w, batch) for w, batch in fam.batches]
    return out


def fixture_options(z, oi):
    """option set oi of the fixture as an Options (the fixture carries its own numbers)"""
    ints = [int(x) for x in z[f"opt{oi}_ints"]]
    return Options(str(z[f"opt{oi}_name"]), *ints, np.asarray(z[f"opt{oi}_mat"], np.int8))


def fixture_batch(z, i):
    """(family, w, ChainBatchSoA) number i of the fixture"""
    cp = lambda k: np.ascontiguousarray(z[f"b{i}_{k}"])
    return str(z[f"b{i}_family"]), int(z[f"b{i}_w"]), ChainBatchSoA(
        l_pac=int(z["l_pac"]), read_len=cp("read_len"), read_off=cp("read_off"), read_pool=cp("read_pool"), chain_cnt=cp("chain_cnt"),
        seed_cnt=cp("seed_cnt"), seed_rbeg=cp("seed_rbeg"), seed_qbeg=cp("seed_qbeg"), seed_len=cp("seed_len"))


# ------------------------------------------------------------------------------------------------------------------ w = 1
@functools.lru_cache(None)
def w1_single():
    """(batch, seeds per read): reads whose chains all hold ONE seed, for the band width at which the reference C and the Scala
    disagree about `w`: 90 and 130 decoy chains on a 250-base read, and short honest reads whose first base left of
    the seed is wrong / right (left score unchanged / changed at the first try)"""
    b, seeds = _Batch(), []

    def add(read, chains):
        b.add(read, chains); seeds.append([ch[0] for ch in chains])

    for n in (90, 130):
        add(win(A, A + 250), [_decoy(i) for i in range(n)])
    p = 12_400
    for k in range(40):
        rd = win(p + 3 * k, p + 3 * k + 60).copy()
        qb = (0, 1, 9, 20)[k % 4]
        if k % 3 == 0 and qb:
            rd[qb - 1] = (rd[qb - 1] + 1) & 3
        if k % 5 == 0:
            rd[qb + 25] = (rd[qb + 25] + 2) & 3
        add(rd, [[(p + 3 * k + qb, qb, 25 if k % 7 else 60 - qb)]])
    return b.soa(), seeds
