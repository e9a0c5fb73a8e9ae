"""Hand-built mate-rescue groups for the host layer of boundary 1 (csrc/bpsw_rescue.cpp, and the rules it shares with the JNI shim and
worker2's prepare step in csrc/bpsw_rescue_core.h): the plan (fast path, lean speculation), the replay and the output assembly, at the
pairs those shortcuts name.  numpy only: no GPU, no library.  The models at the end of this file (infer_dir, first_round_jobs) are
statements of their own and stay so: they are what the header is held to (tests/test_rescue_core_host.py).

A pair is a dict
    reads: [end 0, end 1]           uint8 codes 0..4
    hits:  [[(rb, re, qb, qe, score), ...], [...]]   per end, best first (doubled coordinates)
    win:   {(end, anchor, r): (rb, re) | (rb, re, bytes)}   optional overrides of single windows
and `build` lays a list of them out as a RescueGroupSoA.

THE CONTRACT ON ref_cnt.  build fills ref_cnt[e] = min(#anchors of e, max_matesw), the anchors being the hits of e with
score >= best - pen_unpaired, as memSamPeGroupJNIPrepare does (MemSamPe.scala:1931-1990), and writes four window rows per counted
anchor.  The oracle indexes the window rows of anchor j of end e as (rows before e) + j for j < min(#anchors, max_matesw) and does
not clamp to ref_cnt: a group built with other options than it is run with is outside the contract.  So a case's option overrides
go to build AND to the call (CASES[name] = (group, opt_overrides, what_it_claims)).

Windows follow getAlnRegRefJNI (synth.rescue_window) and are cut from one small random reference (L_PAC bases, synth.random_pac), so
every group can be submitted with window bytes or, after ref_load(PAC, L_PAC), with coordinates only (ref_pool = ref_len = ref_off =
None) -- except where a window is given as explicit bytes.

what_it_claims (checked against the oracle alone in tests/test_rescue_cases.py):
    changed       pairs whose lists differ from the input (both flavours)
    count_unchanged / kept   the region counts stay as they were / hashes of input regions that must still be there
    touched, inside          B: the pair's walk runs an SW at all / its one distance lies inside the limits of its orientation
    n_sw          SW calls of the sequential walk
    killed        hashes of input regions that must be gone from the output
    rb_eq_re      regions with rb == re in the Scala flavour (its non-reversed branch, MemSamPe.scala:1203-1204); none in C
    second_round  the lean plan's first round cannot hold every job of the walk
    windows       minimum numbers of bridging / clamped0 / clamped2l / empty window rows in the group
    zero_len      a mate of length 0 is in the group: the oracle counts an SW call the library never makes; never sent to the
                  reference build
"""
import numpy as np

from bpsw_hip import ALNREG_DTYPE, RescueGroupSoA, synth

L_PAC = 20_011
L2 = 2 * L_PAC
PAC, BASES = synth.random_pac(L_PAC, seed=0x5E5C)
L = 150
LOW, HIGH = 200, 600
FAILED = (0, 0, 1, 0.0, 0.0)
PES_FR = [FAILED, (LOW, HIGH, 0, 400.0, 50.0), FAILED, FAILED]
# four live orientations, every limit different
PES_ALL = [(200, 600, 0, 400.0, 50.0), (210, 640, 0, 425.0, 54.0), (150, 550, 0, 350.0, 50.0), (230, 590, 0, 410.0, 45.0)]
PES_NONE = [FAILED] * 4
# a library so tight that two bases decide: only here can a rescued hit land outside the range its locus's old hit was inside (see I)
PES_NARROW = [FAILED, (399, 400, 0, 399.5, 0.25), FAILED, FAILED]
NO_RESCUE = 0x20


def dbl(rb, re):
    """bases [rb, re) of the doubled reference (empty when the range bridges the strands)"""
    return synth.window_bases(BASES, L_PAC, rb, re)


def revcomp(a):
    r = np.asarray(a, np.uint8)[::-1]
    return np.where(r < 4, 3 - r, 4).astype(np.uint8)


def read_at(b, n=L):
    """the read that aligns at doubled position b; where no such read exists (outside the reference, across the strands) random bases"""
    if b >= 0 and b + n <= L2:
        w = dbl(b, b + n)
        if len(w) == n:
            return w
    return np.random.default_rng(0xA000 + (int(b) & 0xFFFFF)).integers(0, 4, n).astype(np.uint8)


def junk(seed, n=L):
    return np.random.default_rng(0xB000 + seed).integers(0, 4, n).astype(np.uint8)


def full(b, score=None, n=L):
    return (b, b + n, 0, n, n if score is None else score)


def mate_rb(a_rb, r, d):
    """start of the hit that mem_infer_dir (native/bwamem_pair.c:27-34) sees in orientation r at distance d from a hit starting at a_rb"""
    if r == 0:
        return a_rb + d
    if r == 3:
        return a_rb - d
    if r == 1:
        return L2 - 1 - (a_rb + d)
    return L2 - 1 - (a_rb - d)


def infer_dir(b1, b2, l_pac=L_PAC):
    r1, r2 = b1 >= l_pac, b2 >= l_pac
    p2 = b2 if r1 == r2 else 2 * l_pac - 1 - b2
    return (0 if r1 == r2 else 1) ^ (0 if p2 > b1 else 3), abs(p2 - b1)


def build(pairs, pes, max_matesw=100, pen_unpaired=17, l_pac=L_PAC, bases=BASES, **_):
    """pairs -> RescueGroupSoA; see the module docstring for the contract on ref_cnt.  Input hashes are 1 << 40 | pair << 8 | end << 7 | rank."""
    seq_len, seq_off, seq_chunks, seq_at = [], [], [], 0
    reg_cnt, regs, ref_cnt = [], [], []
    ref_rb, ref_re, ref_len, ref_off, ref_chunks, ref_at = [], [], [], [], [], 0
    for k, p in enumerate(pairs):
        for i in range(2):
            s = np.asarray(p["reads"][i], np.uint8)
            seq_len.append(len(s)); seq_off.append(seq_at); seq_chunks.append(s)
            pad = (-len(s)) % 16
            seq_chunks.append(np.zeros(pad, np.uint8))
            seq_at += len(s) + pad
        for i in range(2):
            hl = p["hits"][i]
            assert all(hl[j][4] >= hl[j + 1][4] for j in range(len(hl) - 1)), "hits go best first"
            reg_cnt.append(len(hl))
            for j, (rb, re, qb, qe, score) in enumerate(hl):
                regs.append((rb, re, qb, qe, score, score, 0, 0, 0, 100, (qe - qb) // 2, -1, (1 << 40) | (k << 8) | (i << 7) | j))
            anchors = [h for h in hl if h[4] >= hl[0][4] - pen_unpaired][:max(max_matesw, 0)] if hl else []
            ref_cnt.append(len(anchors))
            mate_len = len(p["reads"][1 - i])
            for j, a in enumerate(anchors):
                for r in range(4):
                    w = p.get("win", {}).get((i, j, r))
                    if w is None:
                        w = synth.rescue_window(pes, l_pac, a[0], r, mate_len)
                    rb, re = int(w[0]), int(w[1])
                    if len(w) == 3:
                        by = np.asarray(w[2], np.uint8)
                    elif rb < 0 and re < 0:
                        by = None
                    else:
                        by = synth.window_bases(bases, l_pac, rb, re)
                    if by is None:
                        ref_rb.append(-1); ref_re.append(-1); ref_len.append(0); ref_off.append(0)
                        continue
                    ref_rb.append(rb); ref_re.append(re); ref_len.append(len(by)); ref_off.append(ref_at)
                    ref_chunks.append(by)
                    pad = (-len(by)) % 16
                    ref_chunks.append(np.zeros(pad, np.uint8))
                    ref_at += len(by) + pad
    cat = lambda ch: np.concatenate(ch + [np.zeros(16, np.uint8)])
    return RescueGroupSoA(group_size=len(pairs), l_pac=l_pac, pes=[tuple(x) for x in pes], seq_len=np.array(seq_len, np.int32),
                          seq_off=np.array(seq_off, np.int64), seq_pool=cat(seq_chunks), reg_cnt=np.array(reg_cnt, np.int32),
                          regs=np.array(regs, dtype=ALNREG_DTYPE) if regs else np.zeros(0, ALNREG_DTYPE),
                          ref_cnt=np.array(ref_cnt, np.int32), ref_rb=np.array(ref_rb, np.int64), ref_re=np.array(ref_re, np.int64),
                          ref_len=np.array(ref_len, np.int64), ref_off=np.array(ref_off, np.int64), ref_pool=cat(ref_chunks))


def as_coords(g):
    """the same group with its windows named by coordinates only (the reference must be loaded: ctx.ref_load(PAC, L_PAC))"""
    import dataclasses
    return dataclasses.replace(g, ref_pool=None, ref_len=None, ref_off=None)


def in_hash(k, i, j):
    return (1 << 40) | (k << 8) | (i << 7) | j


# CASES[name] = (group, opt_overrides, what_it_claims); SPECS[name] = (pairs, pes) for the tests that rebuild parts of a group
CASES, SPECS = {}, {}


def case(name, pairs, pes, claims, **opt):
    assert name not in CASES
    SPECS[name] = (pairs, pes)
    CASES[name] = (build(pairs, pes, **opt), opt, claims)


def pair(r0, r1, h0=(), h1=(), win=None):
    return dict(reads=[r0, r1], hits=[list(h0), list(h1)], win=win or {})


# --- the standard pair: an anchor on one end, the mate where orientation r puts it --------------------------------------------------
def rescue_pair(a_rb, r, rescued_end, pes, off=100, a_score=L, mate_hits=(), mate_len=L, extra_anchor_hits=()):
    """anchor (a full hit at a_rb) on end 1 - rescued_end; the other end's read is cut `off` bases into window r of that anchor, so the
    rescue in orientation r finds it whole"""
    wb, we = synth.rescue_window(pes, L_PAC, a_rb, r, mate_len)
    m = wb + off
    assert wb <= m and m + mate_len <= we and len(dbl(m, m + mate_len)) == mate_len
    is_rev = (r >> 1) != (r & 1)
    mate = revcomp(dbl(m, m + mate_len)) if is_rev else dbl(m, m + mate_len)
    reads, hits = [None, None], [None, None]
    reads[1 - rescued_end], hits[1 - rescued_end] = read_at(a_rb), [full(a_rb, a_score)] + list(extra_anchor_hits)
    reads[rescued_end], hits[rescued_end] = mate, list(mate_hits)
    hits[1 - rescued_end].sort(key=lambda h: -h[4])
    return dict(reads=reads, hits=hits, win={})


A_F, A_R = 5000, L_PAC + 5000   # an anchor on the forward strand and one on the reverse strand, far from every end
FAR = 15000                     # an unrelated locus (forward); L_PAC + FAR on the reverse strand


# === A. options =====================================================================================================================
def _a_pairs():
    decoys0 = rescue_pair(A_F, 1, 1, PES_FR, extra_anchor_hits=[full(FAR, 160), full(FAR - 1500, 158)])      # end 0: decoy, decoy, true
    decoys1 = rescue_pair(A_R, 1, 0, PES_FR, extra_anchor_hits=[full(L_PAC + FAR, 160), full(L_PAC + FAR - 1500, 158)])
    both = pair(read_at(A_F + 1000), read_at(L_PAC + 9000),
                [full(A_F + 1000), full(A_F + 1001, 148), full(A_F + 1003, 146)],
                [full(L_PAC + 9000), full(L_PAC + 9002, 149), full(L_PAC + 9003, 147)])                          # three anchors per end, unpaired
    return [decoys0, decoys1, both]


# (pair 2 changes as soon as one SW ran for it: the dedup that follows removes its near-duplicate hits)
for _m, _claims in ((0, dict(changed=[], n_sw=0, second_round=False)),
                    (1, dict(changed=[2], n_sw=4, second_round=False)),
                    (2, dict(changed=[2], n_sw=8, second_round=True))):
    case(f"A_max_matesw_{_m}", _a_pairs(), PES_FR, _claims, max_matesw=_m)
# without the limit the third anchor of the decoy pairs finds the mate
case("A_max_matesw_default", _a_pairs(), PES_FR, dict(changed=[0, 1, 2], n_sw=12, second_round=True))
# pen_unpaired 0: the two hits of the best score are anchors (a decoy and the true one), the one a point lower is not
case("A_pen_unpaired_0", [rescue_pair(A_F, 1, 1, PES_FR, extra_anchor_hits=[full(FAR, 150), full(A_F + 3, 149)]),
                          rescue_pair(A_R, 1, 0, PES_FR, a_score=149, extra_anchor_hits=[full(L_PAC + FAR, 150)])], PES_FR,
     dict(changed=[0], n_sw=3, second_round=True), pen_unpaired=0)
# pen_unpaired 3: 150 (decoy) and 148 (true) are anchors, 146 is not; in the second pair the true hit is 4 below the decoy
case("A_pen_unpaired_3", [rescue_pair(A_F, 1, 1, PES_FR, a_score=148, extra_anchor_hits=[full(FAR, 150), full(FAR + 2000, 146)]),
                          rescue_pair(A_R, 1, 0, PES_FR, a_score=146, extra_anchor_hits=[full(L_PAC + FAR, 150)])], PES_FR,
     dict(changed=[0], n_sw=3, second_round=True), pen_unpaired=3)
# pen_unpaired -1: no hit passes its own threshold (score >= best + 1): no anchors, and the fast path must not decide for one-hit pairs
case("A_pen_unpaired_minus1", [rescue_pair(A_F, 1, 1, PES_FR), pair(read_at(A_F), read_at(mate_rb(A_F, 1, 300)), [full(A_F)], [full(mate_rb(A_F, 1, 300))]),
                               pair(read_at(A_F), read_at(mate_rb(A_F, 1, 700)), [full(A_F)], [full(mate_rb(A_F, 1, 700))])], PES_FR,
     dict(changed=[], n_sw=0, second_round=False), pen_unpaired=-1)
case("A_no_rescue_flag", [rescue_pair(A_F, 1, 1, PES_FR), rescue_pair(A_R, 1, 0, PES_FR, extra_anchor_hits=[full(L_PAC + FAR, 160)])], PES_FR,
     dict(changed=[], n_sw=0, second_round=False), flag=NO_RESCUE, max_matesw=1)


# === B. distances on the limits: the straight-line path against the general walk ====================================================
# B_TABLE rows: (name of the one-pair fast case, name of its general-walk twin, pes name, r, label of the distance, must be touched)
B_TABLE = []


def _b_cases():
    for pes_name, pes in (("fr", PES_FR), ("all", PES_ALL)):
        for r in range(4):
            a_rb = A_R if r in (1, 3) else A_F          # anchors on either strand
            lo, hi = (pes[r][0], pes[r][1]) if not pes[r][2] else (LOW, HIGH)
            for label, d in (("low-1", lo - 1), ("low", lo), ("high", hi), ("high+1", hi + 1)):
                b2 = mate_rb(a_rb, r, d)
                assert infer_dir(a_rb, b2) == (r, d) and infer_dir(b2, a_rb)[1] == d
                fast = pair(read_at(a_rb), read_at(b2), [full(a_rb)], [full(b2)])
                # the twin: a second hit far below the threshold on one end, nowhere near a proper distance (rc != 1: the general walk)
                weak_end = (r + (label in ("low", "high+1"))) & 1
                weak = (FAR + 2500 if weak_end == 0 else L_PAC + 500, 0, 10, 60, 40)
                weak = (weak[0], weak[0] + 50) + weak[2:]
                walk = pair(read_at(a_rb), read_at(b2), [full(a_rb)] + ([weak] if weak_end == 0 else []), [full(b2)] + ([weak] if weak_end == 1 else []))
                # every orientation skipped on both sides <=> nothing to do: the orientation seen must be live and the distance inside;
                # with four live orientations three others still want a job
                inside = lo <= d <= hi and not pes[r][2]
                touched = not (inside and pes_name == "fr")
                n1, n2 = f"B_{pes_name}_r{r}_{label}_fast", f"B_{pes_name}_r{r}_{label}_walk"
                case(n1, [fast], pes, dict(touched=touched, inside=inside, second_round=False))
                case(n2, [walk], pes, dict(touched=touched, inside=inside, second_round=False))
                B_TABLE.append((n1, n2, pes_name, r, label, touched))
    none = pair(read_at(A_F), read_at(mate_rb(A_F, 1, 900)), [full(A_F)], [full(mate_rb(A_F, 1, 900))])
    case("B_all_four_failed", [none, rescue_pair(A_F, 1, 1, PES_ALL)], PES_NONE, dict(changed=[], n_sw=0, second_round=False))


_b_cases()


# === C. the ends of the coordinate space ============================================================================================
def _c_pairs():
    out = []
    for a_rb in (0, L_PAC - L, L_PAC - 1, L_PAC, L2 - L):
        # the mate is cut from where an FR pair of insert 400 has it when that lies inside the reference, else random bases
        m = a_rb + 250
        mate = revcomp(dbl(m, m + L)) if len(dbl(m, m + L)) == L else junk(a_rb & 0xFFF)
        out.append(pair(read_at(a_rb), mate, [full(a_rb)], []))
        out.append(pair(mate, read_at(a_rb), [], [full(a_rb)]))
    return out


case("C_edges_all_orientations", _c_pairs(), PES_ALL,
     dict(n_sw=32, windows=dict(bridging=2, clamped0=4, clamped2l=4), second_round=False))
case("C_edges_fr", _c_pairs(), PES_FR, dict(n_sw=8, windows=dict(bridging=2, clamped2l=2, failed_rows=30), second_round=False))
# a window with rb == re == 2 l_pac is a valid window of no rows: the job runs and finds nothing, yet the mate's list is still sorted and
# de-duplicated because an SW ran (n > 0): the partial hit under the full one goes
_c_empty = pair(read_at(L2 - L), read_at(FAR), [full(L2 - L)], [full(FAR), (FAR, FAR + 75, 0, 75, 75)],
                win={(0, 0, 1): (L2, L2)})
case("C_empty_window_at_2l", [_c_empty], PES_FR,
     dict(changed=[0], n_sw=2, killed=[in_hash(0, 1, 1)], windows=dict(empty=1), second_round=False))


# === D. a rescue that succeeds in each orientation ==================================================================================
# D_ORDER[k] = (r, anchor on the reverse strand, rescued end) of pair k
D_ORDER = [(r, rev, e) for r in range(4) for rev in (0, 1) for e in (1, 0)]
case("D_each_orientation", [rescue_pair(A_R if rev else A_F, r, e, PES_ALL) for r, rev, e in D_ORDER], PES_ALL,
     dict(changed=list(range(16)), rb_eq_re=8, second_round=False))
# The Scala flavour's rescued region (rb, re, qb, qe, score, seedcov) per (r, anchor strand), by hand from MemSamPe.scala:1192-1212.
# The mate lies whole, without a mismatch, 100 bases into window r = (wb, we) of the anchor at A = 5000 (forward) or L_PAC + 5000 = 25011
# (reverse), so SWAlign2 returns score 150, (tb, te) = (100, 249), (qb, qe) = (0, 149); 2 l_pac = 40022.
#   r = 0 (not reversed): wb = A + 200;        rb = re = wb + te + 1 = wb + 250 (Scala keeps no start: seedcov = min(0, 150) >> 1 = 0)
#   r = 3 (not reversed): wb = A - 590;        rb = re = wb + 250
#   r = 1 (reversed):     wb = A + 210 - 150;  rb = 40022 - (wb + 250), re = 40022 - (wb + 100); q = (150 - 150, 150 - 0); seedcov 75
#   r = 2 (reversed):     wb = A - 550 - 150;  rb = 40022 - (wb + 250), re = 40022 - (wb + 100)
D_SCALA = {
    (0, 0): (5450, 5450, 0, 150, 150, 0), (0, 1): (25461, 25461, 0, 150, 150, 0),
    (1, 0): (34712, 34862, 0, 150, 150, 75), (1, 1): (14701, 14851, 0, 150, 150, 75),
    (2, 0): (35472, 35622, 0, 150, 150, 75), (2, 1): (15461, 15611, 0, 150, 150, 75),
    (3, 0): (4660, 4660, 0, 150, 150, 0), (3, 1): (24671, 24671, 0, 150, 150, 0),
}
# (the C flavour keeps the start: native/bwamem_pair.c:206-207; the reversed ones are the same in both)
D_C = {k: ((v[0] - 150, v[1], 0, 150, 150, 75) if k[0] in (0, 3) else v) for k, v in D_SCALA.items()}


# === E. what the rescue does to the mate's list =====================================================================================
# A mate lying whole at the left edge of the FR window of the anchor at A (forward locus [A + LOW - L, A + LOW)) is seen at distance
# LOW - 1: one short of proper, so a hit of the mate's own at that locus does not stop the rescue.
def _edge_pair(a_rb, mate_hits, mutate=(), anchor_hits=None, rescued_end=1):
    p = rescue_pair(a_rb, 1, rescued_end, PES_FR, off=0, mate_hits=mate_hits)
    for q in mutate:
        p["reads"][rescued_end][q] = (p["reads"][rescued_end][q] + 1) & 3
    if anchor_hits is not None:
        p["hits"][1 - rescued_end] = anchor_hits
    return p


_E_RB = L2 - (A_F + LOW)          # where the mate of _edge_pair(A_F, ...) starts on the reverse strand
assert infer_dir(A_F, _E_RB) == (1, LOW - 1)
case("E_supersedes_partial", [_edge_pair(A_F, [(_E_RB, _E_RB + 75, 0, 75, 75)])], PES_FR,
     dict(changed=[0], n_sw=2, killed=[in_hash(0, 1, 0)], second_round=False))
# three mismatches in the read: the SW scores 135 at the locus where the list already has a hit of 150: the new hit goes, the old one and
# the count stay.  (The mate's hit is an anchor too and rescues end 0's read onto end 0's own hit: equal in score, rb and qb.)
case("E_worse_than_existing", [_edge_pair(A_F, [full(_E_RB)], mutate=(40, 75, 110))], PES_FR,
     dict(count_unchanged=True, kept=[in_hash(0, 1, 0)], n_sw=2, second_round=False))
case("E_equals_existing", [_edge_pair(A_F, [full(_E_RB)])], PES_FR, dict(count_unchanged=True, n_sw=2, second_round=False))
# three hits of one score, given in falling rb: the rescue (which finds the mate) re-sorts them
case("E_three_equal_scores", [rescue_pair(A_F, 1, 1, PES_FR, mate_hits=[full(L_PAC + 12000, 90), full(L_PAC + 11000, 90), full(L_PAC + 10000, 90)])],
     PES_FR, dict(changed=[0], n_sw=4, second_round=True))   # (the three are anchors too; only the first one's job is in the first round)
# two anchors two bases apart: the first one's rescue puts the mate at a proper distance of the second, which is then skipped
case("E_near_duplicate_anchors", [rescue_pair(A_F, 1, 1, PES_FR, extra_anchor_hits=[full(A_F + 2, 148)]),
                                  rescue_pair(A_R, 1, 0, PES_FR, extra_anchor_hits=[full(A_R + 3, 140)])], PES_FR,
     dict(changed=[0, 1], n_sw=2, second_round=False))
# a decoy anchor in front of the true one: its rescue finds nothing, the true anchor's job is wanted in a second round
case("E_decoy_first", [rescue_pair(A_F, 1, 1, PES_FR, extra_anchor_hits=[full(FAR, 155)]),
                       rescue_pair(A_R, 1, 0, PES_FR, extra_anchor_hits=[full(L_PAC + FAR, 151)])], PES_FR,
     dict(changed=[0, 1], n_sw=4, second_round=True))


# === F. mates =======================================================================================================================
_empty = np.zeros(0, np.uint8)
case("F_len0_no_hits", [pair(read_at(A_F), _empty, [full(A_F)], []), pair(_empty, read_at(A_R), [], [full(A_R)])], PES_FR,
     dict(changed=[], n_sw=2, zero_len=True, second_round=False))
case("F_len0_one_hit", [pair(read_at(A_F), _empty, [full(A_F)], [(L_PAC + FAR, L_PAC + FAR + 30, 0, 30, 30)])], PES_FR,
     dict(changed=[], n_sw=2, zero_len=True, second_round=False))   # (the mate's own hit is an anchor and looks for end 0's read)
# around min_seed_len = 19: a mate of 18 bases cannot score 19
case("F_len18_19", [rescue_pair(A_F, 1, 1, PES_FR, mate_len=18), rescue_pair(A_F, 1, 1, PES_FR, mate_len=19),
                    rescue_pair(A_R, 1, 0, PES_FR, mate_len=18), rescue_pair(A_R, 1, 0, PES_FR, mate_len=19)], PES_FR,
     dict(changed=[1, 3], n_sw=4, second_round=False))


def _f_mixed():
    short_anchor = rescue_pair(A_F, 1, 1, PES_FR)
    short_anchor["reads"][0], short_anchor["hits"][0] = read_at(A_F, 50), [full(A_F, n=50)]    # a 50-base anchor rescues a 150-base mate
    short_mate = rescue_pair(A_R, 1, 0, PES_FR, mate_len=50)                                   # ... and a 150-base anchor a 50-base mate
    with_n = rescue_pair(A_F + 700, 1, 1, PES_FR)
    with_n["reads"][1][[0, 1, 74, 75, 76, 148, 149]] = 4                                       # N at both ends and in the middle
    long_pair = rescue_pair(A_F + 2000, 1, 1, PES_FR, mate_len=250)                            # a 250-base pair among the 150-base ones
    long_pair["reads"][0], long_pair["hits"][0] = read_at(A_F + 2000, 250), [full(A_F + 2000, n=250)]
    return [short_anchor, short_mate, with_n, long_pair, rescue_pair(A_R + 900, 1, 0, PES_FR)]


case("F_mixed_lengths", _f_mixed(), PES_FR, dict(changed=[0, 1, 2, 3, 4], n_sw=5, second_round=False))


# === G. output assembly =============================================================================================================
# four pairs that need a job (their two ends hold different numbers of regions) and four that do not, separated by pairs without regions
def _g_pool():
    t = [rescue_pair(A_F, 1, 1, PES_FR),                                                        # 1 / 0 -> 1 / 1
         rescue_pair(A_R, 1, 0, PES_FR),                                                        # 0 / 1 -> 1 / 1
         _edge_pair(A_F + 800, [(L2 - (A_F + 800 + LOW), L2 - (A_F + 800 + LOW) + 75, 0, 75, 75), (L_PAC + FAR, L_PAC + FAR + 40, 0, 40, 40)]),   # 1 / 2 -> 1 / 2
         rescue_pair(A_F + 1600, 1, 1, PES_FR, extra_anchor_hits=[full(FAR, 155), full(FAR + 900, 100)])]   # 3 / 0 -> 3 / 1, second round
    b = mate_rb(A_F + 3000, 1, 380)
    weak0, weak1 = (FAR + 2500, FAR + 2550, 10, 60, 40), (L_PAC + 500, L_PAC + 550, 10, 60, 40)
    u = [pair(read_at(A_F + 3000), read_at(b), [full(A_F + 3000)], [full(b)]),                  # the straight-line path
         pair(read_at(A_F + 3000), read_at(b), [full(A_F + 3000), weak0], [full(b)]),           # 2 / 1
         pair(read_at(A_F + 3000), read_at(b), [full(A_F + 3000)], [full(b), weak1]),           # 1 / 2
         pair(read_at(A_R), read_at(mate_rb(A_R, 1, LOW)), [full(A_R)], [full(mate_rb(A_R, 1, LOW))])]
    e = pair(junk(1), junk(2), [], [])
    return t, u, e


def _g_arrange(order):
    t, u, e = _g_pool()
    it = {"T": iter(t), "U": iter(u)}
    return [dict(e) if c == "E" else next(it[c]) for c in order]


G_ORDERS = {"G_mixed": "TTEUUETEUUT", "G_all_touched": "TETTT", "G_none_touched": "UEUUU", "G_touched_inside": "UETUTTEUTU"}
for _n, _o in G_ORDERS.items():
    case(_n, _g_arrange(_o), PES_FR,
         dict(changed=[i for i, c in enumerate(_o) if c == "T"], second_round=_o.count("T") == 4))


# === I. a boundary-biased random generator ==========================================================================================
I_PES = {1: PES_NARROW, 2: PES_ALL, 3: PES_FR, 4: PES_FR, 5: PES_ALL, 6: PES_NARROW}   # each table meets a max_matesw above 1


def generate(seed, n_pairs=64):
    """pairs, pes and options: each distance from {low-1, low, high, high+1} half of the time, anchors 1 to 3 bases apart, partial mate
    hits at the true locus, one position in eight within L of an end of the doubled reference or of l_pac"""
    rng = np.random.default_rng(0x1E5C0000 + seed)
    pes = I_PES[seed] if seed in I_PES else (PES_NARROW, PES_ALL, PES_FR)[seed % 3]
    opt = dict(max_matesw=int(rng.choice([1, 2, 100])), pen_unpaired=int(rng.choice([0, 3, 17])))
    live = [r for r in range(4) if not pes[r][2]]
    pairs = []
    for _ in range(n_pairs):
        if rng.random() < 0.125:
            a_rb = int(rng.choice([0, L_PAC - L, L_PAC, L2 - L]) + rng.integers(-L, L + 1))
            a_rb = min(max(a_rb, 0), L2 - L)
        else:
            a_rb = int(rng.integers(0, L2 - L))
        r = int(rng.choice(live))
        lo, hi = pes[r][0], pes[r][1]
        d = int(rng.choice([lo - 1, lo, hi, hi + 1])) if rng.random() < 0.5 else int(rng.integers(lo, hi + 1))
        b2 = mate_rb(a_rb, r, d)
        a_end = int(rng.integers(0, 2))
        anchors = [full(a_rb, 150 - int(rng.integers(0, 4)))]
        if rng.random() < 0.25 and L <= a_rb <= L2 - 2 * L:
            # the setting in which a dedup can remove the hit that justified a skip: the mate's own hit is a partial one that sits exactly on
            # a limit as the SECOND anchor sees it, and one base outside as the first anchor, a base away, sees it
            on, step = (lo, 1) if rng.random() < 0.5 else (hi, -1)
            if r in (2, 3):
                step = -step                          # there the distance grows with the anchor's start
            half = int(rng.integers(0, 2)) * 75
            b2 = mate_rb(a_rb, r, on) - half          # the partial hit starts `half` bases into the mate's full alignment at b2
            ok = 0 <= b2 <= L2 - L and len(dbl(b2, b2 + L)) == L
            if ok:
                anchors = [full(a_rb + step, 150), full(a_rb, 150 - int(rng.integers(0, 3)))]
                reads, hits = [None, None], [None, None]
                reads[a_end], hits[a_end] = read_at(a_rb + step), anchors
                reads[1 - a_end], hits[1 - a_end] = read_at(b2), [(b2 + half, b2 + half + 75, half, half + 75, 75 - int(rng.integers(0, 6)))]
                pairs.append(dict(reads=reads, hits=hits, win={}))
                continue
        for _x in range(int(rng.integers(0, 3))):       # near-duplicates 1 to 3 bases further on
            prev = anchors[-1]
            anchors.append(full(min(prev[0] + int(rng.integers(1, 4)), L2 - L), prev[4] - int(rng.integers(0, 5))))
        if rng.random() < 0.2:                          # a decoy in front
            anchors.insert(0, full(int(rng.integers(0, L2 - L)), anchors[0][4] + int(rng.integers(0, 3))))
        ok = 0 <= b2 <= L2 - L
        mate = read_at(b2) if ok else junk(int(rng.integers(0, 1 << 20)))
        u = rng.random()
        mate_hits = []
        if ok and u < 0.35:                             # a partial hit at the true locus: either half of the read
            if rng.random() < 0.5:
                mate_hits.append((b2, b2 + 75, 0, 75, 75 - int(rng.integers(0, 3))))
            else:
                mate_hits.append((b2 + 75, b2 + 150, 75, 150, 75 - int(rng.integers(0, 3))))
        elif ok and u < 0.6:
            mate_hits.append(full(b2, 150 - int(rng.integers(0, 20))))
        if rng.random() < 0.15:                         # and an unrelated weak one
            x = int(rng.integers(0, L2 - L))
            mate_hits.append((x, x + 60, 20, 80, 45))
        mate_hits.sort(key=lambda h: -h[4])
        reads, hits = [None, None], [None, None]
        reads[a_end], hits[a_end] = read_at(a_rb), anchors
        reads[1 - a_end], hits[1 - a_end] = mate, mate_hits
        pairs.append(dict(reads=reads, hits=hits, win={}))
    return pairs, pes, opt


I_SEEDS = (1, 2, 3, 4, 5, 6)
I_SECOND_ROUND = {1: True, 2: True, 3: False, 4: True, 5: True, 6: False}
for _s in I_SEEDS:
    _pairs, _pes, _opt = generate(_s)
    case(f"I_seed{_s}", _pairs, _pes, dict(second_round=I_SECOND_ROUND[_s]), **_opt)

# The dedup removes the justifier (the first seed of the generator that shows it, kept by name).  End 1 has two anchors a base apart,
# at 10067 and 10068, and PES_NARROW admits distances 399 and 400 only.  The mate's own hit q, the second half of the read, lies at
# 400 as anchor 1 sees it (skipped against the initial list) and at 401 as anchor 0 sees it (not skipped).  Anchor 0's window ends 77
# bases short of the mate's end, so its rescue finds the last 73 bases: a hit of q's score two bases further on, which replaces q and
# lies at 398 as anchor 1 sees it -- outside.  Anchor 1's job, which nothing in the initial list asked for, is needed after all.
JUSTIFIER = dict(seed=1, pair=2, end=1, anchor=1, r=1)
_pairs, _pes, _opt = generate(JUSTIFIER["seed"])
case("E_justifier_removed", [_pairs[JUSTIFIER["pair"]]], _pes, dict(changed=[0], n_sw=2, killed=[in_hash(0, 0, 0)], second_round=True), **_opt)


# --- what the tests derive from a group's inputs alone ------------------------------------------------------------------------------
def window_ok(g, x):
    """"no funny things happening" (native/bwamem_pair.c:187): the window's bytes are all there"""
    return int(g.ref_len[x]) == int(g.ref_re[x]) - int(g.ref_rb[x])


def first_round_jobs(g, opt):
    """How many SW jobs the documented lean plan launches before it has seen any result: per end, the windows of the FIRST anchor that
    has one against the mate's initial list (later anchors wait for that result).  Every such job is one the sequential walk runs too
    (an end's anchors are judged against a list that only the other end's anchors change), so a second round is needed exactly when
    the walk's n_sw is larger -- as long as no mate is empty."""
    if opt.flag & NO_RESCUE:
        return 0
    failed = [bool(p[2]) for p in g.pes]
    n, reg_at, row_at = 0, 0, 0
    for k in range(g.group_size):
        cnt = [int(g.reg_cnt[2 * k]), int(g.reg_cnt[2 * k + 1])]
        base = [reg_at, reg_at + cnt[0]]
        rows = [row_at, row_at + int(g.ref_cnt[2 * k])]
        reg_at += cnt[0] + cnt[1]
        row_at += int(g.ref_cnt[2 * k]) + int(g.ref_cnt[2 * k + 1])
        for i in range(2):
            if cnt[i] == 0 or g.seq_len[2 * k + 1 - i] < 1:
                continue
            mine, mates = g.regs[base[i]:base[i] + cnt[i]], g.regs[base[1 - i]:base[1 - i] + cnt[1 - i]]
            j = 0
            for a in mine:
                if a["score"] < mine[0]["score"] - opt.pen_unpaired:
                    continue
                if j >= opt.max_matesw or j >= g.ref_cnt[2 * k + i]:
                    break
                skip = list(failed)
                for m in mates:
                    r, d = infer_dir(int(a["rb"]), int(m["rb"]), g.l_pac)
                    if g.pes[r][0] <= d <= g.pes[r][1]:
                        skip[r] = True
                jobs = sum(1 for r in range(4) if not skip[r] and window_ok(g, 4 * (rows[i] + j) + r))
                n += jobs
                if jobs:
                    break
                j += 1
    return n


def pair_slices(cnt):
    """per pair: the slice of the flat region array its two ends occupy"""
    at, out = 0, []
    for k in range(len(cnt) // 2):
        n = int(cnt[2 * k]) + int(cnt[2 * k + 1])
        out.append(slice(at, at + n))
        at += n
    return out


def changed_pairs(g, out_cnt, out_regs):
    a, b = pair_slices(g.reg_cnt), pair_slices(out_cnt)
    return [k for k in range(g.group_size)
            if g.reg_cnt[2 * k] != out_cnt[2 * k] or g.reg_cnt[2 * k + 1] != out_cnt[2 * k + 1] or g.regs[a[k]].tobytes() != out_regs[b[k]].tobytes()]


def window_census(g):
    rb, re, ln = g.ref_rb, g.ref_re, g.ref_len
    live = ~((rb < 0) & (re < 0))
    return dict(bridging=int((live & (ln == 0) & (re - rb > 0) & (rb < g.l_pac) & (re > g.l_pac)).sum()),
                clamped0=int((live & (rb == 0)).sum()), clamped2l=int((live & (re == 2 * g.l_pac)).sum()),
                empty=int((live & (rb == re)).sum()), failed_rows=int((~live).sum()))
