"""Named cases for the extension's row sweep (csrc/bpsw_extend_rows.h, the full kernel's sweeps in csrc/bpsw_extend_core.h): one table
for the CPU test that holds every case to its name (tests/test_ext_cases.py: the model of tests/ext_rows_model.py must report every
fact a case is named for, and agree with the oracle) and for the GPU test that runs the table on every route against the oracle
(tests/test_ext_forms_gpu.py).

A case is one task: one or two sides (the other empty), a start score, a Scoring (gap costs, band, z-drop, parse, matrix) and the set of
FACTS it exists for, in the vocabulary of facts_of() below.  Cases are BUILT from the constants they aim at -- ROWS_NARROW / ROWS4_NARROW
read from the header's text, the window sizes 64 / 128 / 256, the 64-row target chunk, 30000 -- from an alignment script (ops) over a
fixed base stream; nothing here was found by trying seeds.  Every score stays within int16: h0 + qLen * amax <= 32767.
`bound` says at which setting of the tail-row bound (shortcut bit 16) the facts are claimed: the GPU test runs every case at both."""
from dataclasses import dataclass, field, replace

import numpy as np

import ext_rows_model as erm
from ext_rows_model import Scoring, ZDROP_BWA, ZDROP_SCALA

C = erm.header_constants()
RN, R4N = C["ROWS_NARROW"], C["ROWS4_NARROW"]


# ---- sequences ------------------------------------------------------------------------------------------------------------------
def stream(n, salt=1):
    """n bases of a fixed, aperiodic stream (a 31-bit LCG's top bits); another salt gives an unrelated one"""
    x, out = 12345 + 7919 * salt, []
    for _ in range(n):
        x = (1103515245 * x + 12345) & 0x7FFFFFFF
        out.append((x >> 16) & 3)
    return out


def other(b):
    return (b + 2) & 3


def aln(ops, salt=1):
    """(query, target) from an alignment script: ("M", n) n matching bases; ("X", n) n substitutions; ("I", n) n bases only the query
    has; ("D", n) n bases only the target has; ("TN", n) / ("QN", n) n columns with an N in the target / the query; ("DN", n) n target
    N without a query base; ("T", n) unrelated target bases (as "D", named for tails)"""
    src, extra = iter(stream(4096, salt)), iter(stream(4096, salt + 101))
    q, t = [], []
    for op, n in ops:
        for _ in range(n):
            if op in ("M", "X", "TN", "QN"):
                b = next(src)
                q.append(4 if op == "QN" else b)
                t.append(4 if op == "TN" else other(b) if op == "X" else b)
            elif op == "I":
                q.append(next(extra))
            elif op in ("D", "T"):
                t.append(next(extra))
            elif op == "DN":
                t.append(4)
            else:
                raise ValueError(op)
    return q, t


def mat_of(a, b, n=-1):
    return tuple([a if i == j else -b if i < 4 and j < 4 else n for i in range(5) for j in range(5)])


DEF = Scoring()


@dataclass
class Case:
    name: str
    left: tuple                      # (query, target) or None
    right: tuple
    h0: int
    sc: Scoring = DEF
    facts: tuple = ()                # what the case is named for
    bound: bool = True               # the tail-row bound's setting at which the facts hold
    mat_max: int = 1                 # what the packer's gap bounds use (MemChainToAlignBatched.scala:106-109: the matrix's maximum)
    full: tuple = ()                 # full-kernel forms (erm.full_form) the case is named for
    full_only: bool = False          # a flank above 255 bases: the full kernel's own


def one(name, ops, h0, sc=DEF, facts=(), side="right", salt=1, **kw):
    q, t = aln(ops, salt)
    return Case(name, None if side == "right" else (q, t), (q, t) if side == "right" else None, h0, sc, tuple(facts), **kw)


def soa_of(cases, sc):
    """the cases (all of one Scoring) as one ExtTaskSoA"""
    import bpsw_hip
    pool, f = [], {k: [] for k in ("left_qlen", "left_rlen", "right_qlen", "right_rlen", "left_q_off", "left_r_off", "right_q_off",
                                    "right_r_off", "reg_score", "q_beg", "h0", "idx")}
    for i, c in enumerate(cases):
        lq, lr = c.left or ([], [])
        rq, rr = c.right or ([], [])
        for name, s in (("left_q", lq), ("left_r", lr), ("right_q", rq), ("right_r", rr)):
            f[name + "_off"].append(len(pool))
            f[name.replace("_q", "_qlen").replace("_r", "_rlen")].append(len(s))
            pool.extend(s)
        f["reg_score"].append(c.h0); f["h0"].append(c.h0); f["q_beg"].append(len(lq)); f["idx"].append(i)
    kw = {k: np.array(v, np.int64 if k.endswith("_off") else np.int32) for k, v in f.items()}
    mm = {c.mat_max for c in cases}
    assert len(mm) == 1
    return bpsw_hip.ExtTaskSoA(pool=np.array(pool + [0], np.uint8), o_del=sc.o_del, e_del=sc.e_del, o_ins=sc.o_ins, e_ins=sc.e_ins,
                               pen_clip5=sc.pen_clip5, pen_clip3=sc.pen_clip3, w=sc.w, mat_max=mm.pop(), **kw)


def batches(cases):
    """the table grouped by Scoring (a batch has one header and runs under one set_ext_scoring): [(Scoring, [Case])]"""
    groups = {}
    for c in cases:
        groups.setdefault((c.sc, c.mat_max), []).append(c)
    return [(k[0], v) for k, v in groups.items()]


# ---- facts ----------------------------------------------------------------------------------------------------------------------
def facts_of(case, sides):
    """the facts the model reports for a case: `sides` from erm.extension()"""
    F = set()
    for side, (qt, s) in enumerate(zip((case.left, case.right), sides)):
        if s is None:
            continue
        q, t = qt
        qlen, tlen = len(q), len(t)
        F.add(f"qLen={qlen}"); F.add(f"tLen={tlen}")
        if tlen < qlen:
            F.add("tLen<qLen")
        if q[0] == 4:
            F.add("qN@first")
        if q[-1] == 4:
            F.add("qN@last")
        F.add("retry" if len(s.tries) == 2 else "retry_same_band" if s.same_band else "no_retry")
        mo, thr, changed = s.retry_test
        if changed and mo == thr:
            F.add("max_off=thr")
        if changed and mo == thr - 1:
            F.add("max_off=thr-1")
        if not changed:
            F.add("score_unchanged")
        for k, call in enumerate(s.tries):
            w = call.w
            if k == 0:
                if w < case.sc.w:
                    F.add("wcut")
                F.add(f"w={w}")
            else:
                F.add(f"retry_cols={2 * case.sc.w}")
            F.add(f"first={min(qlen, w + 1)}")
            F.add(f"tle-qle={int(call.res[2] - call.res[1])}")
            F.add(f"h1z={call.i_h1z}")
            F.add("full:" + erm.full_form(call, qlen, case.sc))
            F.add(f"end:{call.ended}")
            if call.ended == "m0":
                F.add("end:m0@0" if call.end_row == 0 else "end:m0@later")
                if call.rows[-1].span < 1:
                    F.add("end:empty_band")
                    if call.end_row == qlen + w:
                        F.add("end:empty_band@qLen+w")
            if call.ended == "tail_bound" and call.end_row == qlen:
                F.add("end:tail_bound@first")
            if call.ended == "last_row":
                F.add("end:last_row")
            if call.res[4] == -1:
                F.add("gscore=-1")
            moves = 0
            for row, what in call.events:
                F.add(what)
                moves += what.startswith("move")
            if moves >= 4:
                F.add("moves>=4")
            order = [what for _, what in call.events if "to" in what and what != "togen"]
            if "4to2" in order and "2to1" in order[order.index("4to2"):]:
                F.add("4to2to1")
            for row, cols, sel in call.entries:
                F.add(f"sel{sel}"); F.add(f"sel{sel}/{cols}")
            if call.u0 >= erm.TAIL_U16:
                F.add("u0>=30000")
            if call.qa >= erm.TAIL_U16:
                F.add("qa>=30000")
            rows = call.rows
            seen_atend = pulled = in_q = False
            nrun = 0
            for a, r in zip([None] + rows[:-1], rows):
                F.add(r.form); F.add(f"cols{r.cols}")
                F.add("live" if r.live else "dead")
                if a is not None and a.live and not r.live:
                    F.add(f"live_to_dead@{r.i}")
                    if r.i == qlen:
                        F.add("live_to_dead@qLen")
                if r.i == 0 and not r.live:
                    F.add("dead_from_0")
                if r.where == "tail":
                    F.add("tail_rows")
                    if r.form.startswith("fast"):
                        F.add("fast_tail")
                    if r.form.startswith("gen"):
                        F.add("gen_tail")
                if r.cols == 2 and r.span == RN + 1:
                    F.add("cols2@narrow+1")
                if r.cols == 4 and r.span == R4N + 1:
                    F.add("cols4@narrow4+1")
                if (r.i, "2to1") in call.events and r.span == RN:
                    F.add("2to1@narrow")
                if (r.i, "4to2") in call.events and r.span == R4N:
                    F.add("4to2@narrow4")
                if r.cols in (1, 2) and not r.moved and r.fill == 64 * r.cols - 1:
                    F.add(f"fill{r.cols}=WIN-1")
                if r.cols in (1, 2) and r.moved and r.fill == 64 * r.cols:
                    F.add(f"fill{r.cols}=WIN:move")
                if r.clamp:
                    F.add(f"clamp{r.cols}")
                if r.n_row:
                    nrun += 1
                    F.add(f"nrow@{r.i}" if r.i in (0, 63, 64) else "nrow")
                    F.add(f"nrow/cols{r.cols}")
                    if r.i == tlen - 1:
                        F.add("nrow@last")
                    if r.i == qlen:
                        F.add("nrow@first_tail")
                    if nrun >= 64 and r.i63 == 63:
                        F.add("nchunk")
                else:
                    nrun = 0
                if r.improved:
                    F.add("lone" if r.n_beat == 1 else "multi")
                    if r.n_max > 1:
                        F.add("row_max_tie")
                elif r.zval is not None:
                    kk = "k>0" if r.zk > 0 else "k<=0"
                    if r.zval == case.sc.zdrop and any(b.improved for b in rows[rows.index(r) + 1:]):
                        F.add(f"znostop:{kk}:zdrop:improves_later")
                    if r.zval == case.sc.zdrop + 1:
                        F.add(f"zstop:{kk}:zdrop+1")
                    if r.zval == case.sc.zdrop:
                        F.add(f"znostop:{kk}:zdrop")
                if not r.improved and case.sc.zdrop == 0 and r.m > 0:
                    F.add("zdrop0_row")
                if r.zero:
                    # the zero cells the trimming stops at: the LAST one left of mj, the FIRST one right of it (SWUtil.scala:202-214);
                    # their slot in the lane is what the two- and four-column rows' interleaved zero masks are indexed by
                    left = [c for c in r.zero_cols if c < r.mj]
                    right = [c for c in r.zero_cols if c > r.mj]
                    for tag, c in (("zL", left[-1] if left else None), ("zR", right[0] if right else None)):
                        if c is None:
                            continue
                        F.add(f"{tag}{r.cols}:slot{(c - r.base) % r.cols}")
                        F.add(f"{tag}@mj{c - r.mj:+d}" if abs(c - r.mj) == 1 else tag)
                        if c == r.beg:
                            F.add("zL@beg")
                        if c == r.end - 1:
                            F.add("zR@end-1")
                    F.add("zero_improved" if r.improved else "zero_not_improved")
                if r.gs_tie:
                    F.add("gs_tie")
                    if r.n_row and call.res[3] == r.i + 1:
                        F.add("gs_tie@nrow")
                    if call.res[4] > 0 and call.res[3] == r.i + 1 and call.res[4] > call.res[0] - (case.sc.pen_clip3 if side else case.sc.pen_clip5):
                        F.add("gs_tie_decides_gtle")
                # `end` at the query end: the fast loops' second body serves a row that follows one with end == qLen and no zero cell;
                # a zero cell sends it back to the first body, which makes no assumption; a zero cell right of mj pulls `end` back
                if r.atend:
                    if pulled:
                        F.add("end_pulled_back_regrows")
                    if in_q and r.zero:
                        F.add("qbody_zero_return")
                        if any(c > r.mj for c in r.zero_cols):
                            F.add("qbody_end_pulled_back")
                    in_q = r.form.startswith("fast") and not r.zero
                    seen_atend = True
                else:
                    in_q = False
                    if seen_atend:
                        pulled = True
    return F


# ---- the table -------------------------------------------------------------------------------------------------------------------
def W(w, **kw):
    return replace(DEF, w=w, **kw)


def cases():
    T = []
    tail = ("T", 40)
    # -- first row and lengths: min(qLen, w + 1) of 63 | 64 and 127 | 128, once through qLen and once through w
    T.append(one("first63_qlen", [("M", 63), tail], 30, facts=["first=63", "start1"]))
    T.append(one("first64_qlen", [("M", 64), tail], 30, facts=["first=64", "start2"]))
    T.append(one("first63_w", [("M", 100), tail], 30, W(62), facts=["first=63", "start1"]))
    T.append(one("first64_w", [("M", 100), tail], 30, W(63), facts=["first=64", "start2"]))
    T.append(one("first127_qlen", [("M", 127), tail], 30, W(127), facts=["first=127", "start2"]))
    T.append(one("first128_qlen", [("M", 128), tail], 30, W(127), facts=["first=128", "start4"]))
    T.append(one("first127_w", [("M", 200), tail], 30, W(126), facts=["first=127", "start2"]))
    T.append(one("first128_w", [("M", 200), tail], 30, W(127), facts=["first=128", "start4"]))
    # -- lengths
    T.append(one("qlen1", [("M", 1), ("T", 3)], 19, facts=["qLen=1"]))
    T.append(one("qlen255", [("M", 255), ("T", 20)], 50, facts=["qLen=255"], full=["leanS"]))
    T.append(one("tlen1", [("M", 1), ("I", 20)], 30, facts=["tLen=1", "tLen<qLen", "end:last_row"]))
    T.append(one("tlen_lt_qlen", [("M", 30), ("I", 30)], 30, facts=["tLen<qLen", "end:last_row"]))
    for n in (63, 64, 65, 128, 129):
        T.append(one(f"tlen{n}", [("M", n), ("I", 10)], 40, facts=[f"tLen={n}", "end:last_row"]))
    for w in (0, 1, 2):
        T.append(one(f"w{w}", [("M", 12), ("X", 1), ("M", 20), tail], 30, W(w), facts=[f"w={w}"]))
    T.append(one("wcut_ins", [("M", 20), tail], 30, replace(DEF, e_ins=10), facts=["wcut", "w=2"]))
    T.append(one("wcut_del", [("M", 20), tail], 30, replace(DEF, e_del=10), facts=["wcut", "w=2"]))
    # -- band tries
    T.append(one("retry_at_thr", [("I", 6), ("M", 40), tail], 40, W(8), facts=["retry", "max_off=thr"]))
    T.append(one("retry_below_thr", [("I", 5), ("M", 40), tail], 40, W(8), facts=["no_retry", "max_off=thr-1"]))
    T.append(one("retry_same_band", [("D", 6), ("M", 20), tail], 40, replace(DEF, w=8, e_ins=3), facts=["retry_same_band", "max_off=thr"]))
    T.append(one("retry_unchanged", [("X", 20), tail], 40, W(8), facts=["no_retry", "score_unchanged"]))
    big = replace(DEF, zmode=ZDROP_BWA)       # (the BWA parse: a long deletion is no z-drop, X - k eDel stays at oDel)
    T.append(one("retry128", [("M", 20), ("D", 48), ("M", 120), tail], 100, replace(big, w=64), facts=["retry", "retry_cols=128", "max_off=thr", "start4"]))
    T.append(one("retry140", [("M", 20), ("D", 52), ("M", 130), tail], 100, replace(big, w=70), facts=["retry", "retry_cols=140", "max_off=thr", "start4"]))
    T.append(one("retry254", [("M", 30), ("D", 94), ("M", 225), tail], 150, replace(big, w=127), facts=["retry", "retry_cols=254", "max_off=thr", "start4"]))
    # -- layout changes (the bands of a perfect flank: LIVE rows grow by a column a row from column 0, DEAD rows slide)
    T.append(one("lay_1to2_2to1", [("M", 255), ("T", 20)], 50, facts=["1to2", "2to1", "2to1@narrow", "cols2@narrow+1", "move2", "fill2=WIN-1", "fill2=WIN:move"]))
    T.append(one("lay_2to4_4to2", [("M", 200), ("T", 150)], 80, W(127), facts=["start4", "4to2", "2to4", "4to2@narrow4", "cols4@narrow4+1"], full=["reg<4>>leanS>reg<4>"]))
    T.append(one("lay_4to2to1", [("M", 128), tail], 30, W(127), facts=["start4", "4to2to1"], full=["reg<3>>leanS"]))
    T.append(one("lay_stay4", [("M", 200), ("T", 150)], 150, W(127), facts=["start4", "cpp4", "clamp4"], full=["reg<4>"]))
    T.append(one("lay_4to2_tail", [("M", 200), ("T", 250)], 150, W(127), facts=["4to2", "4to2@narrow4", "tail_rows", "fast_tail"], bound=False))
    T.append(one("lay_dead_slide200", [("M", 200), tail], 30, W(126), facts=["move1", "moves>=4", "fill1=WIN-1", "fill1=WIN:move", "dead"]))
    # -- phases of h1
    for e, h0, z in ((1, 18, 11), (2, 18, 5), (3, 18, 3), (2, 19, 6), (3, 19, 4)):
        T.append(one(f"ph_edel{e}_h{h0}", [("M", 30), tail], h0, replace(DEF, e_del=e), facts=[f"h1z={z}", f"live_to_dead@{z}"]))
    T.append(one("ph_h0_eq_odel", [("M", 30), tail], 6, facts=["dead_from_0", "h1z=0"]))
    T.append(one("ph_h0_lt_odel", [("M", 30), tail], 5, facts=["dead_from_0", "h1z=0"]))
    T.append(one("ph_h1z0", [("M", 30), tail], 7, facts=["dead_from_0", "h1z=0"]))
    T.append(one("ph_h1z1", [("M", 30), tail], 8, facts=["live_to_dead@1"]))
    T.append(one("ph_h1z63", [("M", 100), tail], 70, facts=["live_to_dead@63"]))
    T.append(one("ph_h1z64", [("M", 100), tail], 71, facts=["live_to_dead@64"]))
    T.append(one("ph_l2d_at_tail", [("M", 26), ("X", 4), ("T", 30)], 37, facts=["live_to_dead@qLen", "tail_rows", "fast_tail", "end:tail_bound"]))
    T.append(one("tb_first_tail_row", [("M", 40), tail], 30, facts=["end:tail_bound@first"]))
    T.append(one("tb_never", [("M", 15), ("I", 200), ("T", 270)], 250, replace(DEF, o_ins=100, zdrop=0), facts=["gscore=-1", "tail_rows"]))
    # -- the 16-bit forms of the tail rows
    M120 = replace(DEF, mat=mat_of(120, 4))
    T.append(one("u16_qa29880", [("M", 245), ("X", 4), ("DN", 1), ("T", 30)], 100, M120, facts=["u0>=30000", "sel0", "gen_tail", "nrow@first_tail"], mat_max=120))
    T.append(one("u16_qa30000", [("M", 246), ("X", 4), ("DN", 1), ("T", 30)], 100, M120, facts=["qa>=30000", "sel0", "gen_tail", "nrow@first_tail"], mat_max=120))
    T.append(one("u16_u0_29999", [("M", 90), ("X", 10), ("DN", 1), ("T", 30)], 29806, facts=["sel3", "fast_tail", "nrow@first_tail"]))
    T.append(one("u16_u0_30000", [("M", 90), ("X", 10), ("DN", 1), ("T", 30)], 29807, facts=["u0>=30000", "sel0", "gen_tail", "nrow@first_tail"]))
    T.append(one("u16_u0_29999_cols1", [("M", 20), ("X", 10), ("DN", 1), ("T", 30)], 29946, facts=["sel3/1", "fast_tail", "nrow@first_tail"]))
    T.append(one("u16_u0_30000_cols1", [("M", 20), ("X", 10), ("DN", 1), ("T", 30)], 29947, facts=["u0>=30000", "sel0/1", "gen_tail", "nrow@first_tail"]))
    # -- left clamp
    T.append(one("clamp_cols1", [("M", 20), ("D", 12), ("M", 30), tail], 40, replace(big, w=8), facts=["clamp1", "togen", "gen1"]))
    T.append(one("clamp_cols2", [("M", 30), ("D", 40), ("M", 100), tail], 120, replace(big, w=40), facts=["clamp2", "togen", "gen2"]))
    # -- N
    T.append(one("n_row0", [("TN", 1), ("M", 40), tail], 30, facts=["nrow@0"]))
    T.append(one("n_row63", [("M", 63), ("TN", 1), ("M", 30), tail], 40, facts=["nrow@63"]))
    T.append(one("n_row64", [("M", 64), ("TN", 1), ("M", 30), tail], 40, facts=["nrow@64"]))
    T.append(one("n_last_row", [("M", 30), ("TN", 1), ("I", 5)], 30, facts=["nrow@last", "end:last_row"]))
    T.append(one("n_chunk", [("M", 64), ("TN", 64), ("M", 20), tail], 100, facts=["nchunk"]))
    T.append(one("n_first_tail_row", [("M", 26), ("X", 4), ("DN", 1), ("T", 30)], 37, facts=["nrow@first_tail", "tail_rows"]))
    T.append(one("n_cols2", [("M", 100), ("TN", 1), ("M", 60), tail], 50, facts=["nrow/cols2"]))
    T.append(one("n_cols4", [("M", 100), ("TN", 1), ("M", 99), tail], 150, W(127), facts=["nrow/cols4"]))
    T.append(one("n_query_ends", [("QN", 1), ("M", 30), ("QN", 1), tail], 30, facts=["qN@first", "qN@last"]))
    # -- row decisions
    T.append(one("lone_cell", [("M", 30), tail], 30, facts=["lone"]))
    # two diagonals, four columns apart, that tie from the row on where both beat the maximum: two substitutions (2 x 5) against an
    # insertion of four (6 + 4) into a period-4 repeat
    rep = [0, 1, 2, 3] * 8
    pre = stream(20, 7)
    T.append(Case("row_max_tie", None, (pre + [2, 3, 2, 3] + rep, pre + rep + [0, 1, 2, 3] + stream(20, 8)), 40, facts=("multi", "row_max_tie")))
    ZS = replace(DEF, zdrop=20)
    T.append(one("zs_scala_kpos_at", [("M", 20), ("T", 30)], 40, ZS, facts=["znostop:k>0:zdrop", "end:zdrop"], salt=3, bound=False))
    T.append(one("zs_scala_kpos_over", [("M", 20), ("I", 1), ("DN", 1), ("T", 30)], 40, ZS, facts=["zstop:k>0:zdrop+1"], salt=3, bound=False))
    # a deletion of seven: its last row sits AT the margin (6 + 2 x 7 == zdrop), and the flank goes on to a new maximum behind it
    T.append(one("zs_scala_kpos_at_then_improves", [("M", 20), ("D", 7), ("M", 40), tail], 40, ZS, facts=["znostop:k>0:zdrop:improves_later", "tle-qle=7"]))
    ZB = replace(DEF, zdrop=10, zmode=ZDROP_BWA)
    T.append(one("zs_bwa_kneg", [("M", 20), ("I", 30), ("DN", 30)], 40, ZB, facts=["znostop:k<=0:zdrop", "zstop:k<=0:zdrop+1"]))
    T.append(one("zs_bwa_kpos_over", [("M", 20), ("I", 5), ("DN", 15)], 40, ZB, facts=["zstop:k>0:zdrop+1"]))
    T.append(one("zs_bwa_kpos_at", [("M", 20), ("I", 4), ("DN", 15)], 40, ZB, facts=["znostop:k>0:zdrop"]))
    T.append(one("zdrop0", [("M", 20), ("T", 60)], 40, replace(DEF, zdrop=0), facts=["zdrop0_row", "end:m0@later"], bound=False))
    T.append(one("zdrop0_bwa", [("M", 20), ("T", 60)], 40, replace(DEF, zdrop=0, zmode=ZDROP_BWA), facts=["zdrop0_row", "end:m0@later"], bound=False))
    T.append(Case("m0_row0", None, ([0] * 5, [2] * 10), 3, facts=("end:m0@0",)))
    T.append(one("m0_later", [("M", 5), ("X", 20), tail], 8, facts=["end:m0@later"]))
    T.append(one("empty_band", [("I", 6), ("M", 40), tail], 40, W(8), facts=["end:empty_band@qLen+w"], bound=False))
    # gscore ties: two substitutions in the first copy of the flank's last four bases (4 - 2 x 5) against deleting it (4 - (6 + 4))
    endq = stream(24, 9)
    r4 = endq[-4:]
    T.append(Case("gscore_tie", None, (endq, endq[:-4] + [other(r4[0]), other(r4[1])] + r4[2:] + r4 + stream(10, 10)), 40,
                  replace(DEF, pen_clip5=10, pen_clip3=10), facts=("gs_tie", "gs_tie_decides_gtle")))
    # (row 0 spans the query, its zero cells pull `end` back to what h0 reaches; it is back at the query end by row 3; five substitutions
    # then starve the cells at the query end while the rows run in the fast loop's second body)
    # ... and with the later row an N row (the C++ row's own gscore step): both bases of the first copy substituted (2 - 2 x 5) against deleting
    # it and meeting one base and an N (-(6 + 2) + 1 - 1)
    r2 = endq[-2:]
    T.append(Case("gscore_tie_n_row", None, (endq, endq[:-2] + [other(r2[0]), other(r2[1])] + [r2[0], 4] + stream(10, 10)), 40,
                  replace(DEF, pen_clip5=10, pen_clip3=10), facts=("gs_tie", "gs_tie_decides_gtle", "gs_tie@nrow")))
    # a flank that starts with a deletion: the best path runs down the h1 column, through the cell every row writes at the band's left end
    T.append(one("h1_path_cols4", [("D", 5), ("M", 200), tail], 150, W(127), facts=["start4", "cpp4", "tle-qle=5"]))
    T.append(one("h1_path_n_rows", [("DN", 3), ("M", 40), tail], 60, facts=["nrow@0", "cpp1", "tle-qle=3"]))
    T.append(one("end_pulled_back", [("M", 6), ("X", 5), ("M", 18), tail], 30, facts=["end_pulled_back_regrows", "qbody_zero_return", "qbody_end_pulled_back", "zR@end-1"]))
    # zero cells next to the maximum in the wide layouts: without deletions (oDel = 100) nothing holds the columns left of the
    # diagonal up, without insertions nothing those right of it
    DELX = replace(DEF, o_del=100, mat=mat_of(2, 4), w=127)
    INSX = replace(DEF, o_ins=100, mat=mat_of(2, 4), w=127)
    T.append(one("zero_left_delx", [("M", 200), ("T", 50)], 60, DELX, mat_max=2, facts=["dead_from_0", "zR4:slot0"]))
    T.append(one("zero_right_insx", [("M", 200), ("T", 50)], 60, INSX, mat_max=2, facts=["zR@mj+1", "zR4:slot1"]))
    # a zero cell LEFT of the maximum in the wide layouts: after an insertion the columns the old diagonal held decay behind the band's
    # left end, which a LIVE h1 keeps where it is; start score and insertion length place the first such cell in each slot of a lane
    for h0, ins, slot in ((60, 10, "zL2:slot0"), (40, 10, "zL2:slot1"), (80, 30, "zL4:slot0"), (100, 60, "zL4:slot1"), (80, 60, "zL4:slot2"),
                          (120, 30, "zL4:slot3")):
        T.append(one(f"zero_left_{slot[2:].replace(':', '_')}", [("M", 20), ("I", ins), ("M", 150), tail], h0, replace(big, w=127), facts=[slot]))
    # (the right-hand slots come with the flanks above: a row's new column `end - 1` is a zero cell until the scores reach it)
    # -- both sides of a task: the right side starts from the score the left one reached
    lq, lt = aln([("M", 30), ("X", 1), ("M", 20), tail], 11)
    rq, rt = aln([("M", 70), ("TN", 1), ("M", 40), tail], 12)
    T.append(Case("two_sides", (lq, lt), (rq, rt), 30, facts=("qLen=51", "qLen=111", "start2", "nrow/cols2")))
    T.append(one("left_only", [("M", 40), ("X", 2), ("M", 30), tail], 25, side="left", facts=["qLen=72", "lone"]))
    # -- the full kernel's own: a first row above 127 columns that never fits the sliding window (no hand-over), flanks above 255 bases
    # (the LDS-row sweep), the limits of include/bpsw.h
    T.append(one("full_reg3_no_handover", [("M", 150), tail], 150, W(127), facts=["start4"], full=["reg<3>"]))
    T.append(one("full_qlen256", [("M", 256), ("T", 20)], 50, facts=["qLen=256"], full=["wave"], full_only=True))
    T.append(one("full_qlen_max", [("M", 400), ("X", 3), ("M", C["MAX_QLEN"] - 403), ("T", 60)], 100, facts=[f"qLen={C['MAX_QLEN']}"], full=["wave"], full_only=True))
    T.append(one("full_rlen_max", [("M", 300), ("T", C["MAX_RLEN"] - 300)], 100, facts=[f"tLen={C['MAX_RLEN']}", "qLen=300"], full=["wave"], full_only=True))
    T.append(one("full_rlen_max_short_flank", [("M", 100), ("T", C["MAX_RLEN"] - 100)], 100, facts=[f"tLen={C['MAX_RLEN']}"], full=["lean2"]))
    return T


def past_the_limits():
    """one task past each limit of include/bpsw.h: refused with BpswError"""
    return [one("qlen_past_max", [("M", C["MAX_QLEN"] + 1), ("T", 10)], 100), one("rlen_past_max", [("M", 50), ("T", C["MAX_RLEN"] + 1 - 50)], 100)]


# every fact, layout, transition, selector value and full-kernel form the table must reach at least once (tests/test_ext_cases.py)
REQUIRED = """
start1 start2 start4 first=63 first=64 first=127 first=128 qLen=1 qLen=255 qLen=256 tLen=1 tLen<qLen tLen=63 tLen=64 tLen=65 tLen=128
tLen=129 w=0 w=1 w=2 wcut retry no_retry retry_same_band score_unchanged max_off=thr max_off=thr-1 retry_cols=128 retry_cols=140
retry_cols=254
1to2 2to1 2to4 4to2 4to2to1 2to1@narrow cols2@narrow+1 4to2@narrow4 cols4@narrow4+1 move1 move2 moves>=4 fill1=WIN-1 fill1=WIN:move
fill2=WIN-1 fill2=WIN:move cols1 cols2 cols4
live dead dead_from_0 h1z=0 live_to_dead@1 live_to_dead@63 live_to_dead@64 live_to_dead@qLen end:tail_bound@first gscore=-1 tail_rows
sel0 sel1 sel2 sel3 sel4 sel0/1 sel0/2 sel1/1 sel1/2 sel2/1 sel2/2 sel3/1 sel3/2 sel4/1 sel4/2 u0>=30000 qa>=30000 fast_tail gen_tail
fast1L fast1D fast1LT fast1DT fast2L fast2D fast2LT fast2DT gen1 gen2 cpp1 cpp2 cpp4 togen clamp1 clamp2 clamp4
nrow@0 nrow@63 nrow@64 nrow@last nchunk nrow@first_tail nrow/cols1 nrow/cols2 nrow/cols4 qN@first qN@last
lone multi row_max_tie zstop:k>0:zdrop+1 znostop:k>0:zdrop znostop:k>0:zdrop:improves_later zstop:k<=0:zdrop+1 znostop:k<=0:zdrop zdrop0_row end:zdrop end:m0@0 end:m0@later
end:empty_band@qLen+w end:last_row zL@mj-1 zR@mj+1 zL@beg zR@end-1 zL2:slot0 zL2:slot1 zR2:slot0 zR2:slot1 zL4:slot0 zL4:slot1 zL4:slot2
zL4:slot3 zR4:slot0 zR4:slot1 zR4:slot2 zR4:slot3 zero_improved zero_not_improved gs_tie gs_tie_decides_gtle gs_tie@nrow tle-qle=5 tle-qle=3 end_pulled_back_regrows
qbody_zero_return qbody_end_pulled_back
full:lean1 full:lean2 full:leanS full:leanS>reg<3> full:leanS>reg<4> full:reg<3> full:reg<4> full:reg<3>>leanS full:reg<4>>leanS
full:reg<3>>leanS>reg<3> full:reg<4>>leanS>reg<4> full:wave
""".split()
