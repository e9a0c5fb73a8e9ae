"""A plain row-by-row SWExtend (SWUtil.scala:61-230) that says WHAT EVERY ROW WAS: CPU only, numpy, no kernel code.

Three things live here.
  * sweep(): one SWExtend call, the recurrences in the kernels' parallel form (a = max(H + s, E), F a max-plus prefix, the LAST
    arg-max of the row), with one record per swept row holding the facts the row loops of csrc/bpsw_extend_rows.h branch on.
    tools/row_mix_census.py bins the rows of a bench-shaped batch with it; tests/test_ext_cases.py holds every named case of
    tests/ext_cases.py to the facts it is named for.
  * the layout state machine of sw_extend_adaptive / rows_cpp / rows_cpp4 restated on the band alone -- columns per lane at each row,
    the window base, each window move or layout change with the row it happens on -- and the dispatcher's loop selector (`sel`) with
    the rows every entry of an assembly loop covers.  A RESTATEMENT: the C++ pieces are quoted line by line below; what the assembly
    loops do between two dispatcher entries (they move their window, change over from LIVE to DEAD and from body to tail by themselves,
    and leave for the general loop where the left clamp may bind) follows their comments.  Only the GPU tests hold the kernel to it.
  * extension(): both sides of a task as ext_do_task runs them (csrc/bpsw_extend.hip): the band tries (wBand << i, cut by the
    record's maxIns / maxDel, the retry whose effective band is the first one's, the max_off test) and the ten output words; and
    full_form(): which of the full kernel's sweeps sw_extend_reg_any gives a call to.
Everything is decoded from the PACKED batch (decode_task), so maxIns / maxDel are the record's."""
import os
import re
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cloud-scale-bwamem_amd", "csrc")
ZDROP_SCALA, ZDROP_BWA = 0, 1
NO_TAIL = 0x7FFFFFFF
TAIL_U16 = 30000   # sw_extend_adaptive: the tail rows' fast loops hold gscore in 16 bits: u0 < 30000 && qa < 30000

_consts = None


def header_constants():
    """ROWS_NARROW / ROWS4_NARROW as csrc/bpsw_extend_rows.h has them TODAY (read from its text: a changed constant moves the case
    tables with it), and the limits of include/bpsw.h"""
    global _consts
    if _consts is None:
        text = open(os.path.join(CSRC, "bpsw_extend_rows.h")).read()
        api = open(os.path.join(ROOT, "include", "bpsw.h")).read()

        def grab(src, pat):
            m = re.search(pat, src)
            assert m, pat
            return int(m.group(1))
        _consts = {"ROWS_NARROW": grab(text, r"constexpr int ROWS_NARROW = (\d+);"),
                   "ROWS4_NARROW": grab(text, r"constexpr int ROWS4_NARROW = (\d+);"),
                   "MAX_QLEN": grab(api, r"#define BPSW_EXT_MAX_QLEN (\d+)"),
                   "MAX_RLEN": grab(api, r"#define BPSW_EXT_MAX_RLEN (\d+)")}
    return _consts


@dataclass(frozen=True)
class Scoring:
    """what a batch's header and the context's scoring say; mat[5 * target + query]"""
    mat: tuple = tuple([1 if i == j else -4 if i < 4 and j < 4 else -1 for i in range(5) for j in range(5)])
    o_del: int = 6
    e_del: int = 1
    o_ins: int = 6
    e_ins: int = 1
    w: int = 100
    zdrop: int = 100
    zmode: int = ZDROP_SCALA
    pen_clip5: int = 5
    pen_clip3: int = 5

    @property
    def amax(self):
        return max(self.mat)   # bpsw_set_ext_scoring: ext_sc.mat_max, the largest entry


@dataclass
class Row:
    i: int
    beg_in: int         # beg as the previous row's trimming left it
    beg: int            # the band [beg, end) the row swept (after the clamp of SWUtil.scala:140-142)
    end: int
    span: int
    live: bool          # h1 > 0 (the kernels: i < i_h1z)
    where: str          # "body" (i < qLen) or "tail"
    atend: bool         # end == qLen
    improved: bool      # m > max so far
    n_beat: int         # cells of the row above the old maximum (1: the fast loops' lone-cell route; more: their out-of-line key scan)
    n_max: int          # cells that hold the row maximum (more than one: the LAST one is mj, SWUtil.scala:158-161)
    zero: bool          # a zero cell in the band
    zero_rel: tuple     # the zero cells' columns relative to mj
    zero_cols: tuple    # ... and absolute
    n_row: bool         # the target base is an N
    i63: int
    clamp: bool         # beg + w + 1 <= i with the band the previous row left: the left clamp may bind (the general loop)
    m: int
    mj: int
    h1: int
    gs_set: bool        # the row set gscore / max_ie (gscore <= hlast at the query end)
    gs_tie: bool        # ... with gscore == hlast: the later row wins
    cols: int = 0       # columns per lane of the layout that swept it (1 / 2 / 4), its window base
    base: int = 0
    fill: int = 0       # end - base before any move: WIN - 1 is the most a window holds
    moved: bool = False
    form: str = ""      # which row loop (layout_forms)
    zk: int = None      # a row that did not improve: the z-drop test's k and its value (X + k eIns or X - k eDel), stop when > zdrop
    zval: int = None


@dataclass
class Call:
    res: np.ndarray                 # max, qle, tle, gtle, gscore, max_off
    rows: list
    ended: str                      # "m0", "zdrop", "tail_bound", "last_row", ("empty_band" rides on "m0": an empty band has m == 0)
    end_row: int
    events: list = field(default_factory=list)     # (row, what): "1to2" "2to1" "2to4" "4to2" "move1" "move2" "move4" "start1|2|4" "overflow"
    entries: list = field(default_factory=list)    # (row, cols, sel): the dispatcher's entries into an assembly loop
    w: int = 0
    i_h1z: int = 0
    u0: int = 0
    qa: int = 0


def i_h1z_of(h0, o_del, e_del):
    """sw_extend_adaptive: the first row whose h1 = max(0, h0 - oDel - eDel (i + 1)) is zero"""
    return (h0 - o_del + e_del - 1) // e_del - 1 if h0 - o_del > 0 else 0


def tail_row_bound(qlen, i, h0, amax, o_del, e_del):
    return max(h0 + qlen * amax - o_del - (i - qlen + 1) * e_del, qlen * amax)


def zdrop_value(k, X, sc):
    """bpsw_extend_core.h zdrop_stop: the value compared with zdrop, or None when this parse has no test for this k"""
    if k > 0:
        return X + k * sc.e_ins if sc.zmode == ZDROP_SCALA else X - k * sc.e_del
    return X + k * sc.e_ins if sc.zmode != ZDROP_SCALA else None


def sweep(q, t, h0, sc, w, tail_bound=True, stats=None, span_hist=None):
    """One SWExtend call with band w (already cut by maxIns / maxDel).  tail_bound: shortcut bit 16 (bpsw_extend_core.h
    tail_row_bound); without it i_tail is infinite.  stats / span_hist: the census's bins (tools/row_mix_census.py)."""
    q = np.asarray(q, np.int64); t = np.asarray(t, np.int64)
    mat = np.asarray(sc.mat, np.int64).reshape(5, 5)
    oD, eD, oI, eI = sc.o_del, sc.e_del, sc.o_ins, sc.e_ins
    qlen, tlen = len(q), len(t)
    amax = sc.amax if tail_bound else 0
    i_tail = qlen if amax > 0 else NO_TAIL
    ih1z = i_h1z_of(h0, oD, eD)
    H = np.zeros(qlen + 2, np.int64); E = np.zeros(qlen + 2, np.int64)
    H[0] = h0
    if qlen >= 1:
        H[1] = h0 - (oI + eI) if h0 > oI + eI else 0
    j = 2
    while j <= qlen and H[j - 1] > eI:
        H[j] = H[j - 1] - eI; j += 1
    mx, max_i, max_j, max_ie, gscore, max_off = h0, -1, -1, -1, -1, 0
    beg, end = 0, qlen
    prof = mat[:, q] if qlen else np.zeros((5, 0), np.int64)
    rows, ended, end_row = [], "last_row", tlen
    for i in range(tlen):
        h1 = max(0, h0 - (oD + eD * (i + 1)))
        beg_in = beg
        clamp = beg + w + 1 <= i
        if i >= i_tail:
            U = tail_row_bound(qlen, i, h0, amax, oD, eD)
            if U <= mx and U < gscore:
                ended, end_row = "tail_bound", i
                break
        beg = max(beg, i - w); end = min(end, i + w + 1, qlen)
        span = end - beg
        if span > 0:
            js = np.arange(beg, end)
            a = np.maximum(H[js] + prof[t[i], js], E[js])
            g = a + js * eI - (oI + eI)
            pre = np.maximum.accumulate(g)
            F = np.concatenate(([0], np.maximum(0, pre[:-1] - (js[1:] - 1) * eI)))
            Hn = np.maximum(np.maximum(a, F), 0)
            m = int(Hn.max()); mj = int(js[len(js) - 1 - int(np.argmax(Hn[::-1]))])
            E[js] = np.maximum(np.maximum(E[js] - eD, Hn - (oD + eD)), 0)
            H[beg] = h1; H[beg + 1:end + 1] = Hn
            E[end] = 0
            hlast = int(Hn[-1])
            zc = js[Hn == 0]
        else:
            m, mj, hlast = 0, -1, h1
            H[end] = h1; E[end] = 0
            zc = np.zeros(0, np.int64); Hn = np.zeros(0, np.int64)
        gs_set = gs_tie = False
        if (end if span > 0 else beg) == qlen and gscore <= hlast:
            gs_set, gs_tie = True, gscore == hlast
            max_ie, gscore = i, hlast
        imp = m > mx
        row = Row(i=i, beg_in=beg_in, beg=beg, end=end, span=span, live=h1 > 0, where="tail" if i >= qlen else "body", atend=end == qlen,
                  improved=imp, n_beat=int((Hn > mx).sum()), n_max=int((Hn == m).sum()) if m > 0 else 0, zero=zc.size > 0, zero_rel=tuple(int(c) - mj for c in zc),
                  zero_cols=tuple(int(c) for c in zc), n_row=int(t[i]) == 4, i63=i & 63, clamp=clamp, m=m, mj=mj, h1=h1,
                  gs_set=gs_set, gs_tie=gs_tie)
        rows.append(row)
        if span_hist is not None:
            span_hist[min(span, 255) // 8] += 1
        if stats is not None:
            stats[("cols2" if span > 63 else "cols1", "live" if h1 > 0 else "dead", "atend" if end == qlen else "inner",
                   "tail" if i >= qlen else "body", "zero" if row.zero else "nozero", "imp" if imp else "noimp")] += 1
        if m == 0:
            ended, end_row = "m0", i
            break
        if imp:
            mx, max_i, max_j = m, i, mj; max_off = max(max_off, abs(mj - i))
        elif sc.zdrop > 0:
            k = (i - max_i) - (mj - max_j)
            row.zk, row.zval = k, zdrop_value(k, mx - m, sc)
            if row.zval is not None and row.zval > sc.zdrop:
                ended, end_row = "zdrop", i
                break
        j = mj
        while j >= beg and H[j] > 0: j -= 1
        beg = j + 1
        j = mj + 2
        while j <= end and H[j] > 0: j += 1
        end = j
    call = Call(res=np.array([mx, max_j + 1, max_i + 1, max_ie + 1, gscore, max_off]), rows=rows, ended=ended, end_row=end_row, w=w,
                i_h1z=ih1z, u0=h0 + qlen * amax - oD + (qlen - 1) * eD, qa=qlen * amax)
    return call


# ---- the layout state machine (sw_extend_adaptive / rows_cpp<1|2> / rows_cpp4) ----------------------------------------------------
def layout(call, qlen, tlen, consts=None):
    """Columns per lane, window base, moves and changes of every swept row, from the bands alone.  Fills Row.cols / base / fill / moved
    and call.events.  (An event carries the row BEFORE which it happens: that row is then swept in the new layout.)"""
    c = consts or header_constants()
    RN, R4N = c["ROWS_NARROW"], c["ROWS4_NARROW"]
    w = call.w
    first = min(qlen, w + 1)                                   # row 0 spans min(qLen, w + 1) columns
    cols = 1 if first <= 63 else 2 if first <= 127 else 4
    base = 0
    ev = call.events
    ev.append((0, f"start{cols}"))
    for r in call.rows:
        nbeg, nend = r.beg, r.end
        r.fill = nend - base
        while True:
            if cols == 4:                                      # rows_cpp4
                if nend - nbeg <= R4N and nend > nbeg:
                    cols, base = 2, nbeg & ~1                  # rows_wide_phase: back to two columns, window at the band's left end
                    ev.append((r.i, "4to2"))
                    continue
                if nend - base > 255:
                    base = nbeg & ~3; r.moved = True
                    ev.append((r.i, "move4"))
            elif cols == 2:                                    # rows_cpp<2>
                if nend - nbeg <= RN and nend > nbeg:
                    cols, base = 1, nbeg
                    ev.append((r.i, "2to1"))
                    continue
                if nend - base > 127:
                    nb = nbeg & ~1
                    if nend - nb > 127:                        # ROWS_OVERFLOW: four columns per lane
                        cols, base = 4, nbeg & ~3
                        ev.append((r.i, "2to4"))
                        continue
                    base = nb; r.moved = True
                    ev.append((r.i, "move2"))
            else:                                              # rows_cpp<1>
                if nend - base > 63:
                    if nend - nbeg > 63:                       # ROWS_OTHER_MODE: two columns per lane
                        nb = nbeg & ~1
                        if nend - nb > 127:
                            ev.append((r.i, "overflow"))       # (sw_extend_adaptive's *overflow: no input is known to get here)
                            return call
                        cols, base = 2, nb
                        ev.append((r.i, "1to2"))
                        continue
                    base = nbeg; r.moved = True
                    ev.append((r.i, "move1"))
            break
        r.cols, r.base = cols, base
    return call


def loop_forms(call, t, qlen, tail_bound=True):
    """Which row loop sweeps each row, and the dispatcher's entries (row, cols, sel) -- sw_extend_adaptive's for (;;):
       sel = (beg + w + 1 > i && (!tail || (u0 < 30000 && qa < 30000))) ? (live ? 1 : 2) + (tail ? 2 : 0) : 0.
    Row.form: "cpp1|2|4" (the C++ row: an N row, a window the general loop will not move, a layout change, an empty band), "gen1|2"
    (the general assembly loop), "fast1|2" + "L|D" (phase of h1) + "T" (rows at and past the query end)."""
    t = np.asarray(t)
    tlen = len(t)
    w = call.w
    i_tail = qlen if tail_bound else NO_TAIL
    changed = {row for row, what in call.events if what in ("1to2", "2to1", "2to4", "4to2")}
    is_n = t == 4
    run = None          # inside an assembly loop: {"kind": "gen" | "fast", "rowend": ...}
    for r in call.rows:
        i = r.i
        WIN = 64 * r.cols
        if r.cols == 4:
            r.form, run = "cpp4", None
            continue
        if i in changed:
            run = None
        entered = False
        while True:
            if run is None:                                                    # the dispatcher
                chunk_end = min(tlen, ((i >> 6) + 1) << 6)
                ahead = np.nonzero(is_n[i:chunk_end])[0]
                row_end = i + int(ahead[0]) if ahead.size else chunk_end        # rows_asm_end
                if row_end <= i:
                    r.form = f"cpp{r.cols}"                                    # an N row
                    break
                tail = i >= i_tail
                sel = ((1 if r.live else 2) + (2 if tail else 0)) if (not tail or (call.u0 < TAIL_U16 and call.qa < TAIL_U16)) else 0
                call.entries.append((i, r.cols, sel))
                run = {"kind": "gen" if sel == 0 else "fast", "rowend": min(row_end, i_tail) if sel == 0 and not tail else row_end}
                entered = True                                                  # (the dispatcher has clamped beg: beg + w + 1 > i on this row)
            elif i >= run["rowend"]:
                # the fast loops fetch the next 64 target rows themselves when row i starts a chunk that holds no N
                if run["kind"] == "fast" and (i & 63) == 0 and not is_n[i:min(tlen, i + 64)].any():
                    run["rowend"] = min(i + 64, tlen)
                else:
                    run = None
                    continue
            if run["kind"] == "fast" and not entered and r.clamp:               # L_ftogen: the left clamp may bind from here on
                run["kind"] = "gen"
                call.events.append((i, "togen"))
            over = r.fill > WIN - 1
            if run["kind"] == "gen":
                if over or r.span < 1:                                           # L_slow: rows_cpp sweeps the row
                    r.form, run = f"cpp{r.cols}", None
                else:
                    r.form = f"gen{r.cols}"
            else:
                if r.span < 1:
                    r.form, run = f"cpp{r.cols}", None
                else:
                    r.form = f"fast{r.cols}" + ("L" if r.live else "D") + ("T" if i >= i_tail else "")
            break
    return call


def annotate(call, q, t, tail_bound=True, consts=None):
    """layout + loop forms of a finished sweep"""
    layout(call, len(q), len(t), consts)
    loop_forms(call, t, len(q), tail_bound)
    return call


# ---- the full kernel's dispatch (bpsw_extend_core.h sw_extend_reg_any; ext_do_task's reg_path) ------------------------------------
def full_form(call, qlen, sc):
    """lean1 | lean2 | leanS | leanS>reg<S> (a later row outgrew the sliding window: the slot sweep from the first row) |
    reg<S>>leanS (hand-over) | reg<S>>leanS>reg<S> | reg<S> (the call ended before its band fitted the window) | wave"""
    if qlen > 255 or sc.o_ins + sc.e_ins <= 0:
        return "wave"
    slots = (qlen + 64) >> 6
    if slots == 1:
        return "lean1"
    if slots == 2:
        return "lean2"
    S = f"reg<{slots}>"

    def lean_s(rows, base):
        for r in rows:
            if r.end - base > 127:
                nb = r.beg & ~1
                if r.end - nb > 127:
                    return False
                base = nb
        return True
    if min(qlen, call.w + 1) <= 127:
        return "leanS" if lean_s(call.rows, 0) else "leanS>" + S
    for k, r in enumerate(call.rows):
        if r.end - (r.beg & ~1) <= 127:                         # sw_extend_reg: this row's band fits the sliding sweep's window
            return S + ">leanS" if lean_s(call.rows[k:], r.beg & ~1) else S + ">leanS>" + S
    return S


# ---- a task: decode, band tries, the ten words (csrc/bpsw_extend.hip ext_do_task) -------------------------------------------------
def _i16(b, at):
    return int(np.frombuffer(bytes(b[at:at + 2]), "<i2")[0])


def decode_task(wire, k):
    """task k of a byte batch (wire format 0, MemChainToAlignBatched.scala:76-172)"""
    wire = np.asarray(wire, np.uint8)
    hdr = wire[:8].view(np.int8)
    rec = 32 + 32 * k
    lq, lr, rq, rr = (_i16(wire, rec + 2 * f) for f in range(4))
    pos = int(np.frombuffer(bytes(wire[rec + 8:rec + 12]), "<i4")[0])
    words = wire[4 * pos: 4 * (pos + (lq + lr + rq + rr + 7) // 8)].view("<u4")
    nib = np.zeros(8 * len(words), np.int64)
    for s in range(8):                                          # first base in the most significant nibble
        nib[s::8] = (words >> (28 - 4 * s)) & 15
    seq = {"lq": nib[:lq], "rq": nib[lq:lq + rq], "lr": nib[lq + rq:lq + rq + lr], "rr": nib[lq + rq + lr:lq + rq + lr + rr]}
    return dict(o_del=int(hdr[0]), e_del=int(hdr[1]), o_ins=int(hdr[2]), e_ins=int(hdr[3]), pen_clip5=int(hdr[4]), pen_clip3=int(hdr[5]),
                w=int(hdr[6]), reg_score=_i16(wire, rec + 12), q_beg=_i16(wire, rec + 14), h0=_i16(wire, rec + 16),
                idx=int(np.frombuffer(bytes(wire[rec + 28:rec + 32]), "<i4")[0]),
                max_gap=((max(1, _i16(wire, rec + 20)), max(1, _i16(wire, rec + 22))), (max(1, _i16(wire, rec + 24)), max(1, _i16(wire, rec + 26)))),
                **seq)


@dataclass
class Side:
    tries: list          # the Calls, one per band tried
    widths: list         # wBand << i of each
    same_band: bool      # the retry was not swept: its effective band is the first one's (bpsw_extend.hip:172)
    retry_test: tuple    # (max_off, (aw >> 1) + (aw >> 2), score changed) of the first try
    aw: int              # the band reported for this side
    hinit: int = 0       # the side's start score: h0 on the left, the score so far on the right


def extension(wire, k, sc, tail_bound=True, consts=None):
    """-> (the ten int16 words of task k, [left Side or None, right Side or None])"""
    d = decode_task(wire, k)
    assert (d["o_del"], d["e_del"], d["o_ins"], d["e_ins"], d["w"]) == (sc.o_del, sc.e_del, sc.o_ins, sc.e_ins, sc.w), "the batch was packed with another scoring"
    wband = d["w"]
    reg = d["reg_score"]
    aw_max = wband
    qb, rb, qe, re_, true_sc, score = 0, 0, len(d["rq"]), 0, reg, -1
    sides = [None, None]
    for side in (0, 1):
        q, t = (d["rq"], d["rr"]) if side else (d["lq"], d["lr"])
        if len(q) <= 0:
            continue
        max_ins, max_del = d["max_gap"][side]
        pen = sc.pen_clip3 if side else sc.pen_clip5
        hinit = reg if side else d["h0"]
        sc0 = reg
        s = Side([], [], False, None, wband, hinit)
        for i in range(2):                                      # MAX_BAND_TRY
            prev = reg
            s.aw = wband << i
            w = min(s.aw, max_ins, max_del)
            if i == 1 and w == min(wband, max_ins, max_del):
                s.same_band = True
                break
            call = annotate(sweep(q, t, hinit, sc, w, tail_bound), q, t, tail_bound, consts)
            s.tries.append(call); s.widths.append(s.aw)
            reg = int(call.res[0])
            if i == 0:
                s.retry_test = (int(call.res[5]), (s.aw >> 1) + (s.aw >> 2), reg != prev)
            if reg == prev or call.res[5] < (s.aw >> 1) + (s.aw >> 2):
                break
        sides[side] = s
        r = s.tries[-1].res
        score = reg
        aw_max = max(aw_max, s.aw)
        local = r[4] <= 0 or r[4] <= reg - pen
        if side == 0:
            qb = d["q_beg"] - int(r[1]) if local else 0
            rb = -int(r[2]) if local else -int(r[3])
            true_sc = reg if local else int(r[4])
        else:
            qe = int(r[1]) if local else len(d["rq"])
            re_ = int(r[2]) if local else int(r[3])
            true_sc += (reg if local else int(r[4])) - sc0
    idx = d["idx"]
    out = np.array([idx & 0xFFFF, (idx >> 16) & 0xFFFF, qb, qe, rb, re_, score, true_sc, aw_max, 0], np.int64)
    return out.astype(np.uint16).view(np.int16), sides
