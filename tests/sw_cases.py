"""Named job tables for the mate-rescue local SW (SWUtil.SWAlign2; csrc/bpsw_swalign.hip): one generator for the CPU test that holds
the tables to what their names say (tests/test_sw_cases.py, oracle alone) and for the kernel-versus-oracle tests
(tests/test_swalign_forms_gpu.py).  Plain numpy from fixed seeds: no GPU, no oracle.

A case is (mate, window, q_rev) plus a tag; a Batch is one call of bpsw_swalign2_batch: its cases, its scoring and its xtra word.
Every table is built around constants of csrc/bpsw_swalign.hip, restated below and quoted in the comment of the table that uses
them.  Which kernel a batch runs is decided by launch_sw_kernel / sw_ring_class / the lone-launch rule of csrc/bpsw_sw_runtime.cpp
from the batch's scoring, its longest mate, its longest window, its size and the process's switches; kernel_for() restates that
decision, so that a test can say which form it ran instead of assuming it.

Three things the tables cannot hold, because the ABI does not let them exist:
  * a matrix entry of -253 ("(1, 254) with a matrix minimum of -253"): bpsw_opt_t.mat is int8.  hi + bias == 254 is reached with the
    matrix (126, -128) instead (HI254), its refusing neighbour hi + bias == 255 with (127, -128) (HI255); b == 254, the largest |b|
    the packed form takes (maxScore == 1), and its neighbour b == 255 ride on the matrix (1, -127) (B254, B255);
  * a negative gap cost on the 32-bit form: make_scoring refuses it with BPSW_ERR_ARG before any dispatch (the GPU test asserts that);
  * an entry of the best-score list at te - tmp + g, g > 0, that is not part of the best alignment itself: the alignment gains at most
    `a` per row, so it covers the tmp = ceil(score / a) rows before te.  The left-hand series of second_copy places the partial copy
    first and lets the full copy overwrite its last g rows.
"""
import functools
from collections import namedtuple

import numpy as np

KSW_XBYTE, KSW_XSTOP, KSW_XSUBO, KSW_XSTART = 0x10000, 0x20000, 0x40000, 0x80000      # oracle/pyoracle.py, include/bpsw.h
XTRA = KSW_XSUBO | KSW_XSTART | KSW_XBYTE | 19                                         # MemSamPe.scala:1187-1189

# ---- constants of csrc/bpsw_swalign.hip and include/bpsw.h -------------------------------------------------------------------
PK_TAIL = 7                       # booking lanes behind the last query column
PK_G = PK_TAIL + 1                # rows booked at a time: 8
PK_COLS = 64 - PK_TAIL            # lanes that hold query columns: PK_LAST + 1 = 57; swp_kernel<C> takes mates up to 57 C
PK_TBUF = 256                     # selector words staged per wave at a time
PK_KEYS_LDS_MAX = 1536            # rows whose keys stay in LDS (swp_kernel<C, true>), and the resident kernel's cap for class 5
RESIDENT_ROWS = {3: 1024, 5: PK_KEYS_LDS_MAX}   # swp_resident_key_rows
SW_LANES = 64                     # sw_kernel<C> takes mates up to 64 C
TBUF = 2048                       # target bases staged per wave in sw_kernel
Q4_COLS = 160                     # sw4_kernel: 16 lanes x Q4C = 10 columns
Q4_TBUF = 512                     # target bases staged per job in sw4_kernel
MAX_QLEN, MAX_TLEN = 512, 65535   # BPSW_SW_MAX_QLEN, BPSW_SW_MAX_TLEN
LONE_LAUNCH_MIN = 16              # the lone-launch rule of sw_stage_run: n >= 16

Scoring = namedtuple("Scoring", "name a b o_del e_del o_ins e_ins mat")
Batch = namedtuple("Batch", "name scoring xtra pairs tags")


def mat(a, b, n=-1):
    m = np.full((5, 5), n, np.int8)
    for i in range(4):
        for j in range(4):
            m[i, j] = a if i == j else -b
    return m.reshape(25)


# the general matrix of test_swalign_gpu.py::test_custom_scoring
_GENERAL = np.array([1, -2, -3, -4, -1, -2, 2, -4, -3, 0, -3, -4, 1, -2, -1, -4, -3, -2, 2, -2, -1, 0, -1, -2, -1], np.int8)

DEFAULT = Scoring("default", 1, 4, 6, 1, 6, 1, mat(1, 4))
M5X4 = Scoring("m5x4", 5, 4, 6, 1, 6, 1, mat(5, 4))                  # max(mat) == |b| + 1: H = 255 is consumed; still packed
M2X1 = Scoring("m2x1", 2, 1, 6, 1, 6, 1, mat(2, 1))
M2X3 = Scoring("m2x3_g5241", 2, 3, 5, 2, 4, 1, mat(2, 3))            # o_del + e_del != o_ins + e_ins: SAME_OE false
DEFAULT_G5241 = Scoring("default_g5241", 1, 4, 5, 2, 4, 1, mat(1, 4))   # SAME_OE false, and no cap on a 150-base mate
GENERAL = Scoring("general_g5241", 2, 4, 5, 2, 4, 1, _GENERAL)
HI254 = Scoring("hi126_lo128", 126, 128, 6, 1, 6, 1, mat(126, 128))   # hi + bias == 254: the last scoring the packed form takes
B254 = Scoring("b254", 1, 254, 6, 1, 6, 1, mat(1, 127))              # |b| == 254: maxScore == 1
PACKABLE = (DEFAULT, M5X4, M2X1, M2X3, DEFAULT_G5241, GENERAL, HI254, B254)
# the pack-refusing neighbours: max(mat) == |b| + 2; hi + bias == 255; |b| == 255.  (test_custom_scoring's (5, 2) is a fourth.)
M5X3 = Scoring("m5x3", 5, 3, 6, 1, 6, 1, mat(5, 3))
HI255 = Scoring("hi127_lo128", 127, 128, 6, 1, 6, 1, mat(127, 128))
B255 = Scoring("b255", 1, 255, 6, 1, 6, 1, mat(1, 127))
REFUSING = (M5X3, HI255, B255)


def apply(opt, s: Scoring):
    """fill a bpsw_hip.Opt / pyoracle.Opt (same layout) from a scoring; returns opt"""
    for f in ("a", "b", "o_del", "e_del", "o_ins", "e_ins"):
        setattr(opt, f, getattr(s, f))
    for k in range(25):
        opt.mat[k] = int(s.mat[k])
    return opt


def jobs_from(pairs):
    """(mate, window, q_rev) cases -> the keyword arguments of swalign2_batch: both pools with every job 16-byte aligned"""
    q_len, t_len, q_off, t_off, q_rev, qp, tp = [], [], [], [], [], [], []
    for q, t, rev in pairs:
        q_off.append(len(qp)); t_off.append(len(tp)); q_len.append(len(q)); t_len.append(len(t)); q_rev.append(rev)
        qp.extend(q); tp.extend(t)
        qp.extend([0] * ((-len(qp)) % 16)); tp.extend([0] * ((-len(tp)) % 16))
    return dict(q_len=np.array(q_len, np.int32), t_len=np.array(t_len, np.int32), q_off=np.array(q_off, np.int64),
                t_off=np.array(t_off, np.int64), q_rev=np.array(q_rev, np.uint8), q_pool=np.array(qp + [0] * 16, np.uint8),
                t_pool=np.array(tp + [0] * 16, np.uint8))


# ---- the dispatch of launch_sw_kernel / sw_ring_class / sw_stage_run, restated ----------------------------------------------
def pack_bias(s: Scoring):
    """sw_pack_bias without its switch: the bias of the packed form, or -1 when the scoring does not fit 16-bit halves"""
    lo, hi = min(0, int(s.mat.min())), max(0, int(s.mat.max()))
    if hi > abs(s.b) + 1 or hi - lo > 254 or abs(s.b) > 254 or s.a < 1 or min(s.o_del, s.e_del, s.o_ins, s.e_ins) < 0:
        return -1
    return -lo


def rows64(tlen):
    return (tlen + 63) & ~63        # sw_scratch_bytes_per_wave / 16


def packed_class(qlen):
    return max((qlen + PK_COLS - 1) // PK_COLS, 1)


def sw_class(qlen):
    c = max((qlen + SW_LANES - 1) // SW_LANES, 1)
    return c if c <= 4 else (6 if c <= 6 else 8)


def geometry(batch):
    return len(batch.pairs), max(len(q) for q, _, _ in batch.pairs), max(len(t) for _, t, _ in batch.pairs)


def ring_class(batch, env):
    """sw_ring_class, with the switches of `env` (a mapping like os.environ): 3 or 5, or 0 for a launch"""
    n, mq, mt = geometry(batch)
    if env.get("BPSW_RING", "1") == "0" or env.get("BPSW_SW_PACK", "1") == "0" or int(env.get("BPSW_ZEROCOPY", "7")) & 6 != 6:
        return 0
    if pack_bias(batch.scoring) < 0 or mq > 4 * 64:
        return 0
    c = 3 if packed_class(mq) <= 3 else 5
    return c if rows64(mt) <= RESIDENT_ROWS[c] else 0


def lone_launch(env):
    return int(env.get("BPSW_RING_LONE_LAUNCH", "1")) > 0


def takes_ring(batch, env):
    """whether a LONE caller's batch (nothing else in flight, no extension call for 20 ms) goes through the submission ring"""
    return ring_class(batch, env) != 0 and not (lone_launch(env) and len(batch.pairs) >= LONE_LAUNCH_MIN)


def kernel_for(batch, env, through_ring):
    """the kernel instantiation a batch runs, by name"""
    n, mq, mt = geometry(batch)
    if through_ring:
        return f"swp_resident_kernel<{ring_class(batch, env)}>"
    if env.get("BPSW_SW_PACK", "1") != "0" and pack_bias(batch.scoring) >= 0 and mq <= 256 and mt < 65536 and n > 1:
        kl = rows64(mt) <= PK_KEYS_LDS_MAX and env.get("BPSW_SW_KEYS_LDS", "1") != "0"
        return f"swp_kernel<{packed_class(mq)},{'lds' if kl else 'hbm'}>"
    quad = env.get("BPSW_SW_QUAD")
    # (unset: from 96 jobs per CU on -- 24 576 at 256 CUs; no table here is that large, and the tests assert n < 96 * 64)
    if mq <= Q4_COLS and quad is not None and int(quad) > 0:
        return "sw4_kernel"
    return f"sw_kernel<{sw_class(mq)}>"


# ---- building blocks ---------------------------------------------------------------------------------------------------------
def _r(rng, n, alphabet=(0, 1, 2, 3)):
    return [alphabet[i] for i in rng.integers(0, len(alphabet), n)]


def _rc(q):
    return [3 - b if b < 4 else 4 for b in q[::-1]]


def _noisy(rng, q, sub=0.05, indel=0.01):
    q = np.asarray(q, np.int64)
    out = np.where(rng.random(q.size) < sub, (q + rng.integers(1, 4, q.size)) % 4, q).tolist()
    for p in sorted(np.nonzero(rng.random(q.size) < indel)[0].tolist(), reverse=True):
        if rng.random() < 0.5:
            del out[p]
        else:
            out.insert(p, int(rng.integers(0, 4)))
    return out


def _embed(rng, mate, tlen, second):
    """a window of exactly tlen rows with a noisy copy of the mate at a random offset (cut where the window ends) and, when asked for
    and there is room, a noisy copy of the mate's last two thirds clear of it"""
    w = _r(rng, tlen)
    copy = _noisy(rng, mate)
    off = int(rng.integers(0, max(tlen - len(copy), 0) + 1))
    n = min(len(copy), tlen - off)
    w[off:off + n] = copy[:n]
    if second:
        part = _noisy(rng, mate[len(mate) // 3:])
        m = len(part)
        if off >= m + 4:
            at = int(rng.integers(0, off - m - 3))
        elif off + len(copy) + 4 + m <= tlen:
            at = int(rng.integers(off + len(copy) + 4, tlen - m + 1))
        else:
            at = -1
        if at >= 0:
            w[at:at + m] = part
    return w


def _short_next_to_long(cases):
    """order the cases so that every duo (2k, 2k+1) and every quartet holds the shortest windows left next to the longest"""
    by = sorted(cases, key=lambda c: (len(c[0][1]), len(c[0][0])))
    out = []
    lo, hi = 0, len(by) - 1
    while lo <= hi:
        out.append(by[hi]); hi -= 1
        if lo <= hi:
            out.append(by[lo]); lo += 1
    return out


def _batch(name, scoring, xtra, cases):
    return Batch(name, scoring, xtra, [c[0] for c in cases], [c[1] for c in cases])


def with_scoring(batch, scoring, xtra=None):
    return Batch(batch.name, scoring, batch.xtra if xtra is None else xtra, batch.pairs, batch.tags)


def chunks(batch, sizes=(13, 14, 15)):
    """the batch again as batches below the lone-launch size, n = 1, 2, 3 (mod 4) in turn: what a lone caller sends through the ring"""
    out, at, k = [], 0, 0
    while at < len(batch.pairs):
        n = sizes[k % len(sizes)]
        out.append(Batch(f"{batch.name}[{at}:{at + n}]", batch.scoring, batch.xtra, batch.pairs[at:at + n], batch.tags[at:at + n]))
        at += n; k += 1
    return out


# ---- length_cases ------------------------------------------------------------------------------------------------------------
# mates around every multiple of PK_COLS = 57 (the packed class switches, C = 1..5) up to 256 = the packed form's last mate;
# windows 0..17 (maxsteps rounding to PK_G = 8, which rows the tail lanes hold), PK_TBUF = 256 +- 1, twice that, and ~700
PACKED_MATES = (1, 56, 57, 58, 113, 114, 115, 170, 171, 172, 227, 228, 229, 255, 256)
PACKED_WINDOWS = tuple(range(18)) + (255, 256, 257, 511, 512, 513, 701)
# mates around every multiple of SW_LANES = 64 (sw_kernel<1|2|3|4|6|8>) up to MAX_QLEN = 512; windows around TBUF = 2048 and two blocks
SW32_MATES = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 384, 385, 448, 512)
SW32_WINDOWS = tuple(range(18)) + (2047, 2048, 2049, 4100)
# mates around Q4C = 10 columns per lane and up to Q4_COLS = 160; windows around Q4_TBUF = 512 and 2 x 512 + 1
QUAD_MATES = (1, 10, 11) + tuple(range(149, 161))
QUAD_WINDOWS = tuple(range(18)) + (511, 512, 513, 1025)


def _length_cases(seed, mates, windows):
    rng = np.random.default_rng(seed)
    cases = []
    for tlen in windows:
        for ql in mates:
            k = len(cases)
            mate = _r(rng, ql)
            w = _embed(rng, mate, tlen, second=k % 3 == 0)         # every third case: a partial second copy
            rev = int(k % 5 == 0)                                  # every fifth: the mate is stored reverse-complemented
            cases.append(((_rc(mate) if rev else mate, w, rev), ("length", ql, tlen)))
    return cases


@functools.lru_cache(None)
def length_cases(form):
    """form 'packed': one batch per class C = 1..5 (the batch's longest mate is 57 C), n = 75 = 3 (mod 4);
    'sw32': one batch per sw_kernel instantiation 1, 2, 3, 4, 6, 8 (longest mate 64 C), n = 66 = 2 (mod 4), and a lone job (n == 1
    never takes the packed form); 'quad': three batches with n = 109, 110, 111 = 1, 2, 3 (mod 4)"""
    out = []
    if form == "packed":
        for c in range(1, 6):
            mates = [m for m in PACKED_MATES if packed_class(m) == c]
            out.append(_batch(f"len_packed_c{c}", DEFAULT, XTRA, _short_next_to_long(_length_cases(100 + c, mates, PACKED_WINDOWS))))
            assert geometry(out[-1])[1] == min(PK_COLS * c, 256) and len(out[-1].pairs) % 4 == 3
    elif form == "sw32":
        for c in (1, 2, 3, 4, 6, 8):
            mates = [m for m in SW32_MATES if sw_class(m) == c]
            out.append(_batch(f"len_sw32_c{c}", DEFAULT, XTRA, _short_next_to_long(_length_cases(200 + c, mates, SW32_WINDOWS))))
            assert geometry(out[-1])[1] == SW_LANES * c and len(out[-1].pairs) % 4 == 2
        one = out[2]
        out.append(Batch("len_sw32_lone_job", DEFAULT, XTRA, one.pairs[:1], one.tags[:1]))
    elif form == "quad":
        cases = _length_cases(300, QUAD_MATES, QUAD_WINDOWS)
        groups = [cases[k::3] for k in range(3)]       # every window length in each of them
        groups[2].append(groups[0].pop())
        assert [len(g) for g in groups] == [109, 110, 111]
        for k, g in enumerate(groups):
            out.append(_batch(f"len_quad_{k}", DEFAULT, XTRA, _short_next_to_long(g)))
    else:
        raise ValueError(form)
    return tuple(out)


# ---- second_best_cases -------------------------------------------------------------------------------------------------------
PLATEAU_P = tuple(range(141))
PLATEAU_K = (20, 40)


def plateau_start(p):
    return 55 + p % 16              # the run starts at rows 55..70: its hot rows cross the 64-row chunks of second_best and their carry


def _plateau(k, p):
    """mate = A^k + 30 of C/G, window = T^s + A^(k+p) + T^40: the row maximum climbs to k at row s + k - 1 and stays there for p more
    rows -- one list entry every other row (the parity chain), the first one beyond te + tmp = s + 2k - 1 being the second best"""
    rng = np.random.default_rng(1000 * k + p)
    return ([0] * k + _r(rng, 30, (1, 2)), [3] * plateau_start(p) + [0] * (k + p) + [3] * 40, 0), ("plateau", k, p)


COPY2_MATES = (100, 60, 120)
COPY2_G = tuple(range(-3, 4))
COPY2_PART = 40


def _second_copy(length, side, g):
    """M2X3 (a = 2: tmp = score / 2 != score): an exact copy of the mate ends at row te; the last 40 bases of the mate once more, ending
    at te + tmp + g (side +1) or te - tmp + g (side -1; the full copy is written over it where they meet).  Window noise is T, the mate
    has none: nothing else scores."""
    rng = np.random.default_rng(7000 + length)          # one mate per series: only the placement differs
    mate = _r(rng, length, (0, 1, 2))
    start = 160
    w = [3] * (start + 2 * length + 80)
    te, tmp = start + length - 1, length
    end = te + side * tmp + g
    w[end - COPY2_PART + 1:end + 1] = mate[-COPY2_PART:]
    w[start:start + length] = mate
    return (mate, w, 0), ("copy2", length, side, g)


THRESHOLDS = (1, 30, 60)


def _threshold(s, d):
    """default scoring, XSUBO | s: a full copy, and 200 rows after its end an exact copy of s + d bases (d = -1, 0, +1) between T rows"""
    rng = np.random.default_rng(8000 + 10 * s + d)
    mate = _r(rng, 150, (0, 1, 2))
    w = [3] * 100 + mate + [3] * 400              # te = 249, tmp = 150: the exclusion window ends at row 399
    n = s + d
    if n > 0:
        w[450:450 + n] = mate[40:40 + n]
    return (mate, w, 0), ("threshold", s, d)


@functools.lru_cache(None)
def second_best_cases():
    out = [_batch("sb_plateau", DEFAULT, XTRA, [_plateau(k, p) for p in PLATEAU_P for k in PLATEAU_K])]
    # the same plateaus at the ends of the threshold's range: every row hot (0, 1), none (256, 0xffff)
    few = [_plateau(k, p) for p in (0, 7, 8, 9, 63, 64, 65, 127, 128, 140) for k in PLATEAU_K]
    for s in (0, 1, 256, 0xffff):
        out.append(_batch(f"sb_plateau_thr{s}", DEFAULT, KSW_XSUBO | KSW_XSTART | s, few))
    out.append(_batch("sb_copy2", M2X3, KSW_XSUBO | KSW_XSTART | 38, [_second_copy(length, side, g) for length in COPY2_MATES for side in (1, -1) for g in COPY2_G]))
    for s in THRESHOLDS:
        out.append(_batch(f"sb_threshold{s}", DEFAULT, KSW_XSUBO | KSW_XSTART | s, [_threshold(s, d) for d in (-1, 0, 1)]))
    rep = []
    for length in (PK_COLS, 2 * PK_COLS, 3 * PK_COLS):      # every row of a repeat scores: the longest lists there are
        di = ([0, 1] * length)[:length]
        rep.append((([0] * length, [0] * (4 * length + 3), 0), ("homopolymer", length)))
        rep.append(((di, [0, 1] * (2 * length + 2), 0), ("dinucleotide", length)))
        rep.append(((di, [1, 0] * (2 * length) + [1], 1), ("dinucleotide_rev", length)))
    out.append(_batch("sb_repeats", DEFAULT, XTRA, rep))
    return tuple(out)


# ---- stop_cases --------------------------------------------------------------------------------------------------------------
STOP_SCORES = (0, 1, 30, 254)
STOP_OFFSETS = tuple(range(40, 56))       # sixteen consecutive rows: every booking lane of a PK_G = 8 group, whatever the pipe depth D


def _stop(s, off, mate_len):
    """an exact copy from row `off` on: the row maximum is i + 1 at row off + i, so it reaches s first at r = off + s - 1 and the
    PK_G - 1 rows after it (other booking lanes of the same group) reach it too; the earliest row wins.  T rows before it."""
    rng = np.random.default_rng(9000 + 100 * s + off + mate_len)
    mate = _r(rng, mate_len, (0, 1, 2))
    stop = min(s, 255 - DEFAULT.b)            # SWUtil.scala:537: the cap stops a pass too
    r = 0 if s == 0 else off + stop - 1
    return (mate, [3] * off + mate + [3] * 40, 0), ("stop", s, r)


def _capped(rng):
    mate = _r(rng, 256)
    return (mate, _r(rng, 5) + mate + _r(rng, 30), 0), ("capped",)


def _uncapped(rng):
    mate = _r(rng, 150)
    return (mate, _r(rng, 520) + _noisy(rng, mate, 0.03, 0.0) + _r(rng, 30), 0), ("uncapped",)


@functools.lru_cache(None)
def stop_cases():
    out = []
    for start in (0, KSW_XSTART):
        tag = "_start" if start else ""
        for s in STOP_SCORES:
            for ql in (256,) if s == 254 else (150, 256):      # (a batch per mate length: the 150-base ones fit the quad form)
                out.append(_batch(f"stop{s}_q{ql}{tag}", DEFAULT, start | KSW_XSTOP | s, [_stop(s, off, ql) for off in STOP_OFFSETS]))
    rng = np.random.default_rng(77)
    duos = []
    for k in range(6):   # one job of a duo capped at row ~255, its partner running on for 700 rows: in both orders
        duos += [_capped(rng), _uncapped(rng)] if k % 2 == 0 else [_uncapped(rng), _capped(rng)]
    out.append(_batch("stop_duo_cap", DEFAULT, XTRA, duos))
    return tuple(out)


# ---- n_cases -----------------------------------------------------------------------------------------------------------------
# a window row is staged PK_TBUF = 256 selector words at a time; row x is word x - L0 (L0 = 7 for a 150-base mate in class 3), so
# rows 240..272 and 496..528 put the one N of a window on every word around the first and the second block edge
N_ROWS = tuple(range(240, 273)) + tuple(range(496, 529))
N_WINDOW = 900


def _n_window(rng, mate, n_rows):
    w = _r(rng, N_WINDOW)
    first = n_rows[0] if n_rows else int(rng.integers(200, 600))
    off = max(first - 75, 0)
    copy = _noisy(rng, mate, 0.03, 0.0)
    w[off:off + len(copy)] = copy
    part = mate[-60:]
    at = off + 260 if off + 260 + 60 <= N_WINDOW else off - 200
    w[at:at + 60] = part
    for x in n_rows:
        w[x] = 4
    return w


@functools.lru_cache(None)
def n_cases():
    rng = np.random.default_rng(31)
    cases = []
    for x in N_ROWS:                                  # duos (2k, 2k+1): the N in job A only, in job B only, in both
        for where in ((1, 0), (0, 1), (1, 1)):
            for has in where:
                mate = _r(rng, 150)
                cases.append(((mate, _n_window(rng, mate, (x,) if has else ()), 0), ("n", x, has)))
    for x in (250, 255, 256, 300):                    # two N exactly PK_TBUF and PK_TBUF + 1 rows apart
        for d in (PK_TBUF, PK_TBUF + 1):
            mate = _r(rng, 150)
            cases.append(((mate, _n_window(rng, mate, (x, x + d)), 0), ("n2", x, d)))
    for k in range(10):                               # N in the mate
        mate = _r(rng, 150)
        clean = list(mate)
        mate[(17 * k) % 150] = 4
        cases.append(((_rc(mate) if k % 2 else mate, _n_window(rng, clean, (250 + k,) if k % 2 else ()), k % 2), ("n_mate", k)))
    assert len(cases) % 2 == 0
    b = _batch("n_one", DEFAULT, XTRA, cases)
    # SAME_OE false combined with N; and two scorings under which the patched step runs into the cap (M5X4: with H = 255 consumed)
    return (b, with_scoring(b, DEFAULT_G5241), with_scoring(b, M5X4), with_scoring(b, M2X1))


# ---- scoring_cases -----------------------------------------------------------------------------------------------------------
M5X4_MATES = (49, 50, 51, 120)            # exact copies: 245, 250 and twice the cap (51 x 5 = 255 >= maxScore = 251)


def _scoring_jobs():
    rng = np.random.default_rng(55)
    cases = []
    for ql in M5X4_MATES:
        mate = _r(rng, ql, (0, 1, 2))
        cases.append(((mate, [3] * 33 + mate + [3] * 47, 0), ("exact", ql)))
    for k in range(96):
        ql = (150, 100, 250, 57, 171, 20)[k % 6]
        mate = _r(rng, ql)
        cases.append(((mate, _embed(rng, mate, 300 + 7 * k, second=k % 2 == 0), k % 2), ("noisy", ql)))
    return cases


@functools.lru_cache(None)
def scoring_cases():
    """a hundred jobs under every packable scoring and every pack-refusing neighbour; the first four are the exact copies of M5X4_MATES"""
    cases = _scoring_jobs()
    return tuple(_batch("scoring", s, XTRA, cases) for s in PACKABLE + REFUSING)


# ---- ends_in_first_columns ---------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def ends_in_first_columns():
    """per class C = 1..5: best alignments that end in query column qe = 0..C -- the second pass runs on qe + 1 <= C columns, all of them
    in lane PK_LAST, pipe depth D = 0 (qe == C: the first that needs a second lane).  mate = A^(qe+1) + G^rest, the window C's with one
    run of A's; the partner of every other duo is an ordinary 700-row job."""
    out = []
    for c in range(1, 6):
        rng = np.random.default_rng(600 + c)
        top = min(PK_COLS * c, 256)
        cases = []
        for qe in range(c + 1):
            for pre in (0, 1, 9, 300):
                ql = top if pre == 0 else max(top - 20, qe + 1)
                cases.append((([0] * (qe + 1) + [2] * (ql - qe - 1), [1] * pre + [0] * (qe + 1) + [1] * 11, 0), ("ends", qe)))
                if pre in (1, 300):
                    mate = _r(rng, top)
                    cases.append(((mate, _embed(rng, mate, 700, second=False), 0), ("partner",)))
        if len(cases) % 2 == 0:
            cases.append((([0], [1, 0], 0), ("ends", 0)))
        out.append(_batch(f"ends_c{c}", DEFAULT, KSW_XSUBO | KSW_XSTART | 1, cases))
    return tuple(out)


# ---- the window-length edges of the key placement ----------------------------------------------------------------------------
KEY_EDGES = ((5, PK_KEYS_LDS_MAX), (5, PK_KEYS_LDS_MAX + 1), (3, RESIDENT_ROWS[3]), (3, RESIDENT_ROWS[3] + 1),
             (3, PK_KEYS_LDS_MAX), (3, PK_KEYS_LDS_MAX + 1))


@functools.lru_cache(None)
def key_edge_cases():
    """class-5 batches whose longest window has 1536 / 1537 rows (keys in LDS / in HBM; the resident kernel's cap for class 5), class-3
    batches at 1024 / 1025 (the resident kernel's cap: ring / launch) and 1536 / 1537; each with n = 9 (below the lone-launch size) and
    n = 17.  The longest window carries its copy in its last rows: the last key row is read."""
    out = []
    for c, rows in KEY_EDGES:
        rng = np.random.default_rng(rows * 10 + c)
        top = min(PK_COLS * c, 256) - 7
        for n in (9, 17):
            cases = []
            for k in range(n):
                mate = _r(rng, top if k < 2 else int(rng.integers(PK_COLS * (c - 1) + 1, top)))
                if k == 1:
                    body = mate[-50:] + _r(rng, 10) + mate
                    w = _r(rng, rows - len(body)) + body
                else:
                    w = _embed(rng, mate, int(rng.integers(1, rows)), second=k % 2 == 0)
                cases.append(((mate, w, 0), ("edge", c, rows)))
            out.append(_batch(f"keys_c{c}_rows{rows}_n{n}", DEFAULT, XTRA, cases))
            assert geometry(out[-1]) == (n, top, rows)
    return tuple(out)


# ---- the longest window ------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def longest_window(mate_len):
    """four jobs with MAX_TLEN = 65 535 rows: a copy that ends in the last row (te = 65 534) with a partial copy around row 300 (te2),
    the same the other way round, a copy across row 32 768, and a reverse-complemented mate whose copy ends in the last row: the
    16-bit row fields at both ends.  mate_len <= 256: packed, keys in HBM; 300: sw_kernel<6>."""
    rng = np.random.default_rng(65535 + mate_len)
    cases = []
    for k in range(4):
        mate = _r(rng, mate_len)
        w = rng.integers(0, 4, MAX_TLEN).tolist()
        copy = _noisy(rng, mate[:-30], 0.04 if mate_len <= 240 else 0.09, 0.0) + mate[-30:]     # (its last rows exact: te is the last row)
        part = mate[-100:]
        if k in (0, 3):
            w[MAX_TLEN - len(copy):] = copy
            w[300 - len(part):300] = part
        elif k == 1:
            w[MAX_TLEN - len(part):] = part
            w[330 - len(copy):330] = copy
        else:
            w[32768 - 100:32768 - 100 + len(copy)] = copy
        cases.append(((_rc(mate) if k == 3 else mate, w, int(k == 3)), ("longest", k)))
    return _batch(f"longest_q{mate_len}", DEFAULT, XTRA, cases)


# ---- reduced failures ------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def reduced_cases():
    """the smallest form of what a table found: sw4_kernel booked row 0 of an EMPTY window for a mate of up to Q4C = 10 bases (its
    last column in lane 0 of the job's row, so the row 'left the pipe' at step 0) whenever another job of the quartet had rows --
    score 0 / te 0 instead of no alignment.  (len_quad_0, job 1.)"""
    rng = np.random.default_rng(4)
    mate = _r(rng, 150)
    cases = [((mate, _r(rng, 40) + mate + _r(rng, 20), 0), ("partner",))]
    cases += [((_r(rng, ql), [], 0), ("empty_window", ql)) for ql in (1, 10, 11)]
    return (_batch("quad_empty_window_short_mate", DEFAULT, XTRA, cases), _batch("quad_empty_window_short_mate", M5X3, XTRA, cases))


# ---- everything --------------------------------------------------------------------------------------------------------------
PACKED_TABLE_SCORINGS = (M5X4, M2X1)       # the packed length table runs under these as well (most of their jobs reach the cap)


@functools.lru_cache(None)
def all_batches():
    """every batch the GPU tests run, once (the chunked and re-ordered forms of a batch hold the same jobs and are not repeated)"""
    out = []
    for form in ("packed", "sw32", "quad"):
        out += length_cases(form)
    out += [with_scoring(b, s) for b in length_cases("packed") for s in PACKED_TABLE_SCORINGS]
    out += [with_scoring(b, M5X3) for b in length_cases("sw32")]
    out += second_best_cases() + stop_cases() + n_cases() + scoring_cases() + ends_in_first_columns() + key_edge_cases()
    out += [longest_window(240), longest_window(300)]
    out += reduced_cases()
    return tuple(out)


_WANT = {}


def want(orc, batch):
    """the oracle's (n, 7) result of a batch, computed once per process"""
    key = (batch.name, batch.scoring.name, batch.xtra)
    if key not in _WANT:
        res = orc.sw_align2_jobs(apply(orc.default_opt(), batch.scoring), batch.xtra, **jobs_from(batch.pairs))[0]
        res.setflags(write=False)
        _WANT[key] = res
    return _WANT[key]
