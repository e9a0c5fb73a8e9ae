"""Test helper (numpy only): the index shapes the seeding kernels are tested on beyond tests/golden/seed_chain_small.npz, their reads
and the option sets -- deterministic, nothing stored.  A genome with a property that chance decides (where `primary` falls) is the
first of np.random.default_rng(0), (1), (2), ... that has it; every genome's property is asserted on the index that
fmi_util.build_index makes of it, so a changed builder cannot quietly lose a case.

Shared by tests/test_smem_plain.py (the plain reference against recordings of the reference), tests/test_seed_index_edges_gpu.py
(the kernels against the plain reference) and tests/golden/make_seed_edges_golden.py (the recordings)."""
import functools
import os

import numpy as np

import fmi_util as fu
import smem_plain

# mem_opt_init's seeding fields (tests/golden/seed_chain_small.npz records them as opt_default_*; test_smem_plain compares)
DEFAULTS = dict(min_seed_len=19, max_occ=10000, split_width=10, max_chain_gap=10000, no_exact=0, split_factor=1.5, chain_drop_ratio=0.5,
                mask_level=0.5)
OPTION_SETS = {
    "defaults": dict(DEFAULTS),
    "every_row": dict(DEFAULTS, min_seed_len=1, max_occ=2**31 - 1, split_width=0),  # every SMEM kept; none emitted twice but an empty one
    "no_exact": dict(DEFAULTS, min_seed_len=10, no_exact=1, split_factor=1.0, split_width=100, max_occ=20),
    "max_occ_0": dict(DEFAULTS, max_occ=0),  # only zero-width intervals are kept: intervals, but no occurrence
}
GENOMES = ("one_block", "tiny", "aligned_p_mid", "aligned_p127", "p_block_start", "p_first", "p_last", "no_cg", "a_only", "runs")
ONE_BASE = [np.array([c], np.uint8) for c in range(4)]  # with every_row: the whole row range of a base


def _primary(fwd) -> int:
    """the row of the whole text among the sorted suffixes, sentinel row included (what build_index calls primary)"""
    t = fu.doubled(fwd).tobytes()
    return 1 + sum(t[i:] < t for i in range(1, len(t)))


def _random(l_pac, want):
    seed = 0
    while True:
        g = np.random.default_rng(seed).integers(0, 4, l_pac).astype(np.uint8)
        if want(_primary(g)):
            return g
        seed += 1


def _make(name):
    if name == "one_block":
        return _random(64, lambda p: True)
    if name == "tiny":
        return _random(10, lambda p: True)
    if name == "aligned_p_mid":
        return _random(192, lambda p: p in (128, 256))
    if name == "aligned_p127":
        return _random(192, lambda p: p % 128 == 127)
    if name == "p_block_start":
        return _random(193, lambda p: p == 128)
    if name == "p_first":
        return _random(100, lambda p: p == 1)
    if name == "p_last":
        return _random(100, lambda p: p == 200)
    if name == "no_cg":
        return (3 * np.random.default_rng(0).integers(0, 2, 300)).astype(np.uint8)
    if name == "a_only":
        return np.zeros(150, np.uint8)
    if name == "runs":
        g = np.random.default_rng(0).integers(0, 4, 1000).astype(np.uint8)
        g[100:400] = 0
        g[500:700] = np.tile(np.array([0, 1], np.uint8), 100)
        return g
    raise KeyError(name)


def _holds(name, g, idx):
    n, p, occ = idx.seq_len, idx.primary, np.diff(idx.L2)
    return {"one_block": n == 128, "tiny": n == 20, "aligned_p_mid": n == 384 and p in (128, 256),
            "aligned_p127": n == 384 and p % 128 == 127, "p_block_start": n == 386 and n % 128 and p == 128,
            "p_first": n == 200 and p == 1, "p_last": n == 200 and p == n,
            "no_cg": n == 600 and occ[1] == 0 and occ[2] == 0 and occ[0] > 0 and occ[3] > 0,
            "a_only": n == 300 and occ[0] == 150 and occ[3] == 150,
            "runs": n == 2000 and not g[100:400].any() and np.array_equal(g[500:700], np.tile(np.array([0, 1], np.uint8), 100))}[name]


@functools.lru_cache(maxsize=None)
def genome(name):
    """-> (bases, full suffix array of the doubled text plus sentinel)"""
    g = _make(name)
    idx, sa = fu.build_index(g, 8)
    assert _holds(name, g, idx), (name, idx.seq_len, idx.primary, idx.L2)
    g.setflags(write=False); sa.setflags(write=False)
    return g, sa


@functools.lru_cache(maxsize=None)
def plain_index(name):
    g, sa = genome(name)
    return smem_plain.PlainIndex(g, sa)


def revcomp(r):
    r = np.asarray(r, np.uint8)[::-1]
    return np.where(r > 3, 4, 3 - r).astype(np.uint8)


def _staircase(ix, n):
    """a read of which every 3-mer occurs in the text and no 4-mer does: an SMEM of three bases starts at every position but the last
    two, so a read of n bases has n - 2 intervals.  Depth-first, smallest base first."""
    def occurs(p):
        return ix.interval(bytes(p), 0, len(p))[2] > 0
    for a in range(64):
        path = [a >> 4, a >> 2 & 3, a & 3]
        if not occurs(path):
            continue
        nxt = [0]
        while nxt and len(path) < n:
            c = nxt[-1]
            if c > 3:  # no base fits here: take back the one before
                nxt.pop()
                if nxt:
                    path.pop(); nxt[-1] += 1
                continue
            if occurs(path[-2:] + [c]) and not occurs(path[-3:] + [c]):
                path.append(c); nxt.append(0)
            else:
                nxt[-1] += 1
        if len(path) == n:
            return np.array(path, np.uint8)
    raise AssertionError("no such read on this text")


def limit_reads():
    """on `runs` (A x 300, (AC) x 100): A x 256, A x 255 + C, C + A x 255, (AC) x 128 -- the interval shrinks with every base, which
    puts the sweep's lists at read_len entries"""
    a = np.zeros(256, np.uint8)
    tail, head = a.copy(), a.copy()
    tail[-1] = 1; head[0] = 1
    return [a, tail, head, np.tile(np.array([0, 1], np.uint8), 128)]


@functools.lru_cache(maxsize=None)
def reads(name):
    """-> tuple of read arrays (codes 0..4); the one-base reads of ONE_BASE are not among them"""
    g, _ = genome(name)
    text = fu.doubled(g)
    n = int(text.size)
    rng = np.random.default_rng(1000 + GENOMES.index(name))
    out = []
    for ln in sorted({min(w, n) for w in (1, 2, 19, 20, 64, 256)}):
        for at in sorted({int(v) for v in np.linspace(0, n - ln, 12)}):  # the first and the last window among them
            w = text[at: at + ln]
            out.append(w.copy())
            if ln >= 19:
                r = w.copy(); r[int(rng.integers(0, ln))] = int(rng.integers(0, 5)); out.append(r)
                r = w.copy(); r[ln // 2] = (r[ln // 2] + int(rng.integers(1, 4))) & 3; out.append(revcomp(r))
    out.append(rng.integers(0, 4, 40).astype(np.uint8))
    out.append(np.full(30, 4, np.uint8))
    if name in ("no_cg", "a_only"):  # a base that does not occur: its zero-width interval runs up to the N (or the end) and is kept
        for c, a, b in ((1, 0, 140), (2, 100, 20), (1, g.size - 30, n - 25)):
            head = np.concatenate([[c], text[a: a + 30]]).astype(np.uint8)
            tail = text[b: b + 25]
            out.append(np.concatenate([head, [4], tail]).astype(np.uint8))   # kept zero-width interval, then kept real ones
            out.append(np.concatenate([tail, [4], head]).astype(np.uint8))   # ... and as the last kept one
    if name == "runs":  # interval lists of read_len entries
        out += limit_reads()
        # reads foreign to the genome: a short SMEM starts at most positions, so the count grows with the length -- from below the
        # first pass's 16 records a read to well above, on more reads than one wavefront has lanes
        for ln in range(20, 56):
            for _ in range(3):
                out.append(rng.integers(0, 4, ln).astype(np.uint8))
    if name == "one_block":
        out.append(_staircase(plain_index(name), 256))  # 254 intervals
        out.append(_staircase(plain_index(name), 19))   # ... and 17
        out.append(_staircase(plain_index(name), 18))   # (shorter than min_seed_len by default)
    for r in out:
        r.setflags(write=False)
    return tuple(out)


def reads_digest(name):
    """of the genome and its reads: the recording says which inputs it was made from"""
    ln, pool = fu.flat(list(reads(name)), np.uint8)
    return smem_plain.digest(np.concatenate([genome(name)[0], ln.view(np.uint8), pool]))


@functools.lru_cache(maxsize=None)
def expected(name, optset, one_base=False):
    """the plain reference on every read of a genome (or on ONE_BASE) -> (list of interval arrays, list of seed arrays)"""
    ix = plain_index(name)
    iv = [smem_plain.intervals(ix, OPTION_SETS[optset], r) for r in (ONE_BASE if one_base else reads(name))]
    sd = [smem_plain.seeds(ix, i) for i in iv]
    for a in iv + sd:
        a.setflags(write=False)
    return iv, sd


RECORDING = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seed_index_edges.npz")


def recording():
    """what the reference's C gave on these cases (tests/golden/make_seed_edges_golden.py): counts and digests per read"""
    return np.load(RECORDING)


def check_recording(rec, key, iv, sd):
    """the counts and digests of one batch's lists (per read) against the recording; a mismatch names the batch and the reads"""
    for what, lists in (("intv", iv), ("seed", sd)):
        cnt = np.array([len(a) for a in lists], np.int32)
        dig = np.array([smem_plain.digest(a) for a in lists], np.uint64)
        assert cnt.shape == rec[f"{key}_{what}_cnt"].shape, (key, what)
        bad = np.nonzero((cnt != rec[f"{key}_{what}_cnt"]) | (dig != rec[f"{key}_{what}_dig"]))[0]
        assert bad.size == 0, f"{key}: the {what} lists of reads {bad.tolist()[:8]} differ from the recording ({bad.size} reads in all)"


def census(name, optset):
    """what the tests need the input to hold, counted on the plain reference's output"""
    iv, sd = expected(name, optset)
    cnt = np.array([len(i) for i in iv])
    c = {"reads": len(iv), "intervals": int(cnt.sum()), "seeds": int(sum(len(s) for s in sd)),
         "n15": int((cnt == 15).sum()), "n16": int((cnt == 16).sum()), "n17": int((cnt == 17).sum()), "n18": int((cnt == 18).sum()),
         "over16": int((cnt > 16).sum()), "max": int(cnt.max()),
         "zero_width": 0, "zero_kept": 0, "zero_before_real": 0, "zero_after_real": 0, "bridging_reads": 0}
    for i, s in zip(iv, sd):
        k = i[i["kept"] != 0]
        z = np.nonzero(k["x2"] == 0)[0]
        real = np.nonzero(k["x2"] > 0)[0]
        c["zero_width"] += int((i["x2"] == 0).sum())
        c["zero_kept"] += z.size
        if z.size and real.size:
            c["zero_before_real"] += bool(z.min() < real.max())
            c["zero_after_real"] += bool(z.max() > real.min())
        c["bridging_reads"] += len(s) < int(k["x2"].sum())
    return c


ROW_LIMIT_BATCH = ("runs", "every_row")  # the batch the tests of the first pass's 16-record rows are made from


def census_failures(table=None):
    """the conditions on the input that the tests rest on -> the ones that do not hold (none, if all is well)"""
    t = table or {(g, o): census(g, o) for g in GENOMES for o in OPTION_SETS}
    bad = []
    row = t[ROW_LIMIT_BATCH]
    if not (row["n15"] and row["n16"] and row["n17"] and row["n18"]):
        bad.append(f"{ROW_LIMIT_BATCH}: no read with exactly 15, 16, 17 and 18 intervals each")
    if row["over16"] <= 64:
        bad.append(f"{ROW_LIMIT_BATCH}: not more than 64 reads with over 16 intervals")
    if not any(c["zero_before_real"] for c in t.values()) or not any(c["zero_after_real"] for c in t.values()):
        bad.append("no kept zero-width interval before a kept non-empty one, or none after")
    if max(c["max"] for c in t.values()) < 200:
        bad.append("no read with 200 intervals or more")
    for g in GENOMES:
        if genome(g)[0].size >= 64 and not any(t[g, o]["bridging_reads"] for o in OPTION_SETS):
            bad.append(f"{g}: no read with a bridging seed")
    if not any(c["intervals"] and not c["seeds"] for (g, o), c in t.items() if o == "max_occ_0"):
        bad.append("max_occ_0: no batch with intervals and no seeds")
    if any(c["seeds"] for (g, o), c in t.items() if o == "max_occ_0"):
        bad.append("max_occ_0: a batch with seeds")
    return bad
