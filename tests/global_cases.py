"""Generated jobs for the banded global alignment (SWUtil.SWGlobal == ksw_global2): one generator for the oracle-versus-reference
test on the CPU (tests/test_oracle_vs_ref.py), the reference fixture (tests/golden/make_golden.py -> ksw_global2_edges.npz) and the
kernel-versus-oracle tests (tests/test_global_gpu.py).  Plain numpy from fixed seeds: no GPU, no oracle.

A job is (q, t, w): query codes, target codes (0..3 bases, 4 = N), band.  Every generated job has w >= |tLen - qLen| except
those of below_band(): neither the reference nor the oracle defines an alignment under a narrower band (they agree on the score
-2^30 only), and bpsw_global_batch refuses such a job.

Device scratch: the library reserves z_per_wave * waves bytes for the direction matrix, z_per_wave = max over the batch of
nCol * tLen rounded up to 256, waves = min(resident waves, jobs rounded up to 4) (scratch_bytes below restates it).  The largest
batch any test here launches is `boundaries` (887 jobs, the largest 1023 x 1093 cells): 1.12 MB * 888 waves = 0.99 GB at 256 CUs;
`edits` takes 0.35 GB, `many` 0.21 GB (25 KB * 8192 resident waves), `limit` (one job of 1023 x 65535) 0.27 GB.  The tests assert
scratch_bytes(...) < 8 GiB before every launch.
"""
import functools
from collections import namedtuple

import numpy as np

Scoring = namedtuple("Scoring", "name mat o_del e_del o_ins e_ins")
Job = namedtuple("Job", "q t w")

MINUS_INF = -0x40000000
WAVES_PER_BLOCK = 4
CIG_LDS = 512


def mat(a, b):
    m = np.full((5, 5), -1, np.int8)
    for i in range(4):
        for j in range(4):
            m[i, j] = a if i == j else -b
    return m.reshape(25)


def _uneven():
    m = mat(1, 4).reshape(5, 5).copy()
    for i, d in enumerate((1, 2, 3, 2)):        # uneven diagonal
        m[i, i] = d
    m[0, 2] = -1                                # one cheaper mismatch, on one side of the diagonal only: a transposed
    m[2, 0] = -2                                # lookup (target row / query column) shows
    m[4, :] = -2; m[:, 4] = -1; m[4, 4] = -3    # an N costs by the side it stands on
    return m.reshape(25)


# (name, matrix, o_del, e_del, o_ins, e_ins)
SCORINGS = (
    Scoring("default", mat(1, 4), 6, 1, 6, 1),
    Scoring("m2x3_g5242", mat(2, 3), 5, 2, 4, 1),
    Scoring("open0", mat(1, 4), 0, 1, 0, 1),
    Scoring("uneven_g3271", _uneven(), 3, 2, 7, 1),
    Scoring("m5x2_g1193", mat(5, 2), 1, 1, 9, 3),
)


def _edit(rng, q, n_edits, max_indel, alphabet=4):
    t = list(int(x) for x in q)
    for _ in range(n_edits):
        p = int(rng.integers(0, max(len(t), 1)))
        r = rng.random()
        k = int(rng.integers(1, max_indel + 1))
        if r < 0.3 and len(t) > 1:
            del t[p:p + min(k, len(t) - 1)]
        elif r < 0.6:
            t[p:p] = rng.integers(0, alphabet, k).tolist()
        elif t:
            t[p] = (t[p] + 1 + int(rng.integers(0, alphabet - 1))) % alphabet
    if not t:
        t = [0]
    return np.array(t, np.uint8)


BOUNDARY_QLENS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 1000, 1023)
BOUNDARY_DS = (-33, -1, 0, 2, 70)
BOUNDARY_WS = (31, 32, 33, 63, 64, 95, 96)


@functools.lru_cache(None)
def boundaries():
    """query lengths at the 64-column chunk edges, targets longer and shorter, bands whose 2w+1 straddles a multiple of 64"""
    rng = np.random.default_rng(20261101)
    out = []
    for ql in BOUNDARY_QLENS:
        q = rng.integers(0, 4, ql).astype(np.uint8)
        for d in BOUNDARY_DS:
            tl = ql + d
            if tl < 1:
                continue
            # the target: the query with |d| bases taken out of / put into one place, and a few substitutions
            p = int(rng.integers(0, ql + 1))
            if d <= 0:
                p = min(p, ql + d)
                t = np.concatenate([q[:p], q[p - d:]])
            else:
                t = np.concatenate([q[:p], rng.integers(0, 4, d).astype(np.uint8), q[p:]])
            t = t.copy()
            for x in rng.integers(0, tl, min(3, tl // 8)):
                t[x] = (t[x] + 1) & 3
            ad = abs(d)
            ws = sorted({w for w in (ad, ad + 1) + BOUNDARY_WS + (ql, 2000) if w >= ad})
            for w in ws:
                out.append(Job(q, t, w))
        out.append(Job(q, q.copy(), 0))                       # w = 0 with equal lengths: the diagonal alone
        t = q.copy(); t[ql // 2] = (t[ql // 2] + 2) & 3
        out.append(Job(q, t, 0))
    return out


@functools.lru_cache(None)
def edits(n=800):
    """random lengths 1-1023, 0-12 edits, indels of up to 40 bases"""
    rng = np.random.default_rng(20261102)
    out = []
    for k in range(n):
        ql = int(rng.integers(1, 1024)) if k % 3 else int(rng.integers(1, 200))
        q = rng.integers(0, 5 if k % 11 == 0 else 4, ql).astype(np.uint8)
        t = _edit(rng, q, int(rng.integers(0, 13)), 40)
        ad = abs(len(t) - ql)
        w = ad + (0 if k % 7 == 0 else int(rng.integers(0, 100)))
        out.append(Job(q, t, w))
    return out


@functools.lru_cache(None)
def ties():
    """inputs on which many alignments share the best score: the direction bits' priority decides the CIGAR"""
    rng = np.random.default_rng(20261103)
    out = []

    def band(q, t, extra):
        return abs(len(t) - len(q)) + extra

    for L in (30, 64, 65, 130, 300):
        for k in (1, 2, 5):
            if k >= L:
                continue
            for base in (0, 3):
                q = np.full(L, base, np.uint8)
                for t in (np.full(L - k, base, np.uint8), np.full(L + k, base, np.uint8)):        # homopolymer: the gap fits anywhere
                    for extra in (0, 3, 40):
                        out.append(Job(q, t, band(q, t, extra)))
                t = np.full(L, base, np.uint8); t[L // 3] = (base + 1) & 3                       # ... with one other base
                t = np.delete(t, 2 * L // 3)
                out.append(Job(q, t, band(q, t, 2)))
        for period in (1, 2, 3, 4):                                                              # tandem repeats: a unit in or out
            unit = rng.permutation(4)[:period].astype(np.uint8) if period > 1 else np.array([rng.integers(0, 4)], np.uint8)
            q = np.tile(unit, L // period + 1)[:L]
            for units in (1, 2):
                k = period * units
                if k >= L:
                    continue
                flank = rng.integers(0, 4, 8).astype(np.uint8)                                   # the repeat between unique flanks
                pairs = [(q, q[:L - k]), (q, np.tile(unit, (L + k) // period + 1)[:L + k]),
                         (np.concatenate([flank, q, flank[::-1]]), np.concatenate([flank, q[:L - k], flank[::-1]]))]
                for qq, t in pairs:
                    for extra in (0, 5, 33):
                        out.append(Job(qq, t, band(qq, t, extra)))
        for n_ed in (1, 3, 6):                                                                   # two letters
            q = rng.integers(0, 2, L).astype(np.uint8) * 3
            t = _edit(rng, q // 3, n_ed, 6, alphabet=2) * 3
            out.append(Job(q, t.astype(np.uint8), band(q, t, 4)))
            out.append(Job(q, t.astype(np.uint8), band(q, t, 64)))
        q = rng.integers(0, 4, L).astype(np.uint8)
        t = _edit(rng, q, 3, 5)
        allN_q, allN_t = np.full(L, 4, np.uint8), np.full(len(t), 4, np.uint8)
        out.append(Job(allN_q, t, band(allN_q, t, 7)))                                           # all-N query
        out.append(Job(q, allN_t, band(q, allN_t, 7)))                                           # all-N target
        out.append(Job(allN_q, allN_t, band(allN_q, allN_t, 0)))
        qn, tn = q.copy(), t.copy()                                                              # about one N per 20 bases
        qn[rng.random(L) < 0.05] = 4
        tn[rng.random(len(t)) < 0.05] = 4
        out.append(Job(qn, tn, band(qn, tn, 10)))
        out.append(Job(qn, t, band(qn, t, 10)))
    return out


@functools.lru_cache(None)
def long_ops():
    """CIGARs of 500-700 operations inside the length limit: one-base insertions every fourth base over the first half of the query,
    one-base deletions every fourth base after it (same-signed neighbours cannot cancel into a run of mismatches), on a query of
    about 1000 bases.  The count depends on the scoring; the tests take it from the oracle and assert that some exceed 512."""
    rng = np.random.default_rng(20261104)
    out = []
    for ql, step, half in ((1000, 4, 0.5), (1023, 4, 0.45), (990, 3, 0.5), (1010, 5, 0.4), (1000, 4, 0.0), (1000, 4, 1.0),
                           (1000, 3, 0.0), (1023, 3, 1.0), (1020, 3, 0.3)):
        q = rng.integers(0, 4, ql).astype(np.uint8)
        t, cut = [], int(ql * half)
        for j in range(ql):
            if j < cut:
                if j % step != step - 1:                   # the query keeps a base the target lacks: an insertion
                    t.append(int(q[j]))
            else:
                t.append(int(q[j]))
                if j % step == step - 1:                   # the target gains a base: a deletion
                    t.append(int((q[j] + 2) & 3))
        t = np.array(t, np.uint8)
        out.append(Job(q, t, abs(len(t) - ql) + 40))
    return out


@functools.lru_cache(None)
def limit():
    """one job at the documented limits: qLen = BPSW_GLOBAL_MAX_QLEN, tLen = BPSW_GLOBAL_MAX_TLEN, the narrowest band allowed"""
    rng = np.random.default_rng(20261105)
    t = rng.integers(0, 4, 65535).astype(np.uint8)
    q = np.concatenate([t[1000:1400], t[30000:30300], t[65535 - 323:]]).copy()
    q[::97] = (q[::97] + 1) & 3
    assert len(q) == 1023
    return [Job(q, t, 65535 - 1023)]


GROUPS = {"boundaries": boundaries, "edits": edits, "ties": ties, "long_ops": long_ops}


def below_band(n=400):
    """w < |tLen - qLen|: outside the domain.  Reference and oracle both return the score -2^30; the CIGARs are not defined."""
    rng = np.random.default_rng(20261106)
    out = []
    for k in range(n):
        ql = int(rng.integers(1, 400))
        q = rng.integers(0, 4, ql).astype(np.uint8)
        d = int(rng.integers(1, 60)) * (1 if k % 2 or ql < 62 else -1)
        tl = max(1, ql + d)
        if tl == ql:
            tl += 1
        t = rng.integers(0, 4, tl).astype(np.uint8)
        out.append(Job(q, t, int(rng.integers(0, abs(tl - ql)))))
    assert all(j.w < abs(len(j.t) - len(j.q)) for j in out)
    return out


@functools.lru_cache(None)
def many(n=20480):
    """short jobs (queries of 1-150 bases, mixed bands) in three orders: more of them than the kernel has resident waves, so every
    wave runs a second and a third job in the LDS its first one left behind, with a longer or a shorter query and a wider or a
    narrower band than before"""
    rng = np.random.default_rng(20261107)
    jobs = []
    for k in range(n):
        ql = int(rng.integers(1, 151))
        q = rng.integers(0, 5 if k % 13 == 0 else 4, ql).astype(np.uint8)
        t = _edit(rng, q, int(rng.integers(0, 5)), 8)
        w = abs(len(t) - ql) + (0, 2, 10, 31, 32, 70, 200)[int(rng.integers(0, 7))]
        jobs.append(Job(q, t, w))
    by_len = sorted(range(n), key=lambda i: (len(jobs[i].q), len(jobs[i].t), jobs[i].w))
    return {"long_to_short": [jobs[i] for i in reversed(by_len)], "short_to_long": [jobs[i] for i in by_len], "shuffled": jobs}


def fixture_subset():
    """the jobs of ksw_global2_edges.npz: a fixed subset of boundaries, ties and long_ops, each under every scoring -> [(job, scoring index)]"""
    b, t, lo = boundaries(), ties(), long_ops()
    picked = [j for j in b if len(j.q) in (1, 63, 64, 65, 128, 129, 257) and j.w in (abs(len(j.t) - len(j.q)), 32, 33, 0, 2000)]
    picked += [j for j in b if len(j.q) == 1023 and len(j.t) in (1023, 1025) and j.w in (2, 96)]
    picked += t[::5]
    picked += lo
    return [(j, s) for j in picked for s in range(len(SCORINGS))]


# --- what the library will ask of the device for a batch (csrc/bpsw_global.hip, bpsw_global_batch) --------------------------------
def lds_per_wave(qcap):
    return (8 * (qcap + 2) + 4 * CIG_LDS + 5 * qcap + 15) & ~15


def resident_waves(num_cu, max_qlen):
    qcap = (max_qlen + 31) & ~31
    per_cu = (160 * 1024) // (lds_per_wave(qcap) * WAVES_PER_BLOCK)
    per_cu = min(8, max(1, per_cu))
    return num_cu * per_cu * WAVES_PER_BLOCK


def n_col(ql, w):
    return min(ql, 2 * w + 1)


def scratch_bytes(jobs, num_cu):
    mz = max(n_col(len(j.q), j.w) * len(j.t) for j in jobs)
    z_per_wave = (mz + 255) & ~255
    started = -(-len(jobs) // WAVES_PER_BLOCK) * WAVES_PER_BLOCK
    return z_per_wave * min(resident_waves(num_cu, max(len(j.q) for j in jobs)), started)
