"""The sift kernel's arithmetic on flanks that hold N (csrc/bpsw_extend_sift_core.h: an N column is a deficit column of weight
dn = a - S(N, .), the certificate's W a score) compiled for the HOST (tests/sift_n_host/sift_n_host.cpp) and held against the
oracle's full DP.  No GPU.

  * exactness: every side the twin returns as SIFT_FORM, applied to a start score it accepts, equals the oracle's sw_extend on all
    six fields; every task it flags 1 equals the oracle's record;
  * completeness, the deterministic part: a side with an N, D < oe_min and tLen >= qLen comes back SIFT_FORM with hmin = D + 1.
    (The closed form itself needs D <= zdrop when a z-drop is set -- bpsw_extend_core.h, "so D <= zdrop is required when
    zdrop > 0", the BWA parse compares max - m <= D with it -- so the assertion is made where zdrop is 0 or >= D; a side with
    D > zdrop must NOT come back with that form, and the exactness test would catch one that did.)
  * the count: the tickets (`flag == 2`) of the bench's own batch fall from 11 004 by more than half of the 1 738 N sides with
    D < 7 -- the condition of the change, not its target;
  * the twin as a program of its own under -fsanitize=address,undefined over the exactness set.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bpsw_hip
from bpsw_hip import synth
import pyoracle as po

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "sift_n_host", "sift_n_host.cpp")
HDR = os.path.join(ROOT, "cloud-scale-bwamem_amd", "csrc", "bpsw_extend_sift_core.h")
OUT = os.path.join(HERE, "sift_n_host", "_build")
SIFT_UNSEEN, SIFT_FAIL, SIFT_FORM = 0, 1, 2


def _stale(path):
    return not os.path.exists(path) or os.path.getmtime(path) < max(os.path.getmtime(SRC), os.path.getmtime(HDR))


@pytest.fixture(scope="module")
def twin():
    os.makedirs(OUT, exist_ok=True)
    so = os.path.join(OUT, "libsift_n_host.so")
    if _stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.dirname(HDR), "-o", so, SRC], check=True)
    lib = C.CDLL(so)
    lib.sift_n_host_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_int] * 7 + [C.c_void_p] * 3
    lib.sift_n_host_sides.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]
    lib.sift_n_host_checksum.argtypes = [C.c_void_p, C.c_size_t, C.c_uint64]
    lib.sift_n_host_checksum.restype = C.c_uint64
    return lib


def _levels(mat):
    """exact_match_score / sift_uniform_dm / sift_uniform_dn / certify_level of csrc/bpsw_runtime.cpp"""
    m = np.asarray(mat, np.int64).reshape(5, 5)
    a = int(m[0, 0])
    diag = all(m[i, i] == a for i in range(4))
    others = [m[r, c] for r in range(5) for c in range(5) if not (r == c and r < 4)]
    exact_a = a if (a > 0 and diag and all(v < a for v in others)) else 0
    mm = int(m[0, 1])
    uniform = all(m[i, j] == mm for i in range(4) for j in range(4) if i != j)
    dm = exact_a - mm if (exact_a > 0 and uniform and exact_a - mm > 0) else 0
    sn = int(m[0, 4])
    uniform_n = all(m[i, 4] == sn and m[4, i] == sn for i in range(5))
    dn = exact_a - sn if (exact_a > 0 and uniform_n and exact_a - sn > 0) else 0
    level = 0
    if exact_a > 0:
        level = 3 if (exact_a == 1 and all(v <= -1 for v in others)) else 1
    return exact_a, dm, dn, level


def _mat(a, mm, sn):
    m = np.full((5, 5), sn, np.int8)
    m[:4, :4] = mm
    for i in range(4):
        m[i, i] = a
    return m.reshape(-1)


# the gap costs (oDel, eDel, oIns, eIns), band and z-drop values of tests/test_sift_host.py's adversarial test; 0/3/5/100 as z-drop
GAPS = (((6, 1, 6, 1), 100), ((6, 1, 6, 1), 3), ((1, 1, 1, 1), 100), ((3, 1, 3, 1), 100), ((2, 1, 2, 1), 7), ((3, 2, 7, 1), 2))
ZDROPS = (0, 3, 5, 100)
# the default matrix (dm 5, dn 2); the family with dn above dm (dm 2, dn 4); dn = dm; a match score above 1 (certificate level 1)
MATS = (po.default_mat(), _mat(1, -1, -3), _mat(1, -2, -2), _mat(2, -3, -1))
PER_COMBO = 4200      # x 6 x 4 x 2 combinations = 201 600 flanks


def _flank(rng, serial):
    """one flank with 1..3 N: lengths 1..127, tLen from n - 1 to n + 20, random / homopolymer / tandem-repeat sequence, 0..3
    substitutions, the N in the query, the target or both in one column; placed at column 0, at the last column, next to a
    substitution or at a distance 1..9 from one (`serial` walks through the distances and the placements in turn)"""
    r = rng.random()
    n = int(rng.integers(1, 13)) if r < 0.2 else (int(rng.integers(120, 128)) if r < 0.3 else int(rng.integers(1, 128)))
    t_len = n + int(rng.integers(-1, 21))
    full = max(n, t_len) + 1
    kind = serial % 5
    if kind == 0:                                   # homopolymer
        t = np.full(full, rng.integers(0, 4), np.uint8)
    elif kind == 1:                                 # tandem repeat, period 2..6
        t = np.resize(rng.integers(0, 4, int(rng.integers(2, 7))).astype(np.uint8), full)
    elif kind == 2:                                 # two letters: shifted diagonals match half the time
        t = rng.integers(0, 2, full).astype(np.uint8)
    else:
        t = rng.integers(0, 4, full).astype(np.uint8)
    q = t[:n].copy()
    n_sub = int(rng.integers(0, 4)) if rng.random() < 0.8 else 0
    subs = rng.integers(0, n, n_sub)
    if n_sub and rng.random() < 0.6:
        subs[0] = 0                                 # a flank starts with an error: the seed is a maximal exact match
    for p in subs:
        q[p] = (q[p] + 1 + rng.integers(0, 3)) & 3
    n_n = 1 + (serial // 5) % 3 if rng.random() < 0.7 else 1
    where = (serial // 15) % 4
    cols = []
    for i in range(n_n):
        if i == 0 and where == 0:
            cols.append(0)
        elif i == 0 and where == 1:
            cols.append(n - 1)
        elif i == 0 and n_sub and where == 2:       # at distance d = 0..9 from a substitution, either side (0: on it)
            d = (serial // 60) % 10
            cols.append(int(subs[-1]) + (d if (serial // 600) % 2 else -d))
        else:
            cols.append(int(rng.integers(0, n)))
    for c in cols:
        c = min(max(c, 0), n - 1)
        side = int(rng.integers(0, 3))
        if side != 1:
            q[c] = 4
        if side != 0 and c < t_len:
            t[c] = 4
    if rng.random() < 0.1 and t_len > n:            # an N in the target past the query end: only the shifted diagonals see it
        t[int(rng.integers(n, t_len))] = 4
    return q, t[:max(t_len, 0)]


class _Set:
    """the flanks of one parameter combination and the twin's verdicts"""
    def __init__(self, lib, rng, gaps, w, zdrop, zmode, mat, count):
        self.gaps, self.w, self.zdrop, self.zmode, self.mat = gaps, w, zdrop, zmode, mat
        self.a, self.dm, self.dn, level = _levels(mat)
        self.certify = level
        self.flanks = [_flank(rng, i) for i in range(count)]
        lens = np.array([(q.size, t.size) for q, t in self.flanks], np.int32).reshape(-1)
        off = np.zeros(lens.size, np.int64)
        off[1:] = np.cumsum(lens[:-1])
        self.pool = np.concatenate([x for f in self.flanks for x in f]) if count else np.zeros(0, np.uint8)
        self.len, self.off = lens, off
        self.rec = np.zeros((count, 8), np.int32)
        g = np.array(gaps, np.int32)
        rc = lib.sift_n_host_sides(count, self.pool.ctypes.data, off.ctypes.data, lens.ctypes.data, g.ctypes.data, w, zdrop,
                                   self.certify, self.a, self.dm, self.dn, self.rec.ctypes.data)
        assert rc == 0

    def header(self):
        return np.array([len(self.flanks), self.pool.size, *self.gaps, self.w, self.zdrop, self.certify, self.a, self.dm, self.dn], np.int32)


@pytest.fixture(scope="module")
def exact_sets(twin):
    sets = []
    combo = 0
    for gi, (gaps, w) in enumerate(GAPS):
        for zdrop in ZDROPS:
            for zmode in (po.ZDROP_SCALA, po.ZDROP_BWA):
                rng = np.random.default_rng(77000 + combo)
                sets.append(_Set(twin, rng, gaps, w, zdrop, zmode, MATS[(combo + gi) % len(MATS)], PER_COMBO))
                combo += 1
    return sets


def test_forms_on_flanks_with_n_equal_the_dp(twin, orc, exact_sets):
    """>= 200 000 seeded flanks with 1..3 N: a side returned as SIFT_FORM is the DP's result for every start score >= hmin --
    tried at hmin itself (where the form is sharpest) and at a start score above it"""
    total = forms = 0
    for si, S in enumerate(exact_sets):
        rng = np.random.default_rng(88000 + si)
        oD, eD, oI, eI = S.gaps
        for i, (q, t) in enumerate(S.flanks):
            kind, hmin, max_rel, g_rel, qle, tle, gtle, max_off = (int(v) for v in S.rec[i])
            total += 1
            if kind != SIFT_FORM:
                continue
            forms += 1
            h0 = hmin if i & 1 else hmin + int(rng.integers(1, 120))
            want, _ = orc.sw_extend(q, t, S.mat, oD, eD, oI, eI, S.w, 5, S.zdrop, h0, S.zmode)
            got = (h0 + max_rel, qle, tle, gtle, h0 + g_rel, max_off)
            assert tuple(int(v) for v in want) == got, (si, i, S.gaps, S.w, S.zdrop, S.zmode, h0, q.tolist(), t.tolist(), got, want)
    print(f"exactness: {forms} of {total} flanks with N came back as a form")
    assert total >= 200_000
    assert forms > 0.2 * total          # the set does exercise the forms


def test_a_small_deficit_with_n_is_always_resolved(exact_sets):
    """completeness, the deterministic part (the module's docstring says why the z-drop is in the condition)"""
    seen = 0
    for S in exact_sets:
        m = np.asarray(S.mat, np.int64).reshape(5, 5)
        oe_min = min(S.gaps[0] + S.gaps[1], S.gaps[2] + S.gaps[3])
        for i, (q, t) in enumerate(S.flanks):
            n = q.size
            if t.size < n:
                continue
            D = int((S.a - m[t[:n], q]).sum())
            if D < oe_min and (S.zdrop == 0 or D <= S.zdrop):
                seen += 1
                assert S.rec[i, 0] == SIFT_FORM and S.rec[i, 1] == D + 1, (S.gaps, S.zdrop, q.tolist(), t.tolist(), S.rec[i].tolist(), D)
    assert seen > 20_000


def _run_batch(lib, wire, mat, zdrop, dn_on=True):
    exact_a, dm, dn, level = _levels(mat)
    n = int(np.frombuffer(wire[8:12].tobytes(), "<i4")[0])
    out = np.zeros(10 * max(n, 1), np.int16)
    flag = np.zeros(max(n, 1), np.uint8)
    kinds = np.zeros(2 * max(n, 1), np.uint8)
    w32 = np.ascontiguousarray(wire).view(np.uint32)
    rc = lib.sift_n_host_batch(w32.ctypes.data, w32.size, n, zdrop, level, exact_a, dm, dn if dn_on else 0, 127, out.ctypes.data,
                               flag.ctypes.data, kinds.ctypes.data)
    assert rc == 0
    return out.reshape(-1, 10)[:n], flag[:n], kinds[:2 * n].reshape(-1, 2)


def _resolved_equal(orc, wire, mat, zdrop, zmode, got, flag):
    want = np.asarray(orc.wire_extend(wire, mat, zdrop, zmode)[0]).reshape(-1, 10)
    done = flag == 1
    bad = np.nonzero(done & (got != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {int(done.sum())} resolved tasks differ from the DP; first {bad[:3]}: got {got[bad[:3]]} want {want[bad[:3]]}"
    return int(done.sum())


def test_resolved_tasks_with_n_equal_the_dp(twin, orc):
    """whole tasks (both sides chained, sift_chain) of read-like batches with N in reads and reference"""
    res = tot = 0
    for sub, indel, n_rate in ((0.01, 0.001, 0.002), (0.02, 0.002, 0.02), (0.04, 0.01, 0.005)):
        soa = synth.ext_tasks(5000, read_len=150, sub_rate=sub, indel_rate=indel, n_rate=n_rate, seed=9100 + int(sub * 1e4))
        pool = soa.pool.copy()
        pool[np.random.default_rng(6).random(pool.size) < n_rate] = 4       # N in the target flanks too
        soa.pool = pool
        for (o, e, w) in ((6, 1, 100), (4, 2, 30), (1, 1, 100)):
            soa.o_del = soa.o_ins = o
            soa.e_del = soa.e_ins = e
            soa.w = w
            wire = bpsw_hip.wire_pack(soa)
            for zmode, zdrop in ((po.ZDROP_SCALA, 100), (po.ZDROP_BWA, 10)):
                for mat in (MATS[0], MATS[1]):
                    got, flag, _ = _run_batch(twin, wire, mat, zdrop)
                    res += _resolved_equal(orc, wire, mat, zdrop, zmode, got, flag)
                    tot += flag.size
    assert res > 0.1 * tot


def test_tickets_of_the_bench_batch(twin, orc):
    """the count: bench.py's own first batch of config 3.  Before N columns were judged: 11 004 tickets, 1 738 N sides with D < 7."""
    sys.path.insert(0, ROOT)
    import bench
    soa = bench.make_ext_soa(bench.WORKLOADS[3], 3, 0, 0)
    wire = bpsw_hip.wire_pack(soa)
    mat = po.default_mat()
    got0, flag0, kinds0 = _run_batch(twin, wire, mat, 100, dn_on=False)      # a matrix without a uniform N score: as before
    got, flag, kinds = _run_batch(twin, wire, mat, 100)
    _resolved_equal(orc, wire, mat, 100, po.ZDROP_SCALA, got0, flag0)
    _resolved_equal(orc, wire, mat, 100, po.ZDROP_SCALA, got, flag)
    before, after = int((flag0 == 2).sum()), int((flag == 2).sum())
    print(f"bench batch: {flag.size} tasks, tickets (flag == 2) {before} -> {after}; sides not examined {int((kinds0[flag0 == 2] == SIFT_UNSEEN).sum())} "
          f"-> {int((kinds[flag == 2] == SIFT_UNSEEN).sum())}")
    assert flag.size == 30_311 and before == 11_004
    assert after < 11_004 - 1_738 / 2


def test_the_twin_as_a_program_under_sanitizers(twin, exact_sets, tmp_path):
    """the twin with its own main, built with -fsanitize=address,undefined, run once over the exactness set in a process of its own:
    no report, and the same verdicts (one checksum) as the library the other tests call"""
    exe = os.path.join(OUT, "sift_n_host_san")
    if _stale(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DSIFT_N_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-I" + os.path.dirname(HDR), "-o", exe, SRC], check=True)
    path = tmp_path / "flanks.bin"
    h = 1469598103934665603
    with open(path, "wb") as f:
        for S in exact_sets:
            f.write(S.header().tobytes())
            f.write(S.off.tobytes())
            f.write(S.len.tobytes())
            f.write(S.pool.tobytes())
            h = twin.sift_n_host_checksum(S.rec.ctypes.data, S.rec.size, h)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-2000:])
    total = sum(len(S.flanks) for S in exact_sets)
    assert r.stdout.split() == [str(total), f"{h:016x}"]
