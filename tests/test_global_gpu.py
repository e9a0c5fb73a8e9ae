"""HIP banded global alignment + CIGAR (SWUtil.SWGlobal, SWUtil.scala:233-397) against the ksw_global2 golden
vectors (reference C) and against the oracle restatement on seeded and edge-case jobs.  Bit-exact score and CIGAR.

The second half runs the generated cases of tests/global_cases.py: five scorings, query lengths and bands at the 64-column chunk
edges and at the documented limits, tie-rich sequences, CIGARs at and beyond the kernel's staging of 512 operations, and batches
of more jobs than the kernel has resident waves (so that a wave's LDS is reused by a second and a third job)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import bpsw_hip
import global_cases
import pyoracle as po

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAT = po.default_mat()


def _run(ctx, qs, ts, ws, max_cigar=128, opt=None):
    q_off, t_off, qp, tp, qat, tat = [], [], [], [], 0, 0
    for q, t in zip(qs, ts):
        q_off.append(qat); t_off.append(tat)
        qat += len(q) + (-len(q)) % 16; tat += len(t) + (-len(t)) % 16
        qp.append(np.concatenate([np.asarray(q, np.uint8), np.zeros((-len(q)) % 16, np.uint8)]))
        tp.append(np.concatenate([np.asarray(t, np.uint8), np.zeros((-len(t)) % 16, np.uint8)]))
    return ctx.global_batch(opt or bpsw_hip.default_opt(), [len(q) for q in qs], [len(t) for t in ts], ws, q_off, t_off,
                            np.concatenate(qp + [np.zeros(16, np.uint8)]), np.concatenate(tp + [np.zeros(16, np.uint8)]), max_cigar)


def test_vs_ksw_global2_golden(ctx):
    z = np.load(os.path.join(G, "ksw_global2.npz"))
    qs = [z["q_pool"][z["q_off"][i]:z["q_off"][i + 1]] for i in range(len(z["w"]))]
    ts = [z["t_pool"][z["t_off"][i]:z["t_off"][i + 1]] for i in range(len(z["w"]))]
    score, ncig, cig = _run(ctx, qs, ts, z["w"])
    assert np.array_equal(score, z["score"])
    for i in range(len(qs)):
        want = z["cig_pool"][z["cig_off"][i]:z["cig_off"][i + 1]]
        assert ncig[i] == len(want) and np.array_equal(cig[i, : ncig[i]], want), i


def test_vs_oracle_seeded_and_edges(ctx, orc):
    rng = np.random.default_rng(8)
    qs, ts, ws = [], [], []
    for n in range(300):
        ql = int(rng.integers(1, 300))
        q = rng.integers(0, 5 if n % 11 == 0 else 4, ql).astype(np.uint8)
        t = list(q)
        for _ in range(int(rng.integers(0, 6))):          # a few indels / substitutions
            p = int(rng.integers(0, max(len(t), 1)))
            r = rng.random()
            if r < 0.3 and len(t) > 1:
                del t[p:p + int(rng.integers(1, 6))]
            elif r < 0.6:
                t[p:p] = rng.integers(0, 4, int(rng.integers(1, 6))).tolist()
            elif len(t):
                t[p] = (t[p] + 1) % 4
        if not t:
            t = [0]
        w = abs(len(t) - ql) + int(rng.integers(0, 50)) + (3 if n % 5 else 0)
        qs.append(q); ts.append(np.array(t, np.uint8)); ws.append(w)
    # edges: band wider than the query (nCol = qLen), w = 0 with equal lengths, one-base sequences, long target
    q = rng.integers(0, 4, 40).astype(np.uint8)
    qs += [q, q, np.array([2], np.uint8), q[:5], rng.integers(0, 4, 150).astype(np.uint8)]
    ts += [q, q, np.array([2], np.uint8), rng.integers(0, 4, 60).astype(np.uint8), rng.integers(0, 4, 400).astype(np.uint8)]
    ws += [100, 0, 3, 60, 260]
    score, ncig, cig = _run(ctx, qs, ts, ws, max_cigar=512)
    for i, (q, t, w) in enumerate(zip(qs, ts, ws)):
        ws_, wc = orc.sw_global(q, t, MAT, 6, 1, 6, 1, int(w))
        assert score[i] == ws_, (i, score[i], ws_)
        assert ncig[i] == len(wc) and np.array_equal(cig[i, : ncig[i]], wc), (i, cig[i, : ncig[i]], wc)


def test_cigar_capacity_is_reported_not_truncated_silently(ctx, orc):
    q = np.array([0, 1] * 30, np.uint8)
    t = np.concatenate([q[:10], [3, 3, 3], q[10:20], q[25:40], [3, 3], q[40:]]).astype(np.uint8)
    ws_, wc = orc.sw_global(q, t, MAT, 6, 1, 6, 1, 20)
    score, ncig, cig = _run(ctx, [q], [t], [20], max_cigar=2)
    assert score[0] == ws_ and ncig[0] == len(wc) and len(wc) > 2        # count reported, caller must resubmit
    score, ncig, cig = _run(ctx, [q], [t], [20], max_cigar=64)
    assert np.array_equal(cig[0, : ncig[0]], wc)


# ---- the generated cases (tests/global_cases.py) ----------------------------------------------------------------------------------
GIB8 = 8 << 30


def _opt(s):
    o = bpsw_hip.default_opt()
    o.a, o.b = int(max(s.mat[k * 6] for k in range(4))), int(-min(s.mat[:24]))
    o.o_del, o.e_del, o.o_ins, o.e_ins = s.o_del, s.e_del, s.o_ins, s.e_ins
    for k in range(25):
        o.mat[k] = int(s.mat[k])
    return o


def _oracle(orc, jobs, s):
    with ThreadPoolExecutor(16) as pool:      # (ctypes releases the GIL during the call)
        return list(pool.map(lambda j: orc.sw_global(j.q, j.t, s.mat, s.o_del, s.e_del, s.o_ins, s.e_ins, int(j.w)), jobs))


def _launch(ctx, jobs, s, max_cigar):
    assert all(j.w >= abs(len(j.t) - len(j.q)) for j in jobs)                     # in-domain, every one: nothing is filtered
    assert global_cases.scratch_bytes(jobs, ctx.num_cu()) < GIB8                       # (the machines are shared)
    return _run(ctx, [j.q for j in jobs], [j.t for j in jobs], [j.w for j in jobs], max_cigar=max_cigar, opt=_opt(s))


def _same(got, want, max_cigar, label):
    """score and true operation count of every job; the words exactly when they fit, else the row as the harness zeroed it"""
    score, ncig, cig = got
    assert len(score) == len(want)
    for i, (ws_, wc) in enumerate(want):
        assert score[i] == ws_, (label, i, score[i], ws_)
        assert ncig[i] == len(wc), (label, i, ncig[i], len(wc))
        if len(wc) <= max_cigar:
            assert np.array_equal(cig[i, : len(wc)], wc) and not cig[i, len(wc):].any(), (label, i, cig[i, : len(wc) + 2], wc)
        else:
            assert not cig[i].any(), (label, i, "a CIGAR that did not fit was written")
    return len(want)


@pytest.mark.parametrize("s", global_cases.SCORINGS, ids=[s.name for s in global_cases.SCORINGS])
@pytest.mark.parametrize("group", list(global_cases.GROUPS))
def test_generated_groups_vs_oracle(ctx, orc, group, s):
    """boundaries / edits / ties / long_ops under every scoring: score, count and every CIGAR word against the oracle"""
    jobs = global_cases.GROUPS[group]()
    want = _oracle(orc, jobs, s)
    n = _same(_launch(ctx, jobs, s, 512), want, 512, (group, s.name))
    over = sum(len(wc) > 512 for _, wc in want)
    print(f"{group} x {s.name}: {n} jobs compared, longest CIGAR {max(len(wc) for _, wc in want)}, {over} beyond 512 operations")
    assert n == len(jobs) and n >= (9 if group == "long_ops" else 600)


def test_long_ops_reach_and_pass_the_staging_limit(orc):
    """the long_ops group is what it says, by the oracle's count: CIGARs of 500-700 operations, some beyond the 512 the kernel stages"""
    counts = [len(wc) for s in global_cases.SCORINGS for _, wc in _oracle(orc, global_cases.long_ops(), s)]
    assert sum(500 <= c <= 700 for c in counts) >= 4 and sum(c > 512 for c in counts) >= 3, counts


def test_one_job_at_the_documented_limits(ctx, orc):
    """q_len = BPSW_GLOBAL_MAX_QLEN against t_len = BPSW_GLOBAL_MAX_TLEN under the narrowest band the rule allows, alone in its batch:
    the scratch is sized by the waves the launch starts (4 x 67 MB), not by every resident wave (about 2000 x 67 MB)"""
    jobs = global_cases.limit()
    assert (len(jobs[0].q), len(jobs[0].t)) == (1023, 65535)
    for s in (global_cases.SCORINGS[0], global_cases.SCORINGS[3]):
        _same(_launch(ctx, jobs, s, 512), _oracle(orc, jobs, s), 512, ("limit", s.name))


@pytest.mark.parametrize("order,si", [("long_to_short", 0), ("short_to_long", 1), ("shuffled", 3)])
def test_more_jobs_than_resident_waves(ctx, orc, order, si):
    """Grid-stride reuse: 20 480 short jobs in one launch, more than the waves the launch can start, so every wave runs two or three
    jobs in the same LDS row, query profile, CIGAR stage and z scratch -- the next one shorter (long_to_short), longer (short_to_long)
    or either way (shuffled) in qLen and nCol.  Every job against the oracle."""
    jobs = global_cases.many()[order]
    s = global_cases.SCORINGS[si]
    resident = global_cases.resident_waves(ctx.num_cu(), max(len(j.q) for j in jobs))
    print(f"many/{order} x {s.name}: n = {len(jobs)} jobs, resident waves = {resident}")
    assert len(jobs) >= 20000 and len(jobs) > resident, (len(jobs), resident)     # else the test proves nothing
    ql = np.array([len(j.q) for j in jobs]); nc = np.array([global_cases.n_col(len(j.q), j.w) for j in jobs])
    nxt_q, nxt_c = ql[resident:] - ql[:-resident], nc[resident:] - nc[:-resident]        # a wave's next job against its previous one
    if order == "long_to_short":
        assert (nxt_q <= 0).all() and (nxt_q < 0).sum() > 5000
    elif order == "short_to_long":
        assert (nxt_q >= 0).all() and (nxt_q > 0).sum() > 5000
    else:
        assert min((nxt_q < 0).sum(), (nxt_q > 0).sum(), (nxt_q == 0).sum(), (nxt_c < 0).sum(), (nxt_c > 0).sum()) > 50
    assert _same(_launch(ctx, jobs, s, 128), _oracle(orc, jobs, s), 128, ("many", order)) == len(jobs)


def _job_with_ops(orc, s, base, target):
    """a prefix of `base` whose alignment has exactly `target` operations (by the oracle)"""
    _, cg = orc.sw_global(base.q, base.t, s.mat, s.o_del, s.e_del, s.o_ins, s.e_ins, base.w)
    assert len(cg) > target + 8
    for k in range(target - 8, target + 9):
        qa = sum(int(c >> 4) for c in cg[:k] if (c & 15) in (0, 1)); ta = sum(int(c >> 4) for c in cg[:k] if (c & 15) in (0, 2))
        for more in (0, 1, 2):                                                     # (and a base or two into the next operation)
            if qa + more < 1 or ta + more < 1:
                continue
            j = global_cases.Job(base.q[:qa + more], base.t[:ta + more], abs(ta - qa) + 40)
            if len(orc.sw_global(j.q, j.t, s.mat, s.o_del, s.e_del, s.o_ins, s.e_ins, j.w)[1]) == target:
                return j
    raise AssertionError(f"no prefix with {target} operations")


def test_cigar_capacity_at_the_edges(ctx, orc):
    """max_cigar in {n - 1, n, n + 1} for jobs of known operation count n (3 ... 513, among them n = 511, 512, 513 around the 512 the
    kernel stages, and the long_ops jobs beyond it): the count is always the true one, the words are written exactly when they fit,
    and the row of a job that did not fit stays as the harness zeroed it"""
    s = global_cases.SCORINGS[2]                                                   # gap open 0: the scoring with the most operations
    long_jobs = global_cases.long_ops()
    base = max(long_jobs, key=lambda j: len(orc.sw_global(j.q, j.t, s.mat, s.o_del, s.e_del, s.o_ins, s.e_ins, j.w)[1]))
    jobs = [_job_with_ops(orc, s, base, n) for n in (3, 4, 16, 17, 63, 64, 65, 128, 129, 511, 512, 513)] + long_jobs
    want = _oracle(orc, jobs, s)
    counts = sorted({len(wc) for _, wc in want})
    assert {3, 16, 64, 511, 512, 513} <= set(counts) and counts[-1] > 600, counts
    caps = sorted({m for n in counts for m in (n - 1, n, n + 1) if 1 <= m <= 512} | {512})
    for cap in caps:
        _same(_launch(ctx, jobs, s, cap), want, cap, ("capacity", cap))
    print(f"capacity: {len(jobs)} jobs with {counts} operations, each under max_cigar in {caps}")


def test_vs_ksw_global2_edges_golden(ctx):
    """tests/golden/ksw_global2_edges.npz: the reference's own ksw_global2 on chunk-edge lengths, tie-rich sequences and CIGARs of up
    to 686 operations under five scorings (stored per entry), against the kernel; no oracle in between"""
    z = np.load(os.path.join(G, "ksw_global2_edges.npz"))
    job, gaps, mats = z["job"], z["gaps"], z["mat"]
    seq = lambda pool, off, i: z[pool][z[off][i]:z[off][i + 1]]
    keys = [tuple(gaps[e]) + tuple(mats[e]) for e in range(len(job))]
    done = 0
    for key in sorted(set(keys)):
        es = [e for e in range(len(job)) if keys[e] == key]
        s = global_cases.Scoring("stored", np.array(key[4:], np.int8), *key[:4])
        jobs = [global_cases.Job(seq("q_pool", "q_off", job[e]), seq("t_pool", "t_off", job[e]), int(z["w"][job[e]])) for e in es]
        want = [(int(z["score"][e]), z["cig_pool"][z["cig_off"][e]:z["cig_off"][e + 1]]) for e in es]
        done += _same(_launch(ctx, jobs, s, 512), want, 512, ("edges golden", key[:4]))
    assert done == len(job) >= 1000 and len(set(keys)) == 5


def _raw(ctx, q_len, t_len, w, q_off=0, t_off=0, q_bytes=2048, t_bytes=2048, max_cigar=64):
    return ctx.global_batch(bpsw_hip.default_opt(), [q_len], [t_len], [w], [q_off], [t_off], np.zeros(q_bytes, np.uint8),
                            np.zeros(t_bytes, np.uint8), max_cigar)


def test_refusals(ctx):
    """what bpsw_global_batch refuses: its host loop returns before anything is staged or launched"""
    score, ncig, _ = _raw(ctx, 100, 100, 0)                                                    # (the helper's own job is accepted)
    assert score[0] == 100 and ncig[0] == 1
    for label, kw in (("q_len 0", dict(q_len=0, t_len=10, w=10)), ("q_len 1024", dict(q_len=1024, t_len=1024, w=5)),
                      ("t_len 0", dict(q_len=10, t_len=0, w=10)), ("t_len 65536", dict(q_len=100, t_len=65536, w=70000, t_bytes=65536 + 16)),
                      ("w -1", dict(q_len=10, t_len=10, w=-1)), ("max_cigar 0", dict(q_len=10, t_len=10, w=3, max_cigar=0)),
                      ("max_cigar 513", dict(q_len=10, t_len=10, w=3, max_cigar=513)),
                      ("q_off past its pool", dict(q_len=100, t_len=100, w=3, q_off=2000)),
                      ("t_off past its pool", dict(q_len=100, t_len=100, w=3, t_off=1949)),
                      ("negative offset", dict(q_len=100, t_len=100, w=3, q_off=-1)),
                      ("w < t_len - q_len", dict(q_len=100, t_len=140, w=39)), ("w < q_len - t_len", dict(q_len=140, t_len=100, w=39)),
                      ("w 0, unequal lengths", dict(q_len=100, t_len=101, w=0))):
        with pytest.raises(bpsw_hip.BpswError, match="global: "):      # (the text of the host loop's own checks)
            _raw(ctx, **kw)
    assert _raw(ctx, 100, 140, 40)[1][0] >= 1 and _raw(ctx, 140, 100, 40)[1][0] >= 1          # w = |d| is the edge of the domain
