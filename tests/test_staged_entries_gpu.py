"""The host entries that ship a job table through the context's staging blocks (csrc/bpsw_stage.h: bpsw_ref_fetch, bpsw_global_batch,
bpsw_chain2aln_batch, bpsw_reg2aln_batch, bpsw_seed_batch, bpsw_swalign2_batch) INTERLEAVED on one context: they share h_stage_in,
h_stage_out, d_sw_in and d_sw_out, and the per-entry tests never run one right behind the other at sizes where the part boundaries
move.  A pass at n = 64 leaves every block full of live data; the passes at n = 1, 3, 5 (4 n and 8 n no multiples of 16) then put every
part boundary inside it.  In between, the degenerate parts: a block with an empty pool, null seed arrays, an empty read.  Every result
is the oracle's (the golden's for seeding), exactly."""
import ctypes as C

import numpy as np
import pytest

import bpsw_hip
import fmi_util as fu
import pyoracle as po
from bpsw_hip import fmi, synth
from tail_util import synthetic_group_with_bases
from test_global_gpu import _run as run_global

pytestmark = pytest.mark.gpu
XTRA = po.KSW_XSUBO | po.KSW_XSTART | po.KSW_XBYTE | 19
N_BIG, N_SMALL = 64, (1, 3, 5)
MAT = po.default_mat()


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    for f in a.dtype.names:
        assert np.array_equal(a[f], b[f]), (what, f)


@pytest.fixture(scope="module")
def data(orc):
    """inputs of N_BIG jobs per entry and the oracle's results on them, computed once; a pass at n takes the first n of each"""
    d = {}
    pac, bases, g = synthetic_group_with_bases(orc, 40, 20261301, contigs=(20_000, 9_000, 12_000))
    l_pac = g.l_pac
    d["pac"], d["g"], d["l_pac"] = pac, g, l_pac
    rng = np.random.default_rng(20261302)
    # ref_fetch: windows on both strands, some clipped at the ends, some bridging the strands (empty)
    beg = rng.integers(-50, 2 * l_pac - 200, N_BIG)
    end = beg + rng.integers(1, 400, N_BIG)
    beg[::9] = l_pac - 30
    end[::9] = l_pac + 50
    d["fetch"] = (beg, end, [orc.bns_get_seq(l_pac, pac, int(b), int(e)) for b, e in zip(beg, end)])
    # global alignment
    qs, ts, ws = [], [], []
    for _ in range(N_BIG):
        q = rng.integers(0, 4, int(rng.integers(1, 200))).astype(np.uint8)
        t = np.delete(q, slice(len(q) // 2, len(q) // 2 + int(rng.integers(0, 4)))) if len(q) > 8 else q.copy()
        t[rng.integers(0, len(t), 2)] = rng.integers(0, 4, 2)
        qs.append(q); ts.append(t); ws.append(abs(len(t) - len(q)) + int(rng.integers(0, 30)))
    d["global"] = (qs, ts, ws, [orc.sw_global(q, t, MAT, 6, 1, 6, 1, int(w)) for q, t, w in zip(qs, ts, ws)])
    # chain2aln: per n, the first n reads with their chains
    chains = synth.read_chains(N_BIG, np.asarray(bases[:l_pac], np.uint8), l_pac, read_len=150, sub_rate=0.03, indel_rate=0.005, seed=20261303)
    d["chains"] = {n: (chains.slice(0, n), orc.chain2aln_batch(orc.default_opt(), pac, chains.slice(0, n))[:2]) for n in (N_BIG,) + N_SMALL}
    # reg2aln: one job per (read, region) of the group
    rl, ro = [], []
    for r in range(2 * g.group_size):
        rl += [int(g.read_len[r])] * int(g.reg_cnt[r]); ro += [int(g.read_off[r])] * int(g.reg_cnt[r])
    assert len(rl) >= N_BIG
    rl, ro, regs = np.array(rl[:N_BIG], np.int32), np.array(ro[:N_BIG], np.int64), g.regs[:N_BIG].copy()
    d["r2a"] = {n: (rl[:n], ro[:n], regs[:n], orc.reg2aln_batch(orc.default_opt(), orc.default_tail_opt(), pac, l_pac, g.ann_off, g.ann_len, rl[:n], ro[:n],
                                                             g.read_pool, regs[:n], cigar_cap=48, md_cap=320)) for n in (N_BIG,) + N_SMALL}
    # seeding: genome 1 of the golden; configuration 3 (no exact matches: the overflow pass runs), configuration 1 for the degenerate batch
    gold = np.load(fu.GOLDEN)
    genome = fu.unpack_pac(gold["g1_pac"], int(gold["g1_l_pac"]))
    d["gold"], d["index"] = gold, fu.build_index(genome, 8)[0]
    d["reads"] = fu.split(gold["g1_read_len"], gold["g1_read_pool"])
    assert int(gold["c3_intv_cnt"][:1].max()) > 16 and list(gold["g1_tags"][:4]) == ["exact", "exact256", "short", "len19"]
    # SWAlign2
    d["sw"] = {}
    for n in (N_BIG,) + N_SMALL:
        jobs = synth.sw_jobs(n, read_len=150, seed=20261304 + n)
        d["sw"][n] = (jobs, orc.sw_align2_jobs(orc.default_opt(), XTRA, **jobs)[0])
    return d


def _seed_opt(gold, key):
    v = dict(zip(fu.SEED_OPT_FIELDS, gold[key + "_opt"]))
    return fu.sopt_from({k: (float(x) if k in ("split_factor", "chain_drop_ratio", "mask_level") else int(x)) for k, x in v.items()})


def _one_pass(c, d, n):
    beg, end, want = d["fetch"]
    seqs, lens = c.ref_fetch(beg[:n], end[:n])
    assert np.array_equal(lens, [len(w) for w in want[:n]])
    assert all(np.array_equal(s, w) for s, w in zip(seqs, want[:n])), ("ref_fetch", n)

    qs, ts, ws, want = d["global"]
    score, ncig, cig = run_global(c, qs[:n], ts[:n], ws[:n], max_cigar=64)
    for i in range(n):
        assert score[i] == want[i][0] and ncig[i] == len(want[i][1]) and np.array_equal(cig[i, : ncig[i]], want[i][1]), ("global", n, i)
        assert not cig[i, ncig[i]:].any(), ("global: words behind a job's operations", n, i)

    b, (want_cnt, want_regs) = d["chains"][n]
    got_cnt, got_regs = c.chain2aln_batch(bpsw_hip.default_opt(), b)
    assert np.array_equal(got_cnt, want_cnt)
    _same(got_regs, want_regs, ("chain2aln", n))

    rl, ro, regs, (want, wc, wm) = d["r2a"][n]
    got, gc, gm = c.reg2aln_batch(bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(), rl, ro, d["g"].read_pool, regs, max_cigar=48, max_md=320)
    _same(got, want, ("reg2aln", n))
    for i in range(n):
        nc, nm = min(int(want["n_cigar"][i]), 48), min(int(want["md_len"][i]), 320)
        assert np.array_equal(gc[i][:nc], wc[i][:nc]) and not gc[i][nc:].any(), ("reg2aln cigar", n, i)
        assert np.array_equal(gm[i][:nm], wm[i][:nm]) and not gm[i][nm:].any(), ("reg2aln md", n, i)

    gold = d["gold"]
    icnt, iv, scnt, sv = c.seed_batch(_seed_opt(gold, "c3"), fmi.ReadBatch.from_list(d["reads"][:n]))
    ni, ns = int(gold["c3_intv_cnt"][:n].sum()), int(gold["c3_seed_cnt"][:n].sum())
    assert np.array_equal(icnt, gold["c3_intv_cnt"][:n]) and np.array_equal(scnt, gold["c3_seed_cnt"][:n])
    _same(iv, gold["c3_intv"][:ni], ("intervals", n))
    _same(sv, gold["c3_seeds"][:ns], ("seeds", n))

    jobs, want = d["sw"][n]
    assert np.array_equal(c.swalign2_batch(bpsw_hip.default_opt(), XTRA, **jobs), want), ("swalign2", n)


def _degenerate_parts(c, d, orc):
    l_pac, pac, n = d["l_pac"], d["pac"], 5
    # ref_fetch: beg == end for every window, no output pool at all (out_pool null, out_pool_bytes 0)
    at = np.array([0, 17, l_pac, 2 * l_pac - 1, 2 * l_pac], np.int64)
    off, lens = np.zeros(n, np.int64), np.full(n, -1, np.int64)
    rc = c.lib.bpsw_ref_fetch(c.h, n, at.ctypes.data_as(C.c_void_p), at.ctypes.data_as(C.c_void_p), None, 0, off.ctypes.data_as(C.c_void_p),
                              lens.ctypes.data_as(C.c_void_p))
    assert rc == 0, c.lib.bpsw_last_error()
    assert np.array_equal(lens, [len(orc.bns_get_seq(l_pac, pac, int(p), int(p))) for p in at]) and not lens.any()

    # chain2aln: no read has a chain; the seed arrays are null pointers
    b = d["chains"][n][0]
    none = bpsw_hip.ChainBatchSoA(l_pac=l_pac, read_len=b.read_len, read_off=b.read_off, read_pool=b.read_pool, chain_cnt=np.zeros(n, np.int32),
                                  seed_cnt=np.zeros(0, np.int32), seed_rbeg=np.zeros(0, np.int64), seed_qbeg=np.zeros(0, np.int32),
                                  seed_len=np.zeros(0, np.int32))
    want_cnt, want_regs = orc.chain2aln_batch(orc.default_opt(), pac, none)[:2]
    st = bpsw_hip.Chains()
    st.n_reads, st.read_pool_bytes = n, none.read_pool.size
    st.read_len, st.read_off, st.read_pool, st.chain_cnt = (a.ctypes.data for a in (none.read_len, none.read_off, none.read_pool, none.chain_cnt))
    st.seed_cnt = st.seed_rbeg = st.seed_qbeg = st.seed_len = None
    got_cnt, total, opt = np.full(n, -1, np.int32), C.c_int64(-1), bpsw_hip.default_opt()
    rc = c.lib.bpsw_chain2aln_batch(c.h, C.byref(opt), C.byref(st), po.ZDROP_SCALA, 0, got_cnt.ctypes.data_as(C.c_void_p), None, 0, C.byref(total))
    assert rc == 0, c.lib.bpsw_last_error()
    assert np.array_equal(got_cnt, want_cnt) and total.value == len(want_regs) == 0

    # seeding: an empty read among reads of min_seed_len bases (the golden's len19 read: one interval, its seeds; nothing for the empty one,
    # as for every read shorter than min_seed_len -- the golden's 18-base read)
    gold, r19 = d["gold"], d["reads"][3]
    assert len(r19) == 19 == int(gold["c1_opt"][0]) and gold["c1_intv_cnt"][2] == 0 and gold["c1_seed_cnt"][2] == 0
    i0, s0 = int(gold["c1_intv_cnt"][:3].sum()), int(gold["c1_seed_cnt"][:3].sum())
    wi, ws = gold["c1_intv"][i0: i0 + int(gold["c1_intv_cnt"][3])], gold["c1_seeds"][s0: s0 + int(gold["c1_seed_cnt"][3])]
    icnt, iv, scnt, sv = c.seed_batch(_seed_opt(gold, "c1"), fmi.ReadBatch.from_list([r19, np.zeros(0, np.uint8), r19, r19]))
    assert list(icnt) == [len(wi), 0, len(wi), len(wi)] and list(scnt) == [len(ws), 0, len(ws), len(ws)]
    _same(iv, np.concatenate([wi] * 3), "intervals of the 19-base reads")
    _same(sv, np.concatenate([ws] * 3), "seeds of the 19-base reads")


def test_entries_interleaved_on_one_context(data, orc):
    g = data["g"]
    c = bpsw_hip.Context(0)
    try:
        c.ref_load(data["pac"], data["l_pac"])
        c.bns_load(g.ann_off, g.ann_len, [bytes(g.ann_name_pool[int(g.ann_name_off[i]):int(g.ann_name_off[i + 1])]).decode() for i in range(len(g.ann_len))])
        c.fmi_load(data["index"])
        _one_pass(c, data, N_BIG)
        _degenerate_parts(c, data, orc)
        for n in N_SMALL:
            _one_pass(c, data, n)
    finally:
        c.close()
