"""bpsw_seed_batch (seed_smem_kernel + seed_sa_kernel, csrc/bpsw_seed.hip) against the reference: the bi-intervals of every
smem_next2 call and the seeds, value AND order, as recorded in tests/golden/seed_chain_small.npz and live where
oracle/_ref/libbwaref.so is built; the index loaded with sa_intv 1, 8 and 32; batch sizes around the wavefront and one that
exceeds the resident lanes; the limits of the entry."""
import os

import numpy as np
import pytest

import bpsw_hip
import fmi_util as fu
import pyoracle
from bpsw_hip import fmi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(fu.GOLDEN)


@pytest.fixture(scope="module")
def genomes(gold):
    """per genome: bases, full suffix array (computed once), reads"""
    out = []
    for gi in (0, 1):
        l_pac = int(gold[f"g{gi}_l_pac"])
        g = fu.unpack_pac(gold[f"g{gi}_pac"], l_pac)
        _, sa = fu.build_index(g, 1)
        out.append((g, sa, fu.split(gold[f"g{gi}_read_len"], gold[f"g{gi}_read_pool"])))
    return out


def _opt(gold, key):
    d = dict(zip(fu.SEED_OPT_FIELDS, gold[key + "_opt"]))
    return fu.sopt_from({k: (float(v) if k in ("split_factor", "chain_drop_ratio", "mask_level") else int(v)) for k, v in d.items()})


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    for f in a.dtype.names:
        assert np.array_equal(a[f], b[f]), (what, f, int((a[f] != b[f]).sum()))


@pytest.mark.parametrize("ci,sa_intv", [(0, 1), (0, 32), (1, 8), (1, 1), (2, 32), (3, 8)])
def test_intervals_and_seeds_against_the_golden(ctx, gold, genomes, ci, sa_intv):
    gi = int(gold["configs"][ci][0])
    g, sa, reads = genomes[gi]
    idx, _ = fu.build_index(g, sa_intv, sa_full=sa)
    ctx.fmi_load(idx)
    assert ctx.fmi_length() == 2 * g.size
    key = f"c{ci}"
    icnt, iv, scnt, sv = ctx.seed_batch(_opt(gold, key), fmi.ReadBatch.from_list(reads))
    assert np.array_equal(icnt, gold[key + "_intv_cnt"])
    _same(iv, gold[key + "_intv"], "intervals")
    assert np.array_equal(scnt, gold[key + "_seed_cnt"])
    _same(sv, gold[key + "_seeds"], "seeds")


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes_around_the_wavefront(ctx, gold, genomes, n):
    g, sa, reads = genomes[1]
    ctx.fmi_load(fu.build_index(g, 8, sa_full=sa)[0])
    icnt, iv, scnt, sv = ctx.seed_batch(_opt(gold, "c1"), fmi.ReadBatch.from_list(reads[:n]))
    ni, ns = int(gold["c1_intv_cnt"][:n].sum()), int(gold["c1_seed_cnt"][:n].sum())
    assert np.array_equal(icnt, gold["c1_intv_cnt"][:n]) and np.array_equal(scnt, gold["c1_seed_cnt"][:n])
    _same(iv, gold["c1_intv"][:ni], "intervals")
    _same(sv, gold["c1_seeds"][:ns], "seeds")


def test_more_reads_than_resident_lanes(ctx, gold, genomes):
    """128 resident lanes, 205 reads: every lane takes a second read (the grid-stride path) and reuses its lists"""
    g, sa, reads = genomes[1]
    ctx.fmi_load(fu.build_index(g, 8, sa_full=sa)[0])
    both = reads + reads[::-1]
    ctx.lib.bpsw_seed_set_resident_lanes(128)
    try:
        icnt, iv, scnt, sv = ctx.seed_batch(_opt(gold, "c1"), fmi.ReadBatch.from_list(both))
    finally:
        ctx.lib.bpsw_seed_set_resident_lanes(0)
    n = len(reads)
    assert np.array_equal(icnt[:n], gold["c1_intv_cnt"]) and np.array_equal(icnt[n:], gold["c1_intv_cnt"][::-1])
    _same(iv[: int(icnt[:n].sum())], gold["c1_intv"], "intervals")
    _same(sv[: int(scnt[:n].sum())], gold["c1_seeds"], "seeds")
    back_i, back_s = fu.split(icnt[n:], iv[int(icnt[:n].sum()):]), fu.split(scnt[n:], sv[int(scnt[:n].sum()):])
    want_i, want_s = fu.split(gold["c1_intv_cnt"], gold["c1_intv"]), fu.split(gold["c1_seed_cnt"], gold["c1_seeds"])
    for k in range(n):
        _same(back_i[k], want_i[n - 1 - k], f"intervals of read {n - 1 - k}")
        _same(back_s[k], want_s[n - 1 - k], f"seeds of read {n - 1 - k}")


@pytest.mark.skipif(not os.path.exists(pyoracle.REF_SO), reason="oracle/_ref/libbwaref.so not built (reference tree absent)")
def test_against_the_live_reference(ctx, gold, genomes):
    """fresh reads and other settings than the fixture's"""
    ref = fu.RefSeeding(pyoracle.REF_SO)
    g, sa, _ = genomes[0]
    idx, _ = fu.build_index(g, 32, sa_full=sa)
    ctx.fmi_load(idx)
    bwt = fu.ref_bwt(idx)
    rng = np.random.default_rng(9)
    reads = []
    for _ in range(70):
        ln = int(rng.integers(19, 257))
        p = int(rng.integers(0, g.size - ln))
        r = g[p: p + ln].copy()
        r[rng.integers(0, ln, 2)] = rng.integers(0, 5, 2)
        reads.append(r if rng.random() < 0.5 else np.where(r[::-1] > 3, 4, 3 - r[::-1]).astype(np.uint8))
    for od in (dict(min_seed_len=12, split_width=3), dict(max_occ=5, split_factor=1.0, no_exact=1)):
        d = dict(ref.default_seed_fields(), **od)
        d.pop("w")
        o = ref.opt(d)
        want_i = [ref.intervals(bwt, o, r) for r in reads]
        want_s = [ref.seeds(bwt, i, g.size) for i in want_i]
        ref.libc.free(o)
        icnt, iv, scnt, sv = ctx.seed_batch(fu.sopt_from(d), fmi.ReadBatch.from_list(reads))
        wc, wi = fu.flat(want_i, fmi.SMEM_DTYPE)
        sc, ws = fu.flat(want_s, fmi.SEED_DTYPE)
        assert np.array_equal(icnt, wc) and np.array_equal(scnt, sc)
        _same(iv, wi, "intervals")
        _same(sv, ws, "seeds")


def test_limits_and_refusals(ctx, gold, genomes):
    g, sa, reads = genomes[0]
    idx, _ = fu.build_index(g, 8, sa_full=sa)
    so = bpsw_hip.default_seed_opt()
    lib, BAD_ARG, LIMIT = ctx.lib, -1, -4

    def load(**kw):
        a = dict(primary=idx.primary, L2=idx.L2, seq_len=idx.seq_len, bwt=idx.bwt, bwt_size=idx.bwt.size, sa_intv=idx.sa_intv, n_sa=idx.sa.size, sa=idx.sa)
        a.update(kw)
        return lib.bpsw_fmi_load(ctx.h, a["primary"], a["L2"].ctypes.data, a["seq_len"], a["bwt"].ctypes.data, a["bwt_size"], a["sa_intv"],
                                 a["n_sa"], a["sa"].ctypes.data)
    ctx.fmi_unload()
    assert ctx.fmi_length() == 0
    with pytest.raises(bpsw_hip.BpswError, match=r"\(-1\)"):     # no index: BPSW_ERR_ARG
        ctx.seed_batch(so, fmi.ReadBatch.from_list(reads[:3]))
    assert load(bwt_size=idx.bwt.size - 1) == BAD_ARG and load(seq_len=idx.seq_len + 16) == BAD_ARG
    assert load(sa_intv=6) == BAD_ARG and load(n_sa=idx.sa.size + 1) == BAD_ARG
    assert ctx.fmi_length() == 0
    assert load() == 0 and ctx.fmi_length() == idx.seq_len
    with pytest.raises(bpsw_hip.BpswError, match=r"\(-4\)"):     # 257 bases: BPSW_ERR_LIMIT
        ctx.seed_batch(so, fmi.ReadBatch.from_list([g[:257]]))
    icnt, iv, scnt, sv = ctx.seed_batch(so, fmi.ReadBatch.from_list([g[:256], g[:18], np.full(40, 4, np.uint8)]))
    assert icnt[0] > 0 and scnt[0] > 0 and icnt[1] == 0 and scnt[1] == 0 and icnt[2] == 0 and scnt[2] == 0
    assert LIMIT == -4
