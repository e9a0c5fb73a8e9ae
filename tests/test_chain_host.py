"""bpsw_chain_seeds (host only: chaining in the B-tree's order, then the chain filter) against the reference's mem_chain /
mem_chain_flt: as recorded in tests/golden/seed_chain_small.npz, and live where oracle/_ref/libbwaref.so is built.  The fixture
holds the cases that show the two klib orders: chains of equal pos (a chimeric read), more than 15 chains (the tree splits), and
chains of equal weight (the introsort's ties).  Also bpsw_seed_opt_default against mem_opt_init."""
import os

import numpy as np
import pytest

import bpsw_hip
import fmi_util as fu
import pyoracle
from bpsw_hip import fmi


@pytest.fixture(scope="module")
def gold():
    return np.load(fu.GOLDEN)


def _configs(gold):
    for ci, (gi, vi) in enumerate(gold["configs"]):
        yield f"c{ci}", int(gi), dict(zip(fu.SEED_OPT_FIELDS, gold[f"c{ci}_opt"]))


def _opt(d):
    return fu.sopt_from({k: (float(v) if k in ("split_factor", "chain_drop_ratio", "mask_level") else int(v)) for k, v in d.items()})


def _same(a, b):
    return a.shape == b.shape and all(np.array_equal(a[f], b[f]) for f in a.dtype.names)


def _weight(chain):
    """mem_chain_weight (native/bwamem.c:244-262) as written: both sums advance `end` by the query coordinates"""
    tot = []
    for key in ("qbeg", "rbeg"):
        w = end = 0
        for s in chain:
            b, e = int(s[key]), int(s[key]) + int(s["len"])
            if b >= end:
                w += int(s["len"])
            elif e > end:
                w += e - end
            end = max(end, int(s["qbeg"]) + int(s["len"]))
        tot.append(w)
    return min(tot)


def test_seed_opt_default_is_mem_opt_init(gold):
    o = bpsw_hip.default_seed_opt()
    want = dict(zip(gold["opt_default_names"].tolist(), gold["opt_default_values"].tolist()))
    for k in fu.SEED_OPT_FIELDS:
        assert float(getattr(o, k)) == want[k], k
    assert bpsw_hip.default_opt().w == want["w"]
    if os.path.exists(pyoracle.REF_SO):
        live = fu.RefSeeding(pyoracle.REF_SO).default_seed_fields()
        assert {k: float(v) for k, v in live.items()} == want


def test_chaining_and_filter_against_the_golden(gold):
    w = bpsw_hip.default_opt().w
    seen = {"equal_pos": 0, "many": 0, "ties": 0, "dropped": 0}
    for key, gi, od in _configs(gold):
        so, l_pac = _opt(od), int(gold[f"g{gi}_l_pac"])
        seeds = fu.split(gold[key + "_seed_cnt"], gold[key + "_seeds"])
        at0 = np.concatenate([[0], np.cumsum(gold[key + "_chain_cnt"])])
        at1 = np.concatenate([[0], np.cumsum(gold[key + "_flt_cnt"])])
        cs0 = fu.split(gold[key + "_chain_seed_cnt"], gold[key + "_chain_seeds"])
        cs1 = fu.split(gold[key + "_flt_seed_cnt"], gold[key + "_flt_seeds"])
        for r, s in enumerate(seeds):
            for filt, at, cs, cnts in ((False, at0, cs0, gold[key + "_chain_seed_cnt"]), (True, at1, cs1, gold[key + "_flt_seed_cnt"])):
                cnt, out = bpsw_hip.chain_seeds(so, w, l_pac, s, filter=filt)
                want_cnt = cnts[at[r]: at[r + 1]]
                want = cs[at[r]: at[r + 1]]
                assert np.array_equal(cnt, want_cnt), (key, r, filt, cnt, want_cnt)
                assert _same(out, np.concatenate(want + [np.zeros(0, fmi.SEED_DTYPE)])), (key, r, filt)
            pos = [int(c["rbeg"][0]) for c in cs0[at0[r]: at0[r + 1]]]
            seen["equal_pos"] += len(pos) != len(set(pos))
            seen["many"] += len(pos) > 15
            seen["dropped"] += at1[r + 1] - at1[r] < len(pos)
            wts = [_weight(c) for c in cs0[at0[r]: at0[r + 1]]]
            seen["ties"] += len(wts) > 2 and len(set(wts)) < len(wts)
    assert seen["equal_pos"] and seen["many"] and seen["dropped"] and seen["ties"], seen


def test_empty_and_refused_inputs():
    so = bpsw_hip.default_seed_opt()
    cnt, out = bpsw_hip.chain_seeds(so, 100, 1000, np.zeros(0, fmi.SEED_DTYPE))
    assert cnt.size == 0 and out.size == 0
    bad = np.array([(5, 0, 0)], fmi.SEED_DTYPE)
    with pytest.raises(bpsw_hip.BpswError):
        bpsw_hip.chain_seeds(so, 100, 1000, bad)


@pytest.mark.skipif(not os.path.exists(pyoracle.REF_SO), reason="oracle/_ref/libbwaref.so not built (reference tree absent)")
def test_chaining_and_filter_against_the_live_reference(gold):
    """fresh reads (not the fixture's) on the fixture's larger genome: seeds by the reference, chains by both"""
    ref = fu.RefSeeding(pyoracle.REF_SO)
    l_pac = int(gold["g1_l_pac"])
    g = fu.unpack_pac(gold["g1_pac"], l_pac)
    idx, _ = fu.build_index(g, 32)
    bwt = fu.ref_bwt(idx)
    rng = np.random.default_rng(77)
    w = bpsw_hip.default_opt().w
    for od in (dict(), dict(max_occ=30, max_chain_gap=40), dict(mask_level=0.2, chain_drop_ratio=0.9)):
        d = dict(ref.default_seed_fields(), **od)
        d.pop("w")
        so, o = fu.sopt_from(d), ref.opt(d)
        for _ in range(40):
            ln = int(rng.integers(30, 257))
            p = int(rng.integers(0, l_pac - ln))
            r = g[p: p + ln].copy()
            r[rng.integers(0, ln, 3)] = rng.integers(0, 4, 3)
            if rng.random() < 0.3:   # a second piece from elsewhere: several chains
                q = int(rng.integers(0, l_pac - 60))
                r[ln // 2: ln // 2 + 50] = g[q: q + 50][: max(0, min(50, ln - ln // 2))]
            s = ref.seeds(bwt, ref.intervals(bwt, o, r), l_pac)
            (bc, bs), (ac, as_) = ref.chains(bwt, o, l_pac, r)
            cnt, out = bpsw_hip.chain_seeds(so, w, l_pac, s, filter=False)
            assert np.array_equal(cnt, bc) and _same(out, bs)
            cnt, out = bpsw_hip.chain_seeds(so, w, l_pac, s, filter=True)
            assert np.array_equal(cnt, ac) and _same(out, as_)
        ref.libc.free(o)
