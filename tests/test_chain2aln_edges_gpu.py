"""chain2aln_kernel (csrc/bpsw_chain2aln.hip) at the limits its code names, against the oracle's sequential walk and against the
reference C's mem_chain2aln (tests/golden/mem_chain2aln_edges.npz).  The batches come from tests/chain_cases.py, one family per
constant or branch: the 64 regions cached in LDS, the lane-strided seed loops and their reductions, the rank's tie-break, the
overlap rule, the second band try, the staged target rows, the cropped windows, and waves that take a second and a third read.
Every family's promise -- that the batch reaches what it was written for -- is asserted on the oracle's output, never the kernel's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bpsw_hip
import chain_cases
import pyoracle as po
from conftest import region_fields_equal

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ARG, CAPACITY, LIMIT = -1, -3, -4
ZMODES = (po.ZDROP_SCALA, po.ZDROP_BWA)
_want = {}      # (family, option, zmode) -> [(cnt, regs) per batch] from the oracle: computed once, never written to


@pytest.fixture(scope="module")
def loaded(ctx):
    pac = chain_cases.reference()[0]
    ctx.ref_load(np.array(pac), chain_cases.L_PAC)
    return ctx


def _family(ctx, name):
    if name == "requeue":   # 3 * resident waves + 5 reads: 24 581 on 256 CUs (chain2aln_resident_waves: 8 blocks of 4 waves a CU)
        return chain_cases.requeue(ctx.num_cu() * 8 * 4)
    return chain_cases.GROUPS[name]()


def _oracle(orc, ctx, name, oi, zmode):
    key = (name, oi, zmode)
    if key not in _want:
        o, pac = chain_cases.OPTIONS[oi], chain_cases.reference()[0]
        res = [orc.chain2aln_batch(chain_cases.apply(orc.default_opt(), o, w), pac, b, zmode)[:2] for w, b in _family(ctx, name).batches]
        for cnt, regs in res:
            cnt.setflags(write=False); regs.setflags(write=False)
        _want[key] = res
    return _want[key]


def _kernel_matches(ctx, fam, oi, zmode, want, flags=0):
    for (w, b), (wcnt, wregs) in zip(fam.batches, want):
        cnt, regs = ctx.chain2aln_batch(chain_cases.apply(bpsw_hip.default_opt(), chain_cases.OPTIONS[oi], w), b, zmode, flags)
        assert np.array_equal(cnt, wcnt), (w, int((cnt != wcnt).sum()), np.flatnonzero(cnt != wcnt)[:8])
        region_fields_equal(regs, wregs)


@pytest.mark.parametrize("zmode", ZMODES)
@pytest.mark.parametrize("oi", range(len(chain_cases.OPTIONS)), ids=[o.name for o in chain_cases.OPTIONS])
@pytest.mark.parametrize("name", list(chain_cases.GROUPS))
def test_family_matches_oracle(loaded, orc, name, oi, zmode):
    fam = _family(loaded, name)
    want = _oracle(orc, loaded, name, oi, zmode)
    print(name, chain_cases.OPTIONS[oi].name, zmode, fam.promise(oi, want, zmode == po.ZDROP_BWA))
    if name == "requeue":
        n = len(want[0][0])
        assert n == 3 * loaded.num_cu() * 32 + 5 and n > 2 * loaded.num_cu() * 32     # more reads than the launch has waves, twice over
    _kernel_matches(loaded, fam, oi, zmode, want)


@pytest.mark.parametrize("mask", [0, 1, 63])
@pytest.mark.parametrize("name", ["band", "seed_lanes"])
def test_shortcut_masks_change_nothing(loaded, orc, name, mask):
    """bpsw_set_ext_shortcuts: the closed forms that stand in for the DP inside this kernel, all off / the first alone / all on"""
    fam = _family(loaded, name)
    try:
        loaded.set_ext_shortcuts(mask)
        for oi in range(len(chain_cases.OPTIONS)):
            for zmode in ZMODES:
                _kernel_matches(loaded, fam, oi, zmode, _oracle(orc, loaded, name, oi, zmode))
    finally:
        loaded.set_ext_shortcuts(63)


def test_reference_fixture(loaded):
    """the kernel in the BWA z-drop parse against mem_chain2aln's own regions"""
    z = np.load(os.path.join(G, "mem_chain2aln_edges.npz"))
    assert np.array_equal(z["pac"], chain_cases.reference()[0]) and int(z["l_pac"]) == chain_cases.L_PAC
    regions = 0
    for i in range(int(z["n_batches"])):
        fam, w, b = chain_cases.fixture_batch(z, i)
        for k in range(int(z["n_options"])):
            opt = chain_cases.apply(bpsw_hip.default_opt(), chain_cases.fixture_options(z, k), w)
            cnt, regs = loaded.chain2aln_batch(opt, b, po.ZDROP_BWA)
            assert np.array_equal(cnt, z[f"b{i}_o{k}_cnt"]), (fam, w, k)
            region_fields_equal(regs, z[f"b{i}_o{k}_regs"])
            regions += len(regs)
    assert regions > 4000


@pytest.mark.parametrize("flags,mode", [(bpsw_hip.C2A_SORT_DEDUP, po.RESCUE_C), (bpsw_hip.C2A_SORT_DEDUP | bpsw_hip.C2A_DEDUP_SCALA, po.RESCUE_SCALA)])
@pytest.mark.parametrize("name", ["region_cache", "seed_lanes"])
def test_sort_dedup_of_long_lists(loaded, orc, name, flags, mode):
    """memSortAndDedup on lists of up to 202 regions, many of them equal"""
    fam = _family(loaded, name)
    (cnt, regs), = _oracle(orc, loaded, name, 0, po.ZDROP_SCALA)
    kept = [orc.sort_dedup(g.copy(), 0.95, mode) for g in chain_cases.per_read(cnt, regs)]
    assert max(len(g) for g in chain_cases.per_read(cnt, regs)) > 64 and sum(len(k) for k in kept) < len(regs)
    _kernel_matches(loaded, fam, 0, po.ZDROP_SCALA, [(np.array([len(k) for k in kept], np.int32), np.concatenate(kept))], flags)


# ------------------------------------------------------------------------------------------------------------- refusals
def _raw(ctx, opt, b, cap, zmode=po.ZDROP_SCALA):
    """bpsw_chain2aln_batch with an output capacity of the caller's choosing -> (rc, total)"""
    st = bpsw_hip.Chains()
    st.n_reads = b.n_reads
    for f in ("read_len", "read_off", "read_pool", "chain_cnt", "seed_cnt", "seed_rbeg", "seed_qbeg", "seed_len"):
        setattr(st, f, getattr(b, f).ctypes.data)
    st.read_pool_bytes = b.read_pool.size
    out_cnt, out, total = np.zeros(max(b.n_reads, 1), np.int32), np.empty(max(cap, 1), bpsw_hip.ALNREG_DTYPE), C.c_int64(-7)
    rc = ctx.lib.bpsw_chain2aln_batch(ctx.h, C.byref(opt), C.byref(st), zmode, 0, out_cnt.ctypes.data_as(C.c_void_p),
                                      out.ctypes.data_as(C.c_void_p), C.c_int64(cap), C.byref(total))
    return rc, total.value, out_cnt, out


def _one(read_len=100, seeds=((5000, 0, 50),), pool=320):
    i32, i64 = (lambda v: np.array(v, np.int32)), (lambda v: np.array(v, np.int64))
    return bpsw_hip.ChainBatchSoA(l_pac=chain_cases.L_PAC, read_len=i32([read_len]), read_off=i64([0]), read_pool=np.zeros(pool, np.uint8),
                                  chain_cnt=i32([1]), seed_cnt=i32([len(seeds)]), seed_rbeg=i64([s[0] for s in seeds]),
                                  seed_qbeg=i32([s[1] for s in seeds]), seed_len=i32([s[2] for s in seeds]))


def test_refusals_name_their_reason(loaded, orc):
    L = chain_cases.L_PAC
    opt = bpsw_hip.default_opt

    def with_(**kw):
        o = opt()
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    cases = [
        ("w = 0", with_(w=0), _one(), po.ZDROP_SCALA, LIMIT),
        ("w = 255", with_(w=255), _one(), po.ZDROP_SCALA, LIMIT),
        ("a 257-base read", opt(), _one(read_len=257), po.ZDROP_SCALA, LIMIT),
        ("e_del = 0", with_(e_del=0), _one(), po.ZDROP_SCALA, ARG),
        ("one seed on each strand", opt(), _one(seeds=((5000, 0, 30), (L + 5000, 40, 30))), po.ZDROP_SCALA, ARG),
        ("a forward seed ending past l_pac", opt(), _one(seeds=((L - 20, 0, 30),)), po.ZDROP_SCALA, ARG),
        ("zdrop_mode = 2", opt(), _one(), 2, ARG),
    ]
    for what, o, b, zmode, code in cases:
        rc, _, _, _ = _raw(loaded, o, b, 64, zmode)
        assert rc == code, (what, rc, loaded.lib.bpsw_last_error().decode())
    assert _raw(loaded, with_(w=254), _one(read_len=256), 64)[0] == bpsw_hip.BPSW_OK       # the limits themselves pass
    assert _raw(loaded, opt(), _one(seeds=((L - 30, 0, 30),)), 64)[0] == bpsw_hip.BPSW_OK
    # out_cap one short of the seed count: CAPACITY, *out_total = the seed count; at that capacity the batch succeeds
    (w, b), = chain_cases.overlap().batches
    n_seeds = int(b.seed_len.shape[0])
    rc, total, _, _ = _raw(loaded, opt(), b, n_seeds - 1)
    assert (rc, total) == (CAPACITY, n_seeds)
    rc, total, cnt, regs = _raw(loaded, opt(), b, n_seeds)
    (wcnt, wregs), = _oracle(orc, loaded, "overlap", 0, po.ZDROP_SCALA)
    assert rc == bpsw_hip.BPSW_OK and total == len(wregs) and np.array_equal(cnt, wcnt)
    region_fields_equal(regs[:total], wregs)
    with pytest.raises(bpsw_hip.BpswError, match=re.escape("(-4)")):
        loaded.chain2aln_batch(with_(w=255), _one())
