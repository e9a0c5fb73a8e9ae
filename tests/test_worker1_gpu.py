"""bpsw_worker1_batch (reads -> regions: seed kernels, host chaining + filter, the round loop of bpsw_chain2aln_batch) against
(a) the reference's chains (tests/golden/seed_chain_small.npz) fed to bpsw_chain2aln_batch on the same context and (b) the
reference's own mem_chain2aln on those chains (ref_chain2aln_batch of the shim, where oracle/_ref is built); and worker1FlatJNI
(with loadPacJNI and loadFmiJNI) through the fake JVM against the C ABI call."""
import os

import numpy as np
import pytest

import bpsw_hip
import fmi_util as fu
import pyoracle
from bpsw_hip import fmi
from conftest import region_fields_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(fu.GOLDEN)


@pytest.fixture(scope="module")
def setup(gold):
    """the larger genome: bases, index (sa_intv 8), reads with at least one base (the round loop takes no empty read)"""
    l_pac = int(gold["g1_l_pac"])
    g = fu.unpack_pac(gold["g1_pac"], l_pac)
    idx, _ = fu.build_index(g, 8)
    return g, idx, fu.split(gold["g1_read_len"], gold["g1_read_pool"])


def _opt(gold, key):
    d = dict(zip(fu.SEED_OPT_FIELDS, gold[key + "_opt"]))
    return fu.sopt_from({k: (float(v) if k in ("split_factor", "chain_drop_ratio", "mask_level") else int(v)) for k, v in d.items()})


def _ref_chain_batch(gold, key, rb, l_pac):
    seeds = gold[key + "_flt_seeds"]
    return bpsw_hip.ChainBatchSoA(l_pac=l_pac, read_len=rb.read_len, read_off=rb.read_off, read_pool=rb.read_pool,
                                  chain_cnt=np.ascontiguousarray(gold[key + "_flt_cnt"]), seed_cnt=np.ascontiguousarray(gold[key + "_flt_seed_cnt"]),
                                  seed_rbeg=np.ascontiguousarray(seeds["rbeg"]), seed_qbeg=np.ascontiguousarray(seeds["qbeg"]),
                                  seed_len=np.ascontiguousarray(seeds["len"]))


@pytest.mark.parametrize("ci,flags", [(1, 0), (1, bpsw_hip.C2A_SORT_DEDUP), (2, 0), (3, bpsw_hip.C2A_SORT_DEDUP | bpsw_hip.C2A_DEDUP_SCALA)])
def test_worker1_equals_reference_chains_through_the_round_loop(ctx, gold, setup, ci, flags):
    g, idx, reads = setup
    ctx.ref_load(gold["g1_pac"], g.size)
    ctx.fmi_load(idx)
    rb = fmi.ReadBatch.from_list(reads)
    opt, key = bpsw_hip.default_opt(), f"c{ci}"
    cnt, regs = ctx.worker1_batch(opt, _opt(gold, key), rb, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=flags)
    wcnt, wregs = ctx.chain2aln_batch(opt, _ref_chain_batch(gold, key, rb, g.size), zdrop_mode=bpsw_hip.ZDROP_BWA, flags=flags)
    assert np.array_equal(cnt, wcnt) and cnt.sum() > len(reads) // 2
    region_fields_equal(regs, wregs)
    assert all(t >= 0 for t in bpsw_hip.last_worker1_times())


@pytest.mark.skipif(not os.path.exists(pyoracle.REF_SO), reason="oracle/_ref/libbwaref.so not built (reference tree absent)")
def test_worker1_equals_the_reference_mem_chain2aln(ctx, gold, setup):
    g, idx, reads = setup
    ctx.ref_load(gold["g1_pac"], g.size)
    ctx.fmi_load(idx)
    rb = fmi.ReadBatch.from_list(reads)
    cnt, regs = ctx.worker1_batch(bpsw_hip.default_opt(), _opt(gold, "c1"), rb, zdrop_mode=bpsw_hip.ZDROP_BWA)
    orc_opt = pyoracle.Oracle().default_opt()
    wcnt, wregs = pyoracle.Ref().chain2aln_batch(orc_opt, gold["g1_pac"], _ref_chain_batch(gold, "c1", rb, g.size))
    assert np.array_equal(cnt, wcnt)
    region_fields_equal(regs, wregs)


def test_worker1_refusals(ctx, gold, setup):
    g, idx, reads = setup
    so, opt = bpsw_hip.default_seed_opt(), bpsw_hip.default_opt()
    ctx.ref_load(gold["g1_pac"], g.size)
    ctx.fmi_unload()
    with pytest.raises(bpsw_hip.BpswError, match=r"\(-1\)"):     # no index
        ctx.worker1_batch(opt, so, fmi.ReadBatch.from_list(reads[:2]))
    l0 = int(gold["g0_l_pac"])
    ctx.fmi_load(fu.build_index(fu.unpack_pac(gold["g0_pac"], l0), 8)[0])
    with pytest.raises(bpsw_hip.BpswError, match=r"\(-1\)"):     # an index of another genome: seq_len != 2 * l_pac
        ctx.worker1_batch(opt, so, fmi.ReadBatch.from_list(reads[:2]))
    ctx.fmi_load(idx)
    with pytest.raises(bpsw_hip.BpswError, match=r"\(-4\)"):     # 257 bases
        ctx.worker1_batch(opt, so, fmi.ReadBatch.from_list([g[:257]]))
    cnt, regs = ctx.worker1_batch(opt, so, fmi.ReadBatch.from_list([g[100:118], g[100:250]]))   # 18 bases: no chains, no error
    assert cnt[0] == 0 and cnt[1] >= 1


@pytest.mark.parametrize("flags", [0, bpsw_hip.C2A_SORT_DEDUP])
def test_worker1_flat_jni_equals_the_c_abi_call(ctx, gold, setup, flags, monkeypatch):
    from bpsw_hip import jnishim
    monkeypatch.setenv("BPSW_ZDROP", "bwa")
    g, idx, reads = setup
    rb = fmi.ReadBatch.from_list(reads)
    opt, so = bpsw_hip.default_opt(), _opt(gold, "c2")
    fake = jnishim.load_fake_worker1()
    ctx.fmi_unload()     # the JNI loaders have to bring both back
    ctx.ref_unload()
    rc, cnt, longs, msg = jnishim.worker1_flat(fake, gold["g1_pac"], g.size, idx, opt, so, flags, rb)
    assert rc == 0, msg
    assert ctx.fmi_length() == 2 * g.size and ctx.ref_length() == g.size
    wcnt, wregs = ctx.worker1_batch(opt, so, rb, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=flags)
    assert np.array_equal(cnt, wcnt) and longs.shape[0] == wregs.shape[0] > 0
    for k, f in enumerate(("rb", "re", "qb", "qe", "score", "truesc", "w", "seedcov")):
        assert np.array_equal(longs[:, k], wregs[f].astype(np.int64)), f
    # a Java exception, not a crash, for what the C ABI refuses: a read of 257 bases
    rc, _, _, msg = jnishim.worker1_flat(fake, None, 0, None, opt, so, flags, fmi.ReadBatch.from_list([g[:257]]))
    assert rc == 1 and "256" in msg, (rc, msg)
