"""bpsw_fmi_build (csrc/bpsw_index.hip): the FM-index built on the device from the 2-bit reference.

The result is unique -- every suffix of text + sentinel is distinct -- so the yardstick is equality, whatever sort is used: primary, L2,
the interleaved BWT words and the sampled suffix array against fmi_util.build_index (which tests/test_fmi_builder.py pins on the
reference) on every genome of tests/fmi_build_cases.py, and against the reference itself: bwt_cal_sa of oracle/_ref/libbwaref.so over
the device-built BWT must return the device-built samples.  The stats of bpsw_last_fmi_build_stats prove that a case went where it was
meant to go: the rounds a one-base first key needs, a non-empty list after the first sort, the tiles the sort spans."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bpsw_hip
import fmi_build_cases as bc
import fmi_util as fu
import index_cases as ic
from bpsw_hip import fmi
from conftest import region_fields_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _defaults():
    yield
    bpsw_hip.fmi_build_set_first_key(0)
    bpsw_hip.fmi_build_set_budget(0)
    bpsw_hip.load_library().bpsw_scan_set_tile(0)


def _build(ctx, name, sa_intv, flags=0, fetch=True):
    g, pac, _ = bc.genome(name)
    return ctx.fmi_build(pac, g.size, sa_intv, flags, fetch)


@pytest.mark.parametrize("name", bc.NAMES)
def test_byte_equality_at_every_interval_and_both_first_keys(ctx, name):
    """sa_intv 1 (the whole suffix array), 8, 32 and one above seq_len (a single sample); the first key at its default and at one base"""
    for k0 in (0, 1):
        bpsw_hip.fmi_build_set_first_key(k0)
        for sa_intv in bc.SA_INTVS + (bc.one_sample_intv(name),):
            got = _build(ctx, name, sa_intv)
            want = bc.expected(name, sa_intv)
            assert not bc.differences(got, want), (name, k0, sa_intv, bc.differences(got, want))
            assert got.L2[0] == 0 and got.L2[4] == got.seq_len and got.sa[0] == -1
            st = bpsw_hip.last_fmi_build_stats()
            assert st["sort_tile"] == bc.TILE and st["first_key"] == (k0 or 29) and st["peak_bytes"] > 100 * got.seq_len
            assert st["unresolved_max"] >= st["unresolved_first"] and st["radix_passes"] >= (8 if k0 == 0 else 1)
            assert (st["rounds"] == 0) == (st["unresolved_first"] == 0)
            assert all(t >= 0 for t in bpsw_hip.last_fmi_build_times())
        assert got.n_sa == 1


@pytest.mark.parametrize("name", bc.LONG_ROUNDS + ("random150k",))
def test_one_base_first_key_runs_the_rounds(ctx, name):
    bpsw_hip.fmi_build_set_first_key(1)
    got = _build(ctx, name, 8)
    st = bpsw_hip.last_fmi_build_stats()
    assert st["first_key"] == 1 and st["unresolved_first"] > 0 and st["unresolved_max"] >= st["unresolved_first"], st
    assert st["rounds"] >= (4 if name == "random150k" else 12), st
    if name == "random150k":
        assert got.seq_len + 1 >= 3 * st["sort_tile"]
    assert not bc.differences(got, bc.expected(name, 8))
    bpsw_hip.fmi_build_set_first_key(0)
    _build(ctx, name, 8)
    assert bpsw_hip.last_fmi_build_stats()["rounds"] < st["rounds"]


@pytest.mark.parametrize("name,k0", [("three_tiles_plus_1", 1), ("random150k", 0), ("runs", 1)])
def test_scans_over_several_tiles(ctx, name, k0):
    """the scans of the digit tables, of the three list columns and of the block counts with 64 items a workgroup"""
    bpsw_hip.load_library().bpsw_scan_set_tile(64)
    bpsw_hip.fmi_build_set_first_key(k0)
    got = _build(ctx, name, 32)
    assert not bc.differences(got, bc.expected(name, 32))


@pytest.mark.skipif(not os.path.exists(bc.REF_SO), reason="oracle/_ref/libbwaref.so is not built")
@pytest.mark.parametrize("name,sa_intv", [("random150k", 32), ("palindrome", 8), ("p_last", 1), ("len3", 2), ("acg5000", 4)])
def test_reference_bwt_cal_sa_over_the_device_built_bwt(ctx, name, sa_intv):
    got = _build(ctx, name, sa_intv)
    lib, libc = C.CDLL(bc.REF_SO), C.CDLL(None)
    lib.bwt_cal_sa.argtypes = [C.c_void_p, C.c_int]
    libc.free.argtypes = [C.c_void_p]
    b = fu.ref_bwt(got)
    b.sa, b.n_sa, b.sa_intv = None, 0, 0
    lib.bwt_cal_sa(C.addressof(b), sa_intv)
    assert b.n_sa == got.n_sa and b.sa_intv == sa_intv
    ref_sa = np.ctypeslib.as_array(C.cast(b.sa, C.POINTER(C.c_int64)), shape=(got.n_sa,)).copy()
    libc.free(b.sa)
    assert np.array_equal(ref_sa, got.sa)


@pytest.fixture(scope="module")
def gold():
    return np.load(fu.GOLDEN)


def _opt(gold, key):
    d = dict(zip(fu.SEED_OPT_FIELDS, gold[key + "_opt"]))
    return fu.sopt_from({k: (float(v) if k in ("split_factor", "chain_drop_ratio", "mask_level") else int(v)) for k, v in d.items()})


def _same(a, b):
    assert a.shape == b.shape
    for f in a.dtype.names:
        assert np.array_equal(a[f], b[f]), f


def test_load_and_ref_flags_feed_the_align_entries(ctx, gold):
    """LOAD | REF with no host arrays: the index and the reference exist on the device only, and seeding and worker1 give exactly what
    they give after bpsw_ref_load and bpsw_fmi_load of build_index's arrays"""
    l_pac, pac = int(gold["g1_l_pac"]), np.ascontiguousarray(gold["g1_pac"])
    g = fu.unpack_pac(pac, l_pac)
    reads = [r for r in fu.split(gold["g1_read_len"], gold["g1_read_pool"]) if r.size]
    rb, so, opt = fmi.ReadBatch.from_list(reads), _opt(gold, "c1"), bpsw_hip.default_opt()
    ctx.ref_load(pac, l_pac)
    ctx.fmi_load(fu.build_index(g, 8)[0])
    want_seed = ctx.seed_batch(so, rb)
    want_cnt, want_regs = ctx.worker1_batch(opt, so, rb, zdrop_mode=bpsw_hip.ZDROP_BWA)
    assert want_seed[2].sum() > 0 and want_cnt.sum() > len(reads) // 2
    ctx.fmi_unload()
    ctx.ref_unload()
    assert ctx.fmi_length() == 0 and ctx.ref_length() == 0
    idx = ctx.fmi_build(pac, l_pac, 8, bpsw_hip.FMI_BUILD_LOAD | bpsw_hip.FMI_BUILD_REF, fetch=False)
    assert idx.bwt.size == 0 and idx.sa.size == 0 and idx.seq_len == 2 * l_pac
    assert ctx.fmi_length() == 2 * l_pac and ctx.ref_length() == l_pac
    got_seed = ctx.seed_batch(so, rb)
    assert np.array_equal(got_seed[0], want_seed[0]) and np.array_equal(got_seed[2], want_seed[2])
    _same(got_seed[1], want_seed[1])
    _same(got_seed[3], want_seed[3])
    cnt, regs = ctx.worker1_batch(opt, so, rb, zdrop_mode=bpsw_hip.ZDROP_BWA)
    assert np.array_equal(cnt, want_cnt)
    region_fields_equal(regs, want_regs)
    # LOAD with host arrays, over an index that is loaded: the arrays come back as well, and a second context of the device sees the index
    idx = ctx.fmi_build(pac, l_pac, 8, bpsw_hip.FMI_BUILD_LOAD)
    assert not bc.differences(idx, fu.build_index(g, 8)[0])
    other = bpsw_hip.Context(0)
    try:
        assert other.fmi_length() == 2 * l_pac
        _same(other.seed_batch(so, rb)[3], want_seed[3])
    finally:
        other.close()


def _raw(ctx, pac, l_pac, sa_intv, flags, bwt, bwt_cap, sa, sa_cap, out):
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return ctx.lib.bpsw_fmi_build(ctx.h, P(pac), l_pac, sa_intv, flags, P(bwt), bwt_cap, P(sa), sa_cap, None if out is None else C.byref(out))


def test_refusals(ctx):
    g, pac, _ = bc.genome("runs")
    pac = np.array(pac)
    sh = bpsw_hip.fmi_build_shape(g.size, 8)
    assert (sh.seq_len, sh.bwt_size, sh.n_sa, sh.sa_intv) == (2000, 125 + 17 * 8, 251, 8)
    bwt, sa, out = np.zeros(sh.bwt_size, np.uint32), np.zeros(sh.n_sa, np.int64), fmi.BuildShape()
    ARG, CAP, LIMIT = -1, -3, -4
    assert _raw(ctx, None, g.size, 8, 0, bwt, bwt.size, sa, sa.size, out) == ARG
    assert _raw(ctx, pac, g.size, 8, 0, bwt, bwt.size, sa, sa.size, None) == ARG
    assert _raw(ctx, pac, 0, 8, 0, bwt, bwt.size, sa, sa.size, out) == ARG
    assert _raw(ctx, pac, g.size, 0, 0, bwt, bwt.size, sa, sa.size, out) == ARG
    assert _raw(ctx, pac, g.size, 12, 0, bwt, bwt.size, sa, sa.size, out) == ARG
    assert _raw(ctx, pac, g.size, 8, 4, bwt, bwt.size, sa, sa.size, out) == ARG
    assert _raw(ctx, pac, g.size, 8, 0, None, 0, None, 0, out) == ARG
    assert _raw(ctx, pac, g.size, 8, bpsw_hip.FMI_BUILD_REF, None, 0, None, 0, out) == ARG
    lib = ctx.lib
    assert lib.bpsw_fmi_build_shape(0, 8, C.byref(out)) == ARG and lib.bpsw_fmi_build_shape(10, 3, C.byref(out)) == ARG
    assert lib.bpsw_fmi_build_shape(10, 8, None) == ARG
    # a short array: nothing is built, the sizes are reported
    for bc_, sc_ in ((bwt.size - 1, sa.size), (bwt.size, sa.size - 1)):
        out = fmi.BuildShape()
        bwt[:] = 0xdeadbeef; sa[:] = -7
        assert _raw(ctx, pac, g.size, 8, 0, bwt, bc_, sa, sc_, out) == CAP
        assert (out.seq_len, out.bwt_size, out.n_sa, out.sa_intv) == (2000, sh.bwt_size, sh.n_sa, 8)
        assert np.all(bwt == 0xdeadbeef) and np.all(sa == -7)
    # a budget the working set does not fit: refused before anything is allocated, and the index loaded before still seeds
    idx = bc.expected("runs", 8)
    ctx.fmi_load(idx)
    so = fu.sopt_from(ic.OPTION_SETS["every_row"])
    rb = fmi.ReadBatch.from_list([np.array([c], np.uint8) for c in range(4)])
    before = ctx.seed_batch(so, rb)
    bpsw_hip.fmi_build_set_budget(100_000)
    for flags in (0, bpsw_hip.FMI_BUILD_LOAD | bpsw_hip.FMI_BUILD_REF):
        assert _raw(ctx, pac, g.size, 8, flags, bwt, bwt.size, sa, sa.size, out) == LIMIT
        msg = lib.bpsw_last_error().decode()
        need, avail = [int(v) for v in re.findall(r"(\d+) bytes", msg)][:2]
        assert avail == 100_000 and need == bpsw_hip.last_fmi_build_stats()["peak_bytes"] and need > 100 * 2001, msg
    assert ctx.fmi_length() == 2000
    after = ctx.seed_batch(so, rb)
    assert int(after[2].sum()) == 2000 and np.array_equal(after[3]["rbeg"], before[3]["rbeg"])
    bpsw_hip.fmi_build_set_budget(0)
    assert _raw(ctx, pac, g.size, 8, 0, bwt, bwt.size, sa, sa.size, out) == 0
    assert out.primary == idx.primary and np.array_equal(bwt, idx.bwt) and np.array_equal(sa, idx.sa)


@pytest.mark.parametrize("name,sa_intv", [("runs", 8), ("len3", 1)])
def test_index_files_of_a_built_index(ctx, tmp_path, name, sa_intv):
    got = _build(ctx, name, sa_intv)
    bc.files_round_trip(got, tmp_path, bc.genome(name)[2])
