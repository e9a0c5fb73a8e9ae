"""The chains resident on the device (BPSW_W1_CHAINS_RESIDENT / BPSW_CHAIN_TABLES_DEVICE: chain_emit_resident_kernel, the scans of
csrc/bpsw_scan.hip, chain_host_merge_kernel, chain_tables_kernel in csrc/bpsw_chain_dev.hip, and the round loop's back half on the
tables they leave).

1. The tables, fetched by bpsw_chain_batch_ex, against bpsw_chain_batch on the same lists (counts, seed counts, seeds field by field,
   filter off and on) and against the fixture's recorded chains; in this process at the default BPSW_CHAIN_DEV_MAX_SEEDS and in
   child processes at 0 (every read on the device; the set in three parts) and 1 (every read of two or more seeds through the
   calling thread and the pool upload).  (Run as `python tests/test_chains_resident_gpu.py parity PART` this file is that child.)
2. Capacity and refusals of bpsw_chain_batch_ex.
3. bpsw_worker1_batch with the flag against the call without any W1 flag: out_cnt, the regions, the capacity contract.
4. The bus bytes of the chain stage: with the flag a constant, 32 bytes a slice and 32 of totals (include/bpsw.h).
5. Reads to SAM, and worker1FlatJNI through the fake JVM."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":      # the child process: what conftest.py does for the suite
    HERE = os.path.dirname(os.path.abspath(__file__))
    ROOT = os.path.dirname(HERE)
    for p in (os.path.join(ROOT, "cloud-scale-bwamem_amd"), os.path.join(ROOT, "oracle"), HERE):
        sys.path.insert(0, p)

import bpsw_hip
import chain_lists as cl
import fmi_util as fu
from bpsw_hip import fmi

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_CAPACITY = -1, -3
TABLES = getattr(bpsw_hip, "CHAIN_TABLES_DEVICE", None)
RESIDENT = getattr(bpsw_hip, "W1_CHAINS_RESIDENT", None)
W1_PLAN = bpsw_hip.W1_SEED_PLAN_DEVICE
FETCHED_PER_SLICE, FETCHED_ONCE = 32, 32      # include/bpsw.h, bpsw_last_chain_bytes


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    for f in a.dtype.names:
        assert np.array_equal(a[f], b[f]), (what, f, int((a[f] != b[f]).sum()))


def _opt(gold, key):
    d = dict(zip(fu.SEED_OPT_FIELDS, gold[key + "_opt"]))
    return fu.sopt_from({k: (float(v) if k in ("split_factor", "chain_drop_ratio", "mask_level") else int(v)) for k, v in d.items()})


# ---- 1. the parity set, shared by the suite's process and the children -----------------------------------------------------------------
def check_batch(ctx, per_read, what, od=None, w=100, l_pac=cl.L_PAC, filters=(False, True)):
    """bpsw_chain_batch_ex with the tables against bpsw_chain_batch; -> the split of the call with the tables"""
    so = cl.sopt(od or {})
    cnt, flat = fu.flat(per_read, fmi.SEED_DTYPE)
    for filt in filters:
        want = ctx.chain_batch(so, w, l_pac, cnt, flat, filter=filt)
        got = ctx.chain_batch(so, w, l_pac, cnt, flat, filter=filt, flags=TABLES)
        assert np.array_equal(got[0], want[0]), (what, filt)
        assert np.array_equal(got[1], want[1]), (what, filt)
        _same(got[2], want[2], (what, filt))
    return bpsw_hip.chain_last_split()


def check_golden(ctx, gold):
    w = bpsw_hip.default_opt().w
    for ci, (gi, _) in enumerate(gold["configs"]):
        key = f"c{ci}"
        so, l_pac = _opt(gold, key), int(gold[f"g{int(gi)}_l_pac"])
        for filt, a, b, c in ((False, "_chain_cnt", "_chain_seed_cnt", "_chain_seeds"), (True, "_flt_cnt", "_flt_seed_cnt", "_flt_seeds")):
            cc, sc, out = ctx.chain_batch(so, w, l_pac, gold[key + "_seed_cnt"], gold[key + "_seeds"], filter=filt, flags=TABLES)
            assert np.array_equal(cc, gold[key + a]), (key, filt)
            assert np.array_equal(sc, gold[key + b]), (key, filt)
            _same(out, gold[key + c], (key, filt))


def _default_lists(lists):
    return [c[4] for c in lists if not c[1] and c[2] == 100 and c[3] == cl.L_PAC]


def _short_lists(lists, rng, n):
    pool = [s for s in _default_lists(lists) if s.size <= 40]
    return [pool[i] for i in rng.integers(0, len(pool), n)]


def check_lists(ctx, lists, half=None):
    """every generated list as a batch of its own (its options); half 0 / 1: every second one"""
    for k, (name, od, w, l_pac, seeds) in enumerate(lists):
        if half is None or k % 2 == half:
            check_batch(ctx, [seeds], name, od, w, l_pac)


def check_shapes(ctx, lists):
    """the shapes of the batch; -> the split of the batch with the read of 3 000 seeds"""
    rng = np.random.default_rng(31)
    mixed = _default_lists(lists)
    for n in (1, 63, 64, 65):
        check_batch(ctx, [mixed[i] for i in rng.integers(0, len(mixed), n)], f"{n} reads", filters=(True,))
    empty = np.zeros(0, fmi.SEED_DTYPE)
    check_batch(ctx, [empty] + _short_lists(lists, rng, 20) + [empty, empty], "first and last reads without seeds", filters=(True,))
    check_batch(ctx, [empty, empty, empty], "no seeds at all", filters=(True,))
    few = [cl.clustered(int(k), rng, spots=2) for k in rng.integers(0, 6, 40)]
    long_one = next(c[4] for c in lists if c[0] == "long_3000")
    return check_batch(ctx, few[:25] + [long_one] + few[25:], "one long read between short ones")


def check_arena_budget(ctx):
    """three slices, and a read beyond the budget; -> the two splits"""
    rng = np.random.default_rng(32)
    reads = [cl.clustered(60, rng, spots=5) for _ in range(90)]
    per_read = 16 + 52 * 60 + 256 * (60 // 7 + 2) + 896      # the slice of a read of 60 seeds (csrc/bpsw_chain_core.h)
    lib = bpsw_hip.load_library()
    try:
        lib.bpsw_chain_set_arena_budget(30 * per_read + 8)
        st3 = check_batch(ctx, reads, "three slices", filters=(True,))
        big = cl.clustered(120, rng, spots=10)
        lib.bpsw_chain_set_arena_budget(7000)
        st1 = check_batch(ctx, [reads[0], big, reads[1]], "a read larger than the budget", filters=(True,))
    finally:
        lib.bpsw_chain_set_arena_budget(0)
    return st3, st1


def check_scan_levels(ctx):
    """4 097 short reads at 64 items a tile: 65 tiles, the second level of the scan loops"""
    rng = np.random.default_rng(33)
    reads = [cl.clustered(int(k), rng, spots=2) for k in rng.integers(0, 5, 4097)]
    lib = bpsw_hip.load_library()
    try:
        lib.bpsw_scan_set_tile(64)
        return check_batch(ctx, reads, "4 097 reads, 65 tiles", filters=(True,))
    finally:
        lib.bpsw_scan_set_tile(0)


@pytest.fixture(scope="module")
def gold():
    return np.load(fu.GOLDEN)


@pytest.fixture(scope="module")
def lists():
    return cl.cases()


def test_tables_equal_the_recorded_chains(ctx, gold):
    check_golden(ctx, gold)


def test_tables_equal_chain_batch_on_generated_lists_and_batch_shapes(ctx, lists):
    check_lists(ctx, lists)
    st = check_shapes(ctx, lists)
    assert st[1] == 1, st       # the read of 3 000 seeds was chained on the calling thread and copied into the pools


def test_tables_over_three_slices_and_a_read_beyond_the_budget(ctx):
    st3, st1 = check_arena_budget(ctx)
    assert st3[0] == 90 and st3[2] == 3, st3
    assert st1[0] == 3 and st1[2] == 3 and st1[3] == 12016, st1


def test_tables_when_the_scan_takes_its_second_level(ctx):
    st = check_scan_levels(ctx)
    assert st[0] > 3000 and st[2] == 1, st


@pytest.mark.parametrize("limit,part", [("0", "lists0"), ("0", "lists1"), ("0", "shapes"), ("1", "all")])
def test_parity_in_a_child_process(limit, part):
    """BPSW_CHAIN_DEV_MAX_SEEDS is read once per process.  0: the kernel chains every read (a lane takes tens of microseconds a
    seed, so the set is run in three parts); 1: every read of two or more seeds is chained on the calling thread and reaches the
    pools through the upload"""
    env = dict(os.environ, BPSW_CHAIN_DEV_MAX_SEEDS=limit)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "parity", part], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "parity OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


# ---- 2. capacity and refusals --------------------------------------------------------------------------------------------------------------
def test_capacity_and_refusals(ctx, lists):
    so, lib = bpsw_hip.default_seed_opt(), bpsw_hip.load_library()
    reads = _short_lists(lists, np.random.default_rng(3), 30)
    cnt, flat = fu.flat(reads, fmi.SEED_DTYPE)
    want = ctx.chain_batch(so, 100, cl.L_PAC, cnt, flat, filter=True)
    chain_cnt = np.zeros(cnt.size, np.int32)
    ct, st = C.c_int64(0), C.c_int64(0)

    def call(n, scnt, seeds, ccap, scap, flags=TABLES):
        sc, out = np.zeros(max(ccap, 1), np.int32), np.zeros(max(scap, 1), fmi.SEED_DTYPE)
        rc = lib.bpsw_chain_batch_ex(ctx.h, C.byref(so), 100, cl.L_PAC, n, scnt.ctypes.data, seeds.ctypes.data, 1, chain_cnt.ctypes.data,
                                     sc.ctypes.data, ccap, out.ctypes.data, scap, C.byref(ct), C.byref(st), flags)
        return rc, sc, out
    assert want[1].size > 2 and want[2].shape[0] > 2
    for ccap, scap in ((want[1].size - 1, want[2].shape[0]), (want[1].size, want[2].shape[0] - 1), (0, 0)):
        rc, _, _ = call(cnt.size, cnt, flat, ccap, scap)
        assert rc == ERR_CAPACITY and (ct.value, st.value) == (want[1].size, want[2].shape[0])
    rc, sc, out = call(cnt.size, cnt, flat, ct.value, st.value)     # a second call with the totals succeeds
    assert rc == 0 and np.array_equal(chain_cnt, want[0]) and np.array_equal(sc, want[1])
    _same(out, want[2], "after the capacity error")
    rc, sc, out = call(cnt.size, cnt, flat, ct.value, st.value, flags=0)     # flags 0 is bpsw_chain_batch itself
    assert rc == 0 and np.array_equal(sc, want[1])
    for flags in (2, TABLES | 2, -2):
        assert call(cnt.size, cnt, flat, flat.shape[0], flat.shape[0], flags=flags)[0] == ERR_ARG
    for field, v in (("len", 0), ("qbeg", -1)):
        bad = flat.copy()
        bad[field][bad.shape[0] // 2] = v
        assert call(cnt.size, cnt, bad, flat.shape[0], flat.shape[0])[0] == ERR_ARG
    ct.value = st.value = 7
    assert call(0, cnt, flat, 0, 0)[0] == 0 and (ct.value, st.value) == (0, 0)     # n_reads == 0


# ---- 3. worker1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def genomes(gold):
    out = []
    for gi in (0, 1):
        l_pac = int(gold[f"g{gi}_l_pac"])
        g = fu.unpack_pac(gold[f"g{gi}_pac"], l_pac)
        idx, _ = fu.build_index(g, 8)
        reads = [r for r in fu.split(gold[f"g{gi}_read_len"], gold[f"g{gi}_read_pool"]) if r.size > 0]
        tail = g[-20:]      # a read across the end of the forward strand: its seed bridges l_pac
        reads.append(np.concatenate([tail, (3 - tail[::-1]).astype(np.uint8)]))
        out.append((gold[f"g{gi}_pac"], g, idx, reads))
    return out


def _load(ctx, genome):
    pac, g, idx, _ = genome
    ctx.ref_load(pac, g.size)
    ctx.fmi_load(idx)


@pytest.mark.parametrize("gi", [0, 1])
@pytest.mark.parametrize("flags", [0, bpsw_hip.C2A_SORT_DEDUP])
@pytest.mark.parametrize("plan", [0, W1_PLAN])
def test_worker1_with_resident_chains_equals_worker1_without(ctx, gold, genomes, gi, flags, plan):
    from conftest import region_fields_equal
    _load(ctx, genomes[gi])
    reads = genomes[gi][3]
    so, opt = _opt(gold, f"c{gi}"), bpsw_hip.default_opt()
    rb = fmi.ReadBatch.from_list(reads)
    wcnt, wregs = ctx.worker1_batch(opt, so, rb, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=flags)
    cnt, regs = ctx.worker1_batch(opt, so, rb, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=flags | plan | RESIDENT)
    assert bpsw_hip.chain_last_split()[0] > len(reads) // 2
    assert np.array_equal(cnt, wcnt) and cnt.sum() > len(reads) // 2
    region_fields_equal(regs, wregs)
    assert all(t >= 0 for t in bpsw_hip.last_worker1_times())
    # the flag implies W1_CHAIN_DEVICE: naming both changes nothing
    cnt2, regs2 = ctx.worker1_batch(opt, so, rb, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=flags | plan | RESIDENT | bpsw_hip.W1_CHAIN_DEVICE)
    assert np.array_equal(cnt2, wcnt)
    region_fields_equal(regs2, wregs)


def test_worker1_with_resident_chains_beyond_the_resident_lanes(ctx, gold, genomes):
    """64 resident lanes of the seed kernel, 205 reads"""
    from conftest import region_fields_equal
    _load(ctx, genomes[1])
    reads = genomes[1][3]
    both = (reads + reads[::-1])[:205]
    assert len(both) == 205
    so, opt = _opt(gold, "c1"), bpsw_hip.default_opt()
    rb = fmi.ReadBatch.from_list(both)
    ctx.lib.bpsw_seed_set_resident_lanes(64)
    try:
        wcnt, wregs = ctx.worker1_batch(opt, so, rb, zdrop_mode=bpsw_hip.ZDROP_BWA)
        cnt, regs = ctx.worker1_batch(opt, so, rb, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=RESIDENT)
        cnt2, regs2 = ctx.worker1_batch(opt, so, rb, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=RESIDENT | W1_PLAN)
    finally:
        ctx.lib.bpsw_seed_set_resident_lanes(0)
    assert np.array_equal(cnt, wcnt) and np.array_equal(cnt2, wcnt)
    region_fields_equal(regs, wregs)
    region_fields_equal(regs2, wregs)


def test_worker1_capacity_contract(ctx, gold, genomes):
    from conftest import region_fields_equal
    _load(ctx, genomes[1])
    so, opt = _opt(gold, "c1"), bpsw_hip.default_opt()
    rb = fmi.ReadBatch.from_list(genomes[1][3])
    st, n = rb.as_struct(), rb.n_reads

    def call(flags, cap):
        out_cnt, out, total = np.zeros(n, np.int32), np.empty(max(cap, 1), bpsw_hip.ALNREG_DTYPE), C.c_int64(0)
        rc = ctx.lib.bpsw_worker1_batch(ctx.h, C.byref(opt), C.byref(so), C.byref(st), bpsw_hip.ZDROP_BWA, flags, bpsw_hip._ptr(out_cnt),
                                        bpsw_hip._ptr(out), cap, C.byref(total))
        return rc, out_cnt, out, total.value
    rc, _, _, need = call(0, 0)
    assert rc == ERR_CAPACITY and need > n // 2       # the seeds in kept chains
    for w1 in (RESIDENT, RESIDENT | W1_PLAN):
        assert call(w1, need - 1)[::3] == (ERR_CAPACITY, need)
        assert call(w1, 0)[::3] == (ERR_CAPACITY, need)
        rc, cnt, regs, total = call(w1, need)          # the retry with the returned capacity
        wrc, wcnt, wregs, wtotal = call(0, need)
        assert rc == 0 and wrc == 0 and total == wtotal and np.array_equal(cnt, wcnt)
        region_fields_equal(regs[:total], wregs[:wtotal])


# ---- 4. what crosses the bus in the chain stage ----------------------------------------------------------------------------------------------
def test_chain_stage_fetches_a_constant_with_the_flag(ctx, gold, genomes):
    _load(ctx, genomes[1])
    so, opt = _opt(gold, "c1"), bpsw_hip.default_opt()
    # the fixture's reads that stay below BPSW_CHAIN_DEV_MAX_SEEDS (128 occurrences of kept intervals): none is chained on the calling thread
    icnt, iv, _, _ = ctx.seed_batch(so, fmi.ReadBatch.from_list(genomes[1][3]))
    occ = [int(i["x2"][i["kept"] != 0].sum()) for i in fu.split(icnt, iv)]
    reads = [r for r, k in zip(genomes[1][3], occ) if k <= 128]
    assert len(genomes[1][3]) - 5 <= len(reads) < len(genomes[1][3])
    fetched = {}
    for n in (64, 4096):
        rb = fmi.ReadBatch.from_list([reads[i % len(reads)] for i in range(n)])
        ctx.worker1_batch(opt, so, rb, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=RESIDENT | W1_PLAN)
        st = bpsw_hip.chain_last_split()
        assert st[1] == 0 and st[2] == 1, st              # no read chained on the calling thread, one slice
        fetched[n] = bpsw_hip.last_chain_bytes()
        assert fetched[n][1] == FETCHED_PER_SLICE * 1 + FETCHED_ONCE, fetched
        assert fetched[n][0] > 12 * n                     # staged: item_read, item_work, seed_beg
    assert fetched[64][1] == fetched[4096][1]
    # without the flag the kept chains come back: 16 bytes a seed at least
    out_cnt, out, total = np.zeros(4096, np.int32), np.empty(1, bpsw_hip.ALNREG_DTYPE), C.c_int64(0)
    st = rb.as_struct()
    rc = ctx.lib.bpsw_worker1_batch(ctx.h, C.byref(opt), C.byref(so), C.byref(st), bpsw_hip.ZDROP_BWA, bpsw_hip.W1_CHAIN_DEVICE,
                                    bpsw_hip._ptr(out_cnt), bpsw_hip._ptr(out), 0, C.byref(total))
    assert rc == ERR_CAPACITY and total.value > 4096 // 2      # the seeds in kept chains
    assert bpsw_hip.last_chain_bytes()[1] >= 16 * total.value


# ---- 5. reads to SAM, the JNI ------------------------------------------------------------------------------------------------------------------
def test_align_se_and_pe_text_with_resident_chains(ctx, gold):
    from test_sam_pe_gpu import _paired_fixture
    from test_sam_se_gpu import NO_PES, TEXT_MODES, _contig_tables
    from test_sam_se_gpu import _load as load_all
    l_pac = int(gold["g1_l_pac"])
    g = fu.unpack_pac(gold["g1_pac"], l_pac)
    idx, _ = fu.build_index(g, 8)
    reads = fu.split(gold["g1_read_len"], gold["g1_read_pool"])
    rng = np.random.default_rng(105)
    quals = [rng.integers(35, 74, len(r)).astype(np.uint8) for r in reads]
    names = [b"frag%d/%s" % (i, b"x" * (i % 7)) for i in range(len(reads))]
    fixture_reads = (g, idx, reads, quals, names)
    table = _contig_tables(g.size)[1]
    load_all(ctx, gold["g1_pac"], g.size, table, idx)
    opt, so, topt = bpsw_hip.default_opt(), _opt(gold, "c1"), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    w1 = RESIDENT | W1_PLAN
    se = bpsw_hip.SeReadsSoA.from_lists(reads, names, quals, id0=1000, id_step=2)
    none = np.zeros(0, bpsw_hip.ALNREG_DTYPE)
    pairs = _paired_fixture(fixture_reads, np.zeros(len(reads), np.int32), none, table, NO_PES)
    bare = copy.copy(pairs)
    bare.reg_cnt, bare.regs, bare.pes = None, None, [(7, 7, 0, 7.0, 7.0)] * 4       # ignored
    for mode in TEXT_MODES:
        want = ctx.align_se_batch(opt, so, topt, se, zdrop_mode=bpsw_hip.ZDROP_BWA, w1_flags=0, flags=mode)
        got = ctx.align_se_batch(opt, so, topt, se, zdrop_mode=bpsw_hip.ZDROP_BWA, w1_flags=w1, flags=mode)
        assert len(want) == len(reads) and sum(t.count(b"\n") for t in want) >= len(reads)
        assert got == want, mode
        want, want_pes = ctx.align_pe_batch(opt, so, topt, bare, zdrop_mode=bpsw_hip.ZDROP_BWA, w1_flags=0, flags=mode)
        got, got_pes = ctx.align_pe_batch(opt, so, topt, bare, zdrop_mode=bpsw_hip.ZDROP_BWA, w1_flags=w1, flags=mode)
        assert len(want) == 104 and got_pes == want_pes
        assert got == want, mode


def test_worker1_flat_jni_with_resident_chains(ctx, gold, genomes, monkeypatch):
    from bpsw_hip import jnishim
    monkeypatch.setenv("BPSW_ZDROP", "bwa")
    pac, g, idx, reads = genomes[1]
    _load(ctx, genomes[1])
    rb = fmi.ReadBatch.from_list(reads)
    opt, so = bpsw_hip.default_opt(), _opt(gold, "c2")
    fake = jnishim.load_fake_worker1()
    rc, wcnt, wlongs, msg = jnishim.worker1_flat(fake, pac, g.size, idx, opt, so, bpsw_hip.C2A_SORT_DEDUP, rb)
    assert rc == 0, msg
    rc, cnt, longs, msg = jnishim.worker1_flat(fake, pac, g.size, idx, opt, so, bpsw_hip.C2A_SORT_DEDUP | W1_PLAN | RESIDENT, rb)
    assert rc == 0, msg
    assert np.array_equal(cnt, wcnt) and longs.shape[0] == wlongs.shape[0] > 0 and np.array_equal(longs, wlongs)


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "parity" and sys.argv[2] in ("lists0", "lists1", "shapes", "all")
    part = sys.argv[2]
    limit = int(os.environ["BPSW_CHAIN_DEV_MAX_SEEDS"])
    c = bpsw_hip.Context(0)
    L = cl.cases()
    if part in ("lists0", "all"):
        check_golden(c, np.load(fu.GOLDEN))
    if part != "shapes":
        check_lists(c, L, {"lists0": 0, "lists1": 1, "all": None}[part])
    if part in ("shapes", "all"):
        split = check_shapes(c, L)
        assert (split[1] == 0 and split[0] > 20) if limit == 0 else (split[1] > 10 and split[0] + split[1] <= 41), split
        st3, st1 = check_arena_budget(c)
        assert (st3[0], st3[1]) == ((90, 0) if limit == 0 else (0, 90)), st3
        st = check_scan_levels(c)
        assert st[0] + st[1] > 3000 and (st[1] == 0 if limit == 0 else st[1] > 1000), st
    c.close()
    print("parity OK")
