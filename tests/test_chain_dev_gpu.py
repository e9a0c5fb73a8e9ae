"""bpsw_chain_batch (chain_kernel + chain_emit_kernel, csrc/bpsw_chain_dev.hip: one read per lane over the algorithm of
csrc/bpsw_chain_core.h) and bpsw_worker1_batch with BPSW_W1_CHAIN_DEVICE: against the reference's chains as recorded in
tests/golden/seed_chain_small.npz, against bpsw_chain_seeds on the generated lists of tests/chain_lists.py packed into batches
around the wavefront, with one long read among short ones, with the arena budget lowered (several slices; a read larger than the
budget), and worker1 with the flag against worker1 without it.  BPSW_CHAIN_DEV_MAX_SEEDS is read once per process: the parity
checks run in this process at the default (reads above 128 seeds are chained on the calling thread) and once more in a child
process at 0, where the kernel chains every read.  (Run as `python tests/test_chain_dev_gpu.py parity` this file is that child.)"""
import ctypes as C
import os
import subprocess
import sys
import threading

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


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    for f in a.dtype.names:
        assert np.array_equal(a[f], b[f]), (what, f, int((a[f] != b[f]).sum()))


def _opt(gold, key):
    d = dict(zip(fu.SEED_OPT_FIELDS, gold[key + "_opt"]))
    return fu.sopt_from({k: (float(v) if k in ("split_factor", "chain_drop_ratio", "mask_level") else int(v)) for k, v in d.items()})


# ---- the checks, shared by the suite's process and the child ------------------------------------------------------------------
def check_golden(ctx, gold):
    """all reads of each fixture config in one call, filter off and on"""
    w = bpsw_hip.default_opt().w
    for ci, (gi, _) in enumerate(gold["configs"]):
        key = f"c{ci}"
        so, l_pac = _opt(gold, key), int(gold[f"g{int(gi)}_l_pac"])
        for filt, a, b, c in ((False, "_chain_cnt", "_chain_seed_cnt", "_chain_seeds"), (True, "_flt_cnt", "_flt_seed_cnt", "_flt_seeds")):
            cc, sc, out = ctx.chain_batch(so, w, l_pac, gold[key + "_seed_cnt"], gold[key + "_seeds"], filter=filt)
            assert np.array_equal(cc, gold[key + a]), (key, filt)
            assert np.array_equal(sc, gold[key + b]), (key, filt)
            _same(out, gold[key + c], (key, filt))
        assert bpsw_hip.chain_last_split()[0] > 0


def _expected(so, w, l_pac, per_read, filt):
    cc, sc, out = [], [], []
    for s in per_read:
        cnt, o = bpsw_hip.chain_seeds(so, w, l_pac, s, filter=filt)
        cc.append(cnt.size); sc.append(cnt); out.append(o)
    return (np.array(cc, np.int32), np.concatenate(sc + [np.zeros(0, np.int32)]).astype(np.int32),
            np.concatenate(out + [np.zeros(0, fmi.SEED_DTYPE)]))


def check_batch(ctx, per_read, what, od=None, w=100, l_pac=cl.L_PAC, filters=(False, True)):
    so = cl.sopt(od or {})
    cnt, flat = fu.flat(per_read, fmi.SEED_DTYPE)
    for filt in filters:
        want = _expected(so, w, l_pac, per_read, filt)
        got = ctx.chain_batch(so, w, l_pac, cnt, flat, filter=filt)
        assert np.array_equal(got[0], want[0]), (what, filt)
        assert np.array_equal(got[1], want[1]), (what, filt)
        _same(got[2], want[2], (what, filt))
    return bpsw_hip.chain_last_split()


def _default_lists(lists):
    """the generated lists that share the default options, w and l_pac: they can lie in one batch"""
    return [c[4] for c in lists if not c[1] and c[2] == 100 and c[3] == cl.L_PAC]


def _short_lists(lists, rng, n):
    pool = [s for s in _default_lists(lists) if s.size <= 40]
    return [pool[i] for i in rng.integers(0, len(pool), n)]


def check_generated(ctx, lists):
    """every generated list as a batch of its own (its options), then the shapes of the batch"""
    for name, od, w, l_pac, seeds in lists:
        check_batch(ctx, [seeds], name, od, w, l_pac)
    rng = np.random.default_rng(11)
    mixed = _default_lists(lists)
    for n in (63, 64, 65):
        check_batch(ctx, [mixed[i] for i in rng.integers(0, len(mixed), n)], f"{n} reads", filters=(True,))
    # one read of 3 000 seeds among 199 of 0-5: divergence, workspace offsets, the count-ordered dealing
    few = [cl.clustered(int(k), rng, spots=2) for k in rng.integers(0, 6, 199)]
    long_one = next(c[4] for c in lists if c[0] == "long_3000")
    st = check_batch(ctx, few[:120] + [long_one] + few[120:], "one long read among 199 short")
    empty = np.zeros(0, fmi.SEED_DTYPE)
    check_batch(ctx, [empty] + _short_lists(lists, rng, 20) + [empty, empty], "first and last reads without seeds", filters=(True,))
    check_batch(ctx, [empty, empty], "no seeds at all", filters=(True,))
    return st


def check_arena_budget(ctx, lists):
    """with the budget lowered: a batch in three slices, and a single read larger than the budget"""
    rng = np.random.default_rng(12)
    reads = [cl.clustered(60, rng, spots=5) for _ in range(90)]
    per_read = 16 + 52 * 60 + 256 * (60 // 7 + 2) + 896      # the slice of a read of 60 seeds (csrc/bpsw_chain_core.h)
    lib = bpsw_hip.load_library()
    try:
        lib.bpsw_chain_set_arena_budget(30 * per_read + 8)
        st = check_batch(ctx, reads, "three slices", filters=(True,))
        assert st[0] == 90 and st[2] == 3 and st[3] == 30 * per_read, st
        big = cl.clustered(120, rng, spots=10)              # its slice: 16 + 52 * 120 + 256 * 19 + 896 = 12 016 bytes
        lib.bpsw_chain_set_arena_budget(7000)               # one read of 60 seeds fits, two do not, the read of 120 does not
        st = check_batch(ctx, [reads[0], big, reads[1]], "a read larger than the budget", filters=(True,))
        assert st[0] == 3 and st[2] == 3 and st[3] == 12016, st
    finally:
        lib.bpsw_chain_set_arena_budget(0)


# ---- the suite ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(fu.GOLDEN)


@pytest.fixture(scope="module")
def lists():
    return cl.cases()


def test_golden_parity(ctx, gold):
    check_golden(ctx, gold)


def _long_on_host():
    """whether a read of 3 000 seeds stays on the calling thread in this process (BPSW_CHAIN_DEV_MAX_SEEDS, default 128)"""
    limit = int(os.environ.get("BPSW_CHAIN_DEV_MAX_SEEDS") or 128)
    return 0 < limit < 3000


def test_generated_lists_and_batch_shapes(ctx, lists):
    st = check_generated(ctx, lists)      # (the split of the batch with the read of 3 000 seeds)
    assert st[1] == (1 if _long_on_host() else 0), st


def test_long_read_is_merged_in_read_order(ctx, lists):
    long_one = next(c[4] for c in lists if c[0] == "long_3000")
    short = next(c[4] for c in lists if c[0] == "distinct_18")
    st = check_batch(ctx, [short, long_one, short], "merge in read order")
    assert st[:3] == ((2, 1, 1) if _long_on_host() else (3, 0, 1)), st
    st = check_batch(ctx, [long_one], "the long read alone")
    assert st[:3] == ((0, 1, 0) if _long_on_host() else (1, 0, 1)), st


def test_arena_budget_slices_and_a_read_beyond_it(ctx, lists):
    check_arena_budget(ctx, lists)


def test_everything_on_the_device_in_a_child_process():
    """BPSW_CHAIN_DEV_MAX_SEEDS=0: the kernel chains every read, the 2 000-chain and 3 000-seed ones included"""
    env = dict(os.environ, BPSW_CHAIN_DEV_MAX_SEEDS="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "parity"], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "parity OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def test_refusals(ctx, lists):
    so, lib = bpsw_hip.default_seed_opt(), bpsw_hip.load_library()
    reads = _short_lists(lists, np.random.default_rng(3), 30)
    cnt, flat = fu.flat(reads, fmi.SEED_DTYPE)
    want = _expected(so, 100, cl.L_PAC, reads, True)
    chain_cnt = np.zeros(cnt.size, np.int32)
    ct, st = C.c_int64(0), C.c_int64(0)

    def call(n, scnt, seeds, ccap, scap):
        sc, out = np.zeros(max(ccap, 1), np.int32), np.zeros(max(scap, 1), fmi.SEED_DTYPE)
        rc = lib.bpsw_chain_batch(ctx.h, C.byref(so), 100, cl.L_PAC, n, scnt.ctypes.data, seeds.ctypes.data, 1, chain_cnt.ctypes.data,
                                  sc.ctypes.data, ccap, out.ctypes.data, scap, C.byref(ct), C.byref(st))
        return rc, sc, out
    assert want[1].size > 2 and want[2].shape[0] > 2
    for ccap, scap in ((want[1].size - 1, want[2].shape[0]), (want[1].size, want[2].shape[0] - 1), (0, 0)):
        rc, _, _ = call(cnt.size, cnt, flat, ccap, scap)
        assert rc == ERR_CAPACITY and (ct.value, st.value) == (want[1].size, want[2].shape[0])
    rc, sc, out = call(cnt.size, cnt, flat, ct.value, st.value)     # a second call with the totals succeeds
    assert rc == 0 and np.array_equal(chain_cnt, want[0]) and np.array_equal(sc, want[1])
    _same(out, want[2], "after the capacity error")
    assert flat.shape[0] >= want[2].shape[0] and flat.shape[0] >= want[1].size     # the sum of seed_cnt always suffices
    for field, v in (("len", 0), ("qbeg", -1)):
        bad = flat.copy()
        bad[field][bad.shape[0] // 2] = v
        assert call(cnt.size, cnt, bad, flat.shape[0], flat.shape[0])[0] == ERR_ARG
    ct.value = st.value = 7
    assert call(0, cnt, flat, 0, 0)[0] == 0 and (ct.value, st.value) == (0, 0)     # n_reads == 0


# ---- worker1 ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def genomes(gold):
    out = []
    for gi in (0, 1):
        l_pac = int(gold[f"g{gi}_l_pac"])
        g = fu.unpack_pac(gold[f"g{gi}_pac"], l_pac)
        idx, _ = fu.build_index(g, 8)
        reads = [r for r in fu.split(gold[f"g{gi}_read_len"], gold[f"g{gi}_read_pool"]) if r.size > 0]
        # a read that lies across the end of the forward strand in the doubled sequence: the genome's last 20 bases and their
        # reverse complement; its seed starts below l_pac and ends above it
        tail = g[-20:]
        reads.append(np.concatenate([tail, (3 - tail[::-1]).astype(np.uint8)]))
        out.append((gold[f"g{gi}_pac"], g, idx, reads))
    return out


def _load(ctx, genome):
    pac, g, idx, _ = genome
    ctx.ref_load(pac, g.size)
    ctx.fmi_load(idx)


def _bridging_dropped(ctx, genome, so):
    """how many seeds of the bridging read the plain path dropped: occurrences of its kept intervals minus the seeds it has"""
    _, g, _, reads = genome
    icnt, iv, scnt, _ = ctx.seed_batch(so, fmi.ReadBatch.from_list(reads[-1:]))
    return int(iv["x2"][iv["kept"] == 1].sum()) - int(scnt[0])


@pytest.mark.parametrize("gi", [0, 1])
@pytest.mark.parametrize("flags", [0, bpsw_hip.C2A_SORT_DEDUP])
def test_worker1_with_device_chaining_equals_worker1_without(ctx, gold, genomes, gi, flags):
    from conftest import region_fields_equal
    _load(ctx, genomes[gi])
    reads = genomes[gi][3]
    so, opt = _opt(gold, f"c{gi}"), bpsw_hip.default_opt()       # (config 0 is genome 0's, config 1 genome 1's)
    assert _bridging_dropped(ctx, genomes[gi], so) >= 1      # the device-side drop has something to drop
    rb = fmi.ReadBatch.from_list(reads)
    wcnt, wregs = ctx.worker1_batch(opt, so, rb, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=flags)
    cnt, regs = ctx.worker1_batch(opt, so, rb, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=flags | bpsw_hip.W1_CHAIN_DEVICE)
    assert bpsw_hip.chain_last_split()[0] > len(reads) // 2
    assert np.array_equal(cnt, wcnt) and cnt.sum() > len(reads) // 2
    region_fields_equal(regs, wregs)
    assert all(t >= 0 for t in bpsw_hip.last_worker1_times())


def test_worker1_with_device_chaining_beyond_the_resident_lanes(ctx, gold, genomes):
    """64 resident lanes of the seed kernel, 205 reads, as tests/test_seed_gpu.py has it"""
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
        cnt, regs = ctx.worker1_batch(opt, so, rb, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=bpsw_hip.W1_CHAIN_DEVICE)
    finally:
        ctx.lib.bpsw_seed_set_resident_lanes(0)
    assert np.array_equal(cnt, wcnt)
    region_fields_equal(regs, wregs)


def test_two_threads_two_contexts(lists):
    """the same batch concurrently on two contexts (each with its own arena): identical results"""
    rng = np.random.default_rng(21)
    reads = _short_lists(lists, rng, 150) + [next(c[4] for c in lists if c[0] == "distinct_300_shuffled")]
    cnt, flat = fu.flat(reads, fmi.SEED_DTYPE)
    so = bpsw_hip.default_seed_opt()
    want = _expected(so, 100, cl.L_PAC, reads, True)
    ctxs = [bpsw_hip.Context(0), bpsw_hip.Context(0)]
    got, errs = [None, None], []

    def work(k):
        try:
            for _ in range(4):
                got[k] = ctxs[k].chain_batch(so, 100, cl.L_PAC, cnt, flat, filter=True)
        except Exception as e:    # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=work, args=(k,)) for k in (0, 1)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for c in ctxs:
        c.close()
    assert not errs, errs
    for k in (0, 1):
        assert np.array_equal(got[k][0], want[0]) and np.array_equal(got[k][1], want[1])
        _same(got[k][2], want[2], f"thread {k}")


if __name__ == "__main__":
    assert sys.argv[1:] == ["parity"]
    c = bpsw_hip.Context(0)
    L = cl.cases()
    check_golden(c, np.load(fu.GOLDEN))
    split = check_generated(c, L)
    check_arena_budget(c, L)
    st = check_batch(c, [next(x[4] for x in L if x[0] == "long_3000")], "the long read alone")
    assert st[:2] == (1, 0), st      # chained by the kernel
    c.close()
    print("parity OK")
