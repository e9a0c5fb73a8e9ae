#!/usr/bin/env python3
"""Throughput of worker1 from reads (bpsw_seed_batch, the chain stage on the host and on the device, bpsw_worker1_batch) on a
synthetic genome, next to the reference's mem_chain on the same reads from oracle/_ref/libbwaref.so on 16 threads where that
library is built.

    python tools/seed_throughput.py [--genome-mb 50] [--reads 100000] [--read-len 150] [--sa-intv 32] [--reps 5] [--threads 16]
                                    [--seed-plan-device] [--chains-resident] [--out profiles/seed_throughput.json]

The chain stage both ways is slot 1 of bpsw_last_worker1_times without and with BPSW_W1_CHAIN_DEVICE on the same batch.  The
long-read threshold (BPSW_CHAIN_DEV_MAX_SEEDS) is read once per process, and reads of a random genome have a handful of seeds,
so its settings are measured in child processes on bpsw_chain_batch over the batch's own seeds plus --long-reads generated
reads of L seeds each (tests/chain_lists.py), for every L of --long-seeds: at 0 the kernel chains them, at a threshold below L
(2 048 for L above it) the calling thread does.

The index is built here (numpy): a random genome has practically no repeated 27-mer, so the suffix array is one sort by the
27-base prefix and a byte-wise comparison inside the few groups that tie.  After one warm-up call the median of --reps calls is
reported, one JSON line.  The three stage times of a bpsw_worker1_batch call come from bpsw_last_worker1_times.

--seed-plan-device adds the seeding stage both ways: bpsw_worker1_batch without and with BPSW_W1_SEED_PLAN_DEVICE, each without and
with BPSW_W1_CHAIN_DEVICE, the four settings taken in turn within every repetition after one warm-up round.  Per setting and
repetition it prints the three stage times, the calling thread's CPU time over the whole call (the stages after seeding are the same
code both ways, so a difference is the seeding stage's) and the H2D / D2H bytes of the seeding stage from bpsw_last_seed_bytes.  A
library without the flag (BPSW_LIB pointing at an older build) is measured on the two settings it has.

--chains-resident adds BPSW_W1_CHAINS_RESIDENT to that rotation (with the plan on the host, and on the device under
--seed-plan-device), and per setting the H2D / D2H bytes of the chain stage from bpsw_last_chain_bytes, the chain stage's, the round
loop call's and the whole call's median."""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cloud-scale-bwamem_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import bpsw_hip  # noqa: E402
import fmi_util as fu  # noqa: E402
import pyoracle  # noqa: E402
from bpsw_hip import fmi  # noqa: E402

K = 27  # 5^27 < 2^63: the prefix of K bases (digit = base + 1, 0 past the end) as one integer


def suffix_array_random_text(text):
    n = text.size
    digits = np.zeros(n + K, np.int64)
    digits[:n] = text.astype(np.int64) + 1
    key = np.zeros(n, np.int64)
    for j in range(K):
        key *= 5
        key += digits[j: j + n]
    order = np.argsort(key, kind="stable")
    ks = key[order]
    ties = np.nonzero(ks[1:] == ks[:-1])[0]
    if ties.size:
        b = text.tobytes()
        starts = ties[np.concatenate([[True], np.diff(ties) > 1])]
        for s in starts:
            e = s + 1
            while e < n and ks[e] == ks[s]:
                e += 1
            grp = sorted(order[s:e].tolist(), key=lambda i: b[i:])
            order[s:e] = grp
    return np.concatenate([[n], order]).astype(np.int64), int(ties.size)


def build_index(fwd, sa_intv):
    text = fu.doubled(fwd)
    n = text.size
    sa, n_ties = suffix_array_random_text(text)
    primary = int(np.nonzero(sa == 0)[0][0])
    bwt = text[sa[sa != 0] - 1]
    L2 = np.zeros(5, np.int64)
    L2[1:] = np.cumsum(np.bincount(text, minlength=4))
    n_words, n_blk = (n + 15) // 16, (n + 127) // 128
    padded = np.zeros(n_blk * 128, np.uint32)
    padded[:n] = bwt
    words = np.zeros(n_blk * 8, np.uint32)
    for j in range(16):
        words |= padded[j::16] << np.uint32(30 - 2 * j)
    cnt = np.zeros((n_blk + 1, 4), np.uint64)
    for c in range(4):
        per = (padded.reshape(n_blk, 128) == c).sum(axis=1).astype(np.uint64)
        if c == 0:
            per[-1] -= np.uint64(n_blk * 128 - n)   # the padding reads as A
        cnt[1:, c] = np.cumsum(per)
    arr = np.zeros((n_blk, 16), np.uint32)
    arr[:, :8] = cnt[:n_blk].view(np.uint32).reshape(n_blk, 8)
    arr[:, 8:] = words.reshape(n_blk, 8)
    flat = arr.reshape(-1)[: (n_blk - 1) * 16 + 8 + (n_words - (n_blk - 1) * 8)]
    flat = np.ascontiguousarray(np.concatenate([flat, cnt[n_blk].view(np.uint32)]))
    assert flat.size == n_words + (n_blk + 1) * 8
    samp = sa[::sa_intv].copy()
    samp[0] = -1
    return fmi.FmIndex(primary=primary, L2=L2, seq_len=n, bwt=flat, sa_intv=sa_intv, sa=samp), n_ties


def make_reads(fwd, n, ln, rng):
    pos = rng.integers(0, fwd.size - ln, n)
    pool = fwd[(pos[:, None] + np.arange(ln)[None, :])].astype(np.uint8)
    mut = rng.random((n, ln)) < 0.01
    pool = np.where(mut, (pool + rng.integers(1, 4, (n, ln))) & 3, pool).astype(np.uint8)
    rev = rng.random(n) < 0.5
    pool[rev] = 3 - pool[rev, ::-1]
    return fmi.ReadBatch(np.full(n, ln, np.int32), (np.arange(n, dtype=np.int64) * ln), np.ascontiguousarray(pool.reshape(-1)))


def reference_mem_chain(idx, l_pac, rb, threads):
    ref = fu.RefSeeding(pyoracle.REF_SO)
    bwt = fu.ref_bwt(idx)
    o = ref.opt()
    n, ln = rb.n_reads, int(rb.read_len[0])
    base = rb.read_pool.ctypes.data

    def work(lo, hi):
        for r in range(lo, hi):
            v = ref.lib.mem_chain(o, C.addressof(bwt), l_pac, ln, C.c_void_p(base + r * ln))
            for i in range(v.n):
                ref.libc.free(v.a[i].seeds)
            if v.a:
                ref.libc.free(v.a)
    cuts = np.linspace(0, n, threads + 1).astype(int)
    ts = [threading.Thread(target=work, args=(cuts[i], cuts[i + 1])) for i in range(threads)]
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return n / (time.perf_counter() - t0)


def chain_child(path, reps):
    """bpsw_chain_batch over the seeds in `path` at this process's BPSW_CHAIN_DEV_MAX_SEEDS: median wall ms and the split"""
    d = np.load(path)
    ctx = bpsw_hip.Context(0)
    so, w = bpsw_hip.default_seed_opt(), bpsw_hip.default_opt().w
    ms = []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        ctx.chain_batch(so, w, int(d["l_pac"]), d["cnt"], d["seeds"], filter=True)
        if k:
            ms.append(1e3 * (time.perf_counter() - t0))
    split = bpsw_hip.chain_last_split()
    ctx.close()
    print(json.dumps({"ms": round(float(np.median(ms)), 2), "reads_on_device": split[0], "reads_on_host": split[1], "slices": split[2],
                      "arena_bytes": split[3]}))


def threshold_runs(scnt, sv, l_pac, n_long, sizes, reps):
    """per size L: the batch's seeds plus n_long generated reads of L seeds through bpsw_chain_batch in child processes, once with
    BPSW_CHAIN_DEV_MAX_SEEDS=0 (the kernel chains them) and once with the threshold below L (the calling thread does; 2 048 where L
    is above it)"""
    import subprocess
    import tempfile
    import chain_lists as cl
    rng = np.random.default_rng(7)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for L in sizes:
            longs = [cl.clustered(L, rng, l_pac=l_pac, spots=max(2, L // 8)) for _ in range(n_long)]
            path = os.path.join(tmp, f"seeds_{L}.npz")
            np.savez(path, cnt=np.concatenate([scnt, np.full(n_long, L, np.int32)]).astype(np.int32), seeds=np.concatenate([sv] + longs),
                     l_pac=np.int64(l_pac))
            res = {}
            for limit in (0, min(2048, L - 1)):
                env = dict(os.environ, BPSW_CHAIN_DEV_MAX_SEEDS=str(limit))
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--chain-child", path, "--reps", str(reps)], env=env,
                                   capture_output=True, text=True, check=True)
                res[f"max_seeds_{limit}"] = json.loads(p.stdout.strip().splitlines()[-1])
            out[f"long_reads_of_{L}_seeds"] = res
    return out


def seed_plan_runs(ctx, opt, so, rb, reps, plan=True, resident=False):
    """worker1_batch on the settings of (seeding plan on the host / the device) x (chaining on the host / the device / the device with
    the chains resident), in turn; those the library has"""
    has_plan = plan and hasattr(ctx.lib, "bpsw_seed_batch_ex")
    has_resident = resident and hasattr(ctx.lib, "bpsw_chain_batch_ex")
    has_chain_bytes = hasattr(ctx.lib, "bpsw_last_chain_bytes")
    settings = {"plan_host__chain_host": 0, "plan_host__chain_device": bpsw_hip.W1_CHAIN_DEVICE}
    if has_resident:
        settings["plan_host__chains_resident"] = bpsw_hip.W1_CHAINS_RESIDENT
    if has_plan:
        settings["plan_device__chain_host"] = bpsw_hip.W1_SEED_PLAN_DEVICE
        settings["plan_device__chain_device"] = bpsw_hip.W1_SEED_PLAN_DEVICE | bpsw_hip.W1_CHAIN_DEVICE
        if has_resident:
            settings["plan_device__chains_resident"] = bpsw_hip.W1_SEED_PLAN_DEVICE | bpsw_hip.W1_CHAINS_RESIDENT
    runs = {k: {"stage_ms": [], "call_ms": [], "thread_cpu_ms": [], "seed_bytes_h2d_d2h": None, "chain_bytes_h2d_d2h": None} for k in settings}
    want = None
    for k in range(reps + 1):
        for name, fl in settings.items():
            c0, t0 = time.thread_time(), time.perf_counter()
            cnt, regs = ctx.worker1_batch(opt, so, rb, flags=bpsw_hip.C2A_SORT_DEDUP | fl)
            t1, c1 = time.perf_counter(), time.thread_time()
            if want is None:
                want = (cnt.copy(), regs.copy())
            assert np.array_equal(cnt, want[0]) and regs.tobytes() == want[1].tobytes(), f"{name} changed the regions"
            if k:
                r = runs[name]
                r["stage_ms"].append([round(x, 2) for x in bpsw_hip.last_worker1_times()])
                r["call_ms"].append(round(1e3 * (t1 - t0), 2))
                r["thread_cpu_ms"].append(round(1e3 * (c1 - c0), 2))
                if hasattr(ctx.lib, "bpsw_last_seed_bytes"):
                    r["seed_bytes_h2d_d2h"] = list(ctx.last_seed_bytes())
                if has_chain_bytes and fl & ~bpsw_hip.W1_SEED_PLAN_DEVICE:
                    r["chain_bytes_h2d_d2h"] = list(bpsw_hip.last_chain_bytes())
    for r in runs.values():
        r["seeding_call_ms_median"] = round(float(np.median([s[0] for s in r["stage_ms"]])), 2)
        r["chain_stage_ms_median"] = round(float(np.median([s[1] for s in r["stage_ms"]])), 2)
        r["round_loop_call_ms_median"] = round(float(np.median([s[2] for s in r["stage_ms"]])), 2)
        r["call_ms_median"] = round(float(np.median(r["call_ms"])), 2)
        r["thread_cpu_ms_median"] = round(float(np.median(r["thread_cpu_ms"])), 2)
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=50.0)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--sa-intv", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--long-reads", type=int, default=64)
    ap.add_argument("--long-seeds", default="64,128,512,3000", help="'' leaves the long-read runs out")
    ap.add_argument("--seed-plan-device", action="store_true", help="also measure the seeding stage with its plan on the host and on the device")
    ap.add_argument("--chains-resident", action="store_true",
                    help="add BPSW_W1_CHAINS_RESIDENT to the rotation (alone, and with the plan on the device under --seed-plan-device)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seed_throughput.json"))
    ap.add_argument("--chain-child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.chain_child:
        return chain_child(a.chain_child, a.reps)
    rng = np.random.default_rng(20260101)
    l_pac = int(a.genome_mb * 1e6) | 1
    fwd = rng.integers(0, 4, l_pac).astype(np.uint8)
    t0 = time.perf_counter()
    idx, n_ties = build_index(fwd, a.sa_intv)
    t_build = time.perf_counter() - t0
    rb = make_reads(fwd, a.reads, a.read_len, rng)
    ctx = bpsw_hip.Context(0)
    ctx.ref_load(fu.pack_pac(fwd), l_pac)
    ctx.fmi_load(idx)
    opt, so = bpsw_hip.default_opt(), bpsw_hip.default_seed_opt()
    seed_s, w1_s, stages, w1d_s, stages_dev = [], [], [], [], []
    n_intv = n_seeds = n_regs = 0
    for k in range(a.reps + 1):
        t0 = time.perf_counter()
        icnt, iv, scnt, sv = ctx.seed_batch(so, rb)
        t1 = time.perf_counter()
        cnt, regs = ctx.worker1_batch(opt, so, rb, flags=bpsw_hip.C2A_SORT_DEDUP)
        t2 = time.perf_counter()
        if k:
            seed_s.append(t1 - t0); w1_s.append(t2 - t1); stages.append(bpsw_hip.last_worker1_times())
        t2 = time.perf_counter()
        dcnt, dregs = ctx.worker1_batch(opt, so, rb, flags=bpsw_hip.C2A_SORT_DEDUP | bpsw_hip.W1_CHAIN_DEVICE)
        t3 = time.perf_counter()
        if k:
            w1d_s.append(t3 - t2); stages_dev.append(bpsw_hip.last_worker1_times())
        split = bpsw_hip.chain_last_split()
        assert np.array_equal(cnt, dcnt) and all(np.array_equal(regs[f], dregs[f]) for f in regs.dtype.names), "device chaining changed the regions"
        n_intv, n_seeds, n_regs = int(icnt.sum()), int(scnt.sum()), int(cnt.sum())
    st = np.median(np.array(stages), axis=0)
    sd = np.median(np.array(stages_dev), axis=0)
    res = {
        "genome_bases": l_pac, "index_bytes": int(idx.bwt.nbytes + idx.sa.nbytes), "sa_intv": a.sa_intv, "index_build_s": round(t_build, 1),
        "tied_27mers": n_ties, "reads": a.reads, "read_len": a.read_len, "reps": a.reps,
        "intervals_per_read": round(n_intv / a.reads, 2), "seeds_per_read": round(n_seeds / a.reads, 2), "regions_per_read": round(n_regs / a.reads, 2),
        "seed_batch_reads_per_s": round(a.reads / float(np.median(seed_s))),
        "worker1_batch_reads_per_s": round(a.reads / float(np.median(w1_s))),
        "worker1_stage_ms": {"seeding_call": round(float(st[0]), 2), "host_chaining": round(float(st[1]), 2), "round_loop_call": round(float(st[2]), 2)},
        "seeding_stage_reads_per_s": round(a.reads / (float(st[0]) / 1e3)),
        "host_chaining_reads_per_s": round(a.reads / max(float(st[1]) / 1e3, 1e-9)),
        "round_loop_reads_per_s": round(a.reads / max(float(st[2]) / 1e3, 1e-9)),
    }
    res["bound_by"] = ("seeding_call", "host_chaining", "round_loop_call")[int(np.argmax(st))]
    res["chain_stage_ms"] = {"host": round(float(st[1]), 2), "device": round(float(sd[1]), 2)}
    res["device_chaining"] = {
        "worker1_batch_reads_per_s": round(a.reads / float(np.median(w1d_s))),
        "worker1_stage_ms": {"seeding_call": round(float(sd[0]), 2), "device_chaining": round(float(sd[1]), 2), "round_loop_call": round(float(sd[2]), 2)},
        "reads_on_device": split[0], "reads_on_host": split[1], "slices": split[2], "arena_bytes": split[3],
        "max_seeds_in_a_read": int(scnt.max()),
    }
    if a.seed_plan_device or a.chains_resident:
        res["seed_plan"] = seed_plan_runs(ctx, opt, so, rb, a.reps, plan=a.seed_plan_device, resident=a.chains_resident)
        for name, r in res["seed_plan"].items():
            print(f"{name}: stages (seeding, chaining, round loop) ms {r['stage_ms']}; call ms {r['call_ms']}; thread CPU ms {r['thread_cpu_ms']}; "
                  f"seeding stage H2D / D2H bytes {r['seed_bytes_h2d_d2h']}; chain stage H2D / D2H bytes {r['chain_bytes_h2d_d2h']}", file=sys.stderr)
    if a.long_seeds:
        res["chain_batch_with_long_reads"] = dict(threshold_runs(scnt, sv, l_pac, a.long_reads, [int(x) for x in a.long_seeds.split(",")], a.reps),
                                                  long_reads=a.long_reads)
    if os.path.exists(pyoracle.REF_SO):
        res["reference_mem_chain_reads_per_s"] = round(reference_mem_chain(idx, l_pac, rb, a.threads))
        res["reference_threads"] = a.threads
    ctx.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
