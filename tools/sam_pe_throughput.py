#!/usr/bin/env python3
"""Throughput of the paired tail from region lists to SAM text (bpsw_sam_pe_batch_ex) with the text written on the calling thread
and on the device (BPSW_SAM_TEXT_DEVICE), and the stage split of bpsw_align_pe_batch (paired reads to text in one call), on
synthetic FR pairs of 150-base reads of a random genome.

    python tools/sam_pe_throughput.py [--genome-mb 8] [--pairs 100000] [--read-len 150] [--sa-intv 32] [--reps 5]
                                      [--out profiles/sam_pe_throughput.json]

The regions are bpsw_worker1_batch's on the 2n reads (index built here as tools/seed_throughput.py builds it), the insert-size
statistics bpsw_pe_stat's over them.  After one warm-up call the median of --reps calls is reported, one JSON line: pairs/s of
bpsw_sam_pe_batch_ex both ways (the C call alone, into a buffer that fits), the three host stages of bpsw_last_tail_times both
ways, the two text kernels' times, the line table's and the text round trip's, and bpsw_align_pe_batch's worker1 / statistics /
rescue / tail split both ways.  The two texts are compared byte for byte."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cloud-scale-bwamem_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import bpsw_hip  # noqa: E402
import fmi_util as fu  # noqa: E402
import seed_throughput as st  # noqa: E402
from bpsw_hip import fmi  # noqa: E402
from sam_se_throughput import timed_calls  # noqa: E402


def make_pairs(fwd, n, ln, rng):
    """n FR pairs with inserts of 200 to 500, 1 % substitutions, half of them with the ends swapped"""
    ins = rng.integers(200, 501, n)
    pos = rng.integers(0, fwd.size - 500, n)
    a = fwd[(pos[:, None] + np.arange(ln)[None, :])]
    b = 3 - fwd[((pos + ins)[:, None] - 1 - np.arange(ln)[None, :])]
    swap = rng.random(n) < 0.5
    first, second = np.where(swap[:, None], b, a), np.where(swap[:, None], a, b)
    pool = np.stack([first, second], axis=1).reshape(2 * n, ln).astype(np.uint8)
    mut = rng.random(pool.shape) < 0.01
    pool = np.where(mut, (pool + rng.integers(1, 4, pool.shape)) & 3, pool).astype(np.uint8)
    return fmi.ReadBatch(np.full(2 * n, ln, np.int32), (np.arange(2 * n, dtype=np.int64) * ln), np.ascontiguousarray(pool.reshape(-1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=8.0)
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--sa-intv", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_pe_throughput.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(20261019)
    l_pac = int(a.genome_mb * 1e6) | 1
    fwd = rng.integers(0, 4, l_pac).astype(np.uint8)
    idx, _ = st.build_index(fwd, a.sa_intv)
    n = a.pairs
    rb = make_pairs(fwd, n, a.read_len, rng)
    ctx = bpsw_hip.Context(0)
    ctx.ref_load(fu.pack_pac(fwd), l_pac)
    ctx.bns_load(np.array([0], np.int64), np.array([l_pac], np.int32), ["chrSynthetic"])
    ctx.fmi_load(idx)
    opt, so, topt = bpsw_hip.default_opt(), bpsw_hip.default_seed_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    cnt, regs = ctx.worker1_batch(opt, so, rb, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=bpsw_hip.C2A_SORT_DEDUP)
    pes = bpsw_hip.pe_stat(opt, topt, l_pac, cnt, regs)
    names = [b"synthetic.%07d" % i for i in range(n)]
    name_off = np.zeros(n + 1, np.int64)
    name_off[1:] = np.cumsum([len(s) for s in names])
    g = bpsw_hip.TailGroupSoA(group_size=n, l_pac=l_pac, id0=0, pes=pes, read_len=rb.read_len, read_off=rb.read_off, read_pool=rb.read_pool,
                              qual_pool=rng.integers(35, 74, rb.read_pool.size).astype(np.uint8), name_off=name_off,
                              name_pool=np.frombuffer(b"".join(names) + b"\0", np.uint8).copy(), reg_cnt=cnt, regs=regs,
                              ann_off=None, ann_len=None, ann_name_off=None, ann_name_pool=None)
    s_regs, keep, _ = bpsw_hip._pairs_struct(g)
    s_reads, keep2, _ = bpsw_hip._pairs_struct(g, False)
    cap = 1024 * 2 * n
    buf = {0: np.zeros(cap, np.uint8), 1: np.zeros(cap, np.uint8)}
    off = np.zeros(2 * n + 1, np.int64)
    need = C.c_size_t(0)
    res = {"genome_bases": l_pac, "pairs": n, "read_len": a.read_len, "reps": a.reps, "regions_per_read": round(float(cnt.sum()) / (2 * n), 2),
           "pes": [list(p) for p in pes]}
    for mode, key in ((0, "text_on_host"), (bpsw_hip.SAM_TEXT_DEVICE, "text_on_device")):
        def call():
            rc = ctx.lib.bpsw_sam_pe_batch_ex(ctx.h, C.byref(opt), C.byref(topt), C.byref(s_regs), mode, bpsw_hip._ptr(buf[mode]), cap,
                                              bpsw_hip._ptr(off), C.byref(need), None)
            assert rc == 0, ctx.lib.bpsw_last_error()
            return lambda: (ctx.last_tail_host_ms(), ctx.last_tail_kernel()[0], bpsw_hip.last_sam_pe_times())
        wall, extra = timed_calls(a.reps, call)
        host = np.median(np.array([e[0] for e in extra]), axis=0)
        t = np.median(np.array([e[2] for e in extra]), axis=0)
        res[key] = {
            "sam_pe_batch_pairs_per_s": round(n / wall), "call_ms": round(1e3 * wall, 2), "text_bytes": int(need.value),
            "tail_host_ms": {"plan": round(float(host[0]), 2), "device_round_trip": round(float(host[1]), 2), "emit": round(float(host[2]), 2)},
            "reg2aln_kernel_ms": round(float(np.median([e[1] for e in extra])), 3),
        }
        if mode:
            res[key].update({"sam_len_kernel_ms": round(float(t[0]), 3), "sam_write_kernel_ms": round(float(t[1]), 3),
                             "line_table_ms": round(float(t[2]), 2), "text_round_trip_ms": round(float(t[3]), 2)})
    total = int(need.value)
    assert buf[0][:total].tobytes() == buf[1][:total].tobytes(), "the device text differs from the host text"
    res["lines"] = int(np.count_nonzero(buf[0][:total] == 10))
    out_pes = (bpsw_hip.PeStat * 4)()
    for mode, key in ((0, "text_on_host"), (bpsw_hip.SAM_TEXT_DEVICE, "text_on_device")):
        def call():
            rc = ctx.lib.bpsw_align_pe_batch(ctx.h, C.byref(opt), C.byref(so), C.byref(topt), C.byref(s_reads), None, bpsw_hip.ZDROP_BWA, 0,
                                             bpsw_hip.RESCUE_C, mode, bpsw_hip._ptr(buf[mode]), cap, bpsw_hip._ptr(off), C.byref(need), out_pes)
            assert rc == 0, ctx.lib.bpsw_last_error()
            return bpsw_hip.last_sam_pe_times
        wall, extra = timed_calls(a.reps, call)
        t = np.median(np.array(extra), axis=0)
        res["align_pe_batch_" + key] = {"pairs_per_s": round(n / wall), "call_ms": round(1e3 * wall, 2), "text_bytes": int(need.value),
                                        "stage_ms": {"worker1": round(float(t[4]), 2), "pe_stat": round(float(t[5]), 2),
                                                     "rescue": round(float(t[6]), 2), "sam_pe": round(float(t[7]), 2)}}
    total = int(need.value)
    assert buf[0][:total].tobytes() == buf[1][:total].tobytes(), "bpsw_align_pe_batch: the device text differs from the host text"
    ctx.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
