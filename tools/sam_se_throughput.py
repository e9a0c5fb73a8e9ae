#!/usr/bin/env python3
"""Throughput of the single-end path from region lists to SAM text (bpsw_sam_se_batch) with the text written on the calling
thread and on the device (BPSW_SAM_TEXT_DEVICE), and the stage split of bpsw_align_se_batch (reads to text in one call), on
synthetic 150-base reads of a random genome.

    python tools/sam_se_throughput.py [--genome-mb 8] [--reads 100000] [--read-len 150] [--sa-intv 32] [--reps 5]
                                      [--out profiles/sam_se_throughput.json]

The regions are bpsw_worker1_batch's on the same reads (index built here as tools/seed_throughput.py builds it).  After one warm-up
call the median of --reps calls is reported, one JSON line: reads/s of bpsw_sam_se_batch both ways (the C call alone, into a buffer
that fits), the three host stages of bpsw_last_tail_times both ways, the two text kernels' times, the line table's and the text
round trip's, and bpsw_align_se_batch's worker1 / tail split both ways.  The two texts are compared byte for byte."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cloud-scale-bwamem_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import bpsw_hip  # noqa: E402
import fmi_util as fu  # noqa: E402
import seed_throughput as st  # noqa: E402


def timed_calls(reps, call):
    """one warm-up call, then `reps`: (median wall s, what `after()` returned for each timed call)"""
    wall, extra = [], []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        after = call()
        dt = time.perf_counter() - t0
        if k:
            wall.append(dt)
            extra.append(after())
    return float(np.median(wall)), extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=8.0)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--sa-intv", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_se_throughput.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(20261018)
    l_pac = int(a.genome_mb * 1e6) | 1
    fwd = rng.integers(0, 4, l_pac).astype(np.uint8)
    idx, _ = st.build_index(fwd, a.sa_intv)
    rb = st.make_reads(fwd, a.reads, a.read_len, rng)
    n = a.reads
    ctx = bpsw_hip.Context(0)
    ctx.ref_load(fu.pack_pac(fwd), l_pac)
    ctx.bns_load(np.array([0], np.int64), np.array([l_pac], np.int32), ["chrSynthetic"])
    ctx.fmi_load(idx)
    opt, so, topt = bpsw_hip.default_opt(), bpsw_hip.default_seed_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    cnt, regs = ctx.worker1_batch(opt, so, rb, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=bpsw_hip.C2A_SORT_DEDUP)
    names = [b"synthetic.%07d" % i for i in range(n)]
    name_off = np.zeros(n + 1, np.int64)
    name_off[1:] = np.cumsum([len(s) for s in names])
    se = bpsw_hip.SeReadsSoA(read_len=rb.read_len, read_off=rb.read_off, read_pool=rb.read_pool,
                             qual_pool=rng.integers(35, 74, rb.read_pool.size).astype(np.uint8), name_off=name_off,
                             name_pool=np.frombuffer(b"".join(names) + b"\0", np.uint8).copy(), reg_cnt=cnt, regs=regs, id0=0, id_step=1)
    s_regs, keep, _ = bpsw_hip._se_struct(se, True)
    s_reads, keep2, _ = bpsw_hip._se_struct(se, False)
    cap = 1024 * n
    buf = {0: np.zeros(cap, np.uint8), 1: np.zeros(cap, np.uint8)}
    off = np.zeros(n + 1, np.int64)
    need = C.c_size_t(0)
    res = {"genome_bases": l_pac, "reads": n, "read_len": a.read_len, "reps": a.reps, "regions_per_read": round(float(cnt.sum()) / n, 2)}
    for mode, key in ((0, "text_on_host"), (bpsw_hip.SAM_TEXT_DEVICE, "text_on_device")):
        def call():
            rc = ctx.lib.bpsw_sam_se_batch(ctx.h, C.byref(opt), C.byref(topt), C.byref(s_regs), mode, bpsw_hip._ptr(buf[mode]), cap,
                                           bpsw_hip._ptr(off), C.byref(need), None)
            assert rc == 0, ctx.lib.bpsw_last_error()
            return lambda: (ctx.last_tail_host_ms(), ctx.last_tail_kernel()[0], bpsw_hip.last_sam_se_times())
        wall, extra = timed_calls(a.reps, call)
        host = np.median(np.array([e[0] for e in extra]), axis=0)
        t = np.median(np.array([e[2] for e in extra]), axis=0)
        res[key] = {
            "sam_se_batch_reads_per_s": round(n / wall), "call_ms": round(1e3 * wall, 2), "text_bytes": int(need.value),
            "tail_host_ms": {"plan": round(float(host[0]), 2), "device_round_trip": round(float(host[1]), 2), "emit": round(float(host[2]), 2)},
            "reg2aln_kernel_ms": round(float(np.median([e[1] for e in extra])), 3),
        }
        if mode:
            res[key].update({"sam_len_kernel_ms": round(float(t[0]), 3), "sam_write_kernel_ms": round(float(t[1]), 3),
                             "line_table_ms": round(float(t[2]), 2), "text_round_trip_ms": round(float(t[3]), 2)})
    total = int(need.value)
    assert buf[0][:total].tobytes() == buf[1][:total].tobytes(), "the device text differs from the host text"
    res["lines"] = int(np.count_nonzero(buf[0][:total] == 10))
    for mode, key in ((0, "text_on_host"), (bpsw_hip.SAM_TEXT_DEVICE, "text_on_device")):
        def call():
            rc = ctx.lib.bpsw_align_se_batch(ctx.h, C.byref(opt), C.byref(so), C.byref(topt), C.byref(s_reads), bpsw_hip.ZDROP_BWA, 0, mode,
                                             bpsw_hip._ptr(buf[mode]), cap, bpsw_hip._ptr(off), C.byref(need))
            assert rc == 0, ctx.lib.bpsw_last_error()
            return bpsw_hip.last_sam_se_times
        wall, extra = timed_calls(a.reps, call)
        t = np.median(np.array(extra), axis=0)
        res["align_se_batch_" + key] = {"reads_per_s": round(n / wall), "call_ms": round(1e3 * wall, 2),
                                        "stage_ms": {"worker1": round(float(t[4]), 2), "sam_se": round(float(t[5]), 2)}}
    assert buf[0][:total].tobytes() == buf[1][:total].tobytes(), "bpsw_align_se_batch: the device text differs from the host text"
    ctx.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
