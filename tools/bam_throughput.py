#!/usr/bin/env python3
"""The paired tail from region lists to BAM (bpsw_bam_pe_batch) beside the same tail to SAM text written on the device
(bpsw_sam_pe_batch_ex with BPSW_SAM_TEXT_DEVICE), of the same build, on the synthetic FR pairs of tools/sam_pe_throughput.py.

    python tools/bam_throughput.py [--genome-mb 8] [--pairs 100000] [--read-len 150] [--sa-intv 32] [--reps 5]
                                   [--out profiles/bam_throughput.json]

After one warm-up call of each, the two entries are called ALTERNATING --reps times; the medians are reported as one JSON line:
the call's wall time (a host clock around a call that ends in a stream synchronise), the calling thread's CPU time
(time.thread_time around the call), the bytes copied back, the three host stages of bpsw_last_tail_times, the reg2aln kernel, and
per form its own kernels (hipEvents on the launch stream), the line table and the round trip.  Run it several times for the spread.
Before anything is timed the BAM is decoded with tests/bam_plain.py: every member's CRC32 / ISIZE, and the first 4 000 records
against the specification applied to the SAM text."""
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

import bam_plain as bp  # noqa: E402
import bpsw_hip  # noqa: E402
import fmi_util as fu  # noqa: E402
import seed_throughput as st  # noqa: E402
from sam_pe_throughput import make_pairs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=8.0)
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--sa-intv", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_throughput.json"))
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
    cap = 1024 * 2 * n
    buf = {"sam": np.zeros(cap, np.uint8), "bam": np.zeros(cap, np.uint8)}
    off = np.zeros(2 * n + 1, np.int64)
    need = {"sam": C.c_size_t(0), "bam": C.c_size_t(0)}

    def call_sam():
        rc = ctx.lib.bpsw_sam_pe_batch_ex(ctx.h, C.byref(opt), C.byref(topt), C.byref(s_regs), bpsw_hip.SAM_TEXT_DEVICE, bpsw_hip._ptr(buf["sam"]), cap,
                                          bpsw_hip._ptr(off), C.byref(need["sam"]), None)
        assert rc == 0, ctx.lib.bpsw_last_error()
        return bpsw_hip.last_sam_pe_times()[:4]

    def call_bam():
        rc = ctx.lib.bpsw_bam_pe_batch(ctx.h, C.byref(opt), C.byref(topt), C.byref(s_regs), 0, bpsw_hip._ptr(buf["bam"]), cap, C.byref(need["bam"]), None)
        assert rc == 0, ctx.lib.bpsw_last_error()
        return bpsw_hip.last_bam_times()

    calls = {"sam": call_sam, "bam": call_bam}
    rows = {"sam": [], "bam": []}
    for k in range(a.reps + 1):   # (the first round warms both up)
        for form in ("bam", "sam"):
            w0, c0 = time.perf_counter(), time.thread_time()
            t = calls[form]()
            wall, cpu = time.perf_counter() - w0, time.thread_time() - c0
            if k:
                rows[form].append([1e3 * wall, 1e3 * cpu, ctx.last_tail_kernel()[0], *ctx.last_tail_host_ms(), *t])
        if k == 0:   # what is timed is right
            text = buf["sam"][: need["sam"].value].tobytes()
            bam = buf["bam"][: need["bam"].value].tobytes()
            stream = bp.bgzf_inflate(bam)
            lines = text.split(b"\n")[:4000]
            want = b"".join(bp.sam_to_bam(l, {b"chrSynthetic": 0}) for l in lines)
            assert stream[: len(want)] == want, "the BAM records differ from the specification applied to the SAM text"
            assert len(bam) == len(stream) + 31 * -(-len(stream) // 65280)
    res = {"genome_bases": l_pac, "pairs": n, "read_len": a.read_len, "reps": a.reps, "lines": int(text.count(b"\n")), "record_stream_bytes": len(stream)}
    for form, kernels in (("sam", ("sam_len_kernel_ms", "sam_write_kernel_ms")), ("bam", ("bam_len_kernel_ms", "bam_write_kernel_ms", "bgzf_frame_kernel_ms"))):
        m = np.median(np.array(rows[form]), axis=0)
        d = {"call_ms": round(float(m[0]), 2), "calling_thread_cpu_ms": round(float(m[1]), 2), "pairs_per_s": round(n / (1e-3 * float(m[0]))),
             "bytes_copied_back": int(need[form].value), "reg2aln_kernel_ms": round(float(m[2]), 3),
             "tail_host_ms": {"plan": round(float(m[3]), 2), "device_round_trip": round(float(m[4]), 2), "emit": round(float(m[5]), 2)}}
        for i, kname in enumerate(kernels):
            d[kname] = round(float(m[6 + i]), 3)
        d["line_table_ms"] = round(float(m[6 + len(kernels)]), 2)
        d["round_trip_ms"] = round(float(m[7 + len(kernels)]), 2)
        d["call_ms_all"] = [round(r[0], 2) for r in rows[form]]
        d["calling_thread_cpu_ms_all"] = [round(r[1], 2) for r in rows[form]]
        res[form] = d
    ctx.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
