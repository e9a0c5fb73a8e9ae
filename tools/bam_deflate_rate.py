#!/usr/bin/env python3
"""bpsw_bam_pe_batch with and without BPSW_BAM_DEFLATE, of the same build, on the synthetic FR pairs of tools/sam_pe_throughput.py:
what compressing the BGZF blocks on the device costs and saves.

    python tools/bam_deflate_rate.py [--genome-mb 8] [--pairs 16384] [--read-len 150] [--sa-intv 32] [--reps 5]
                                     [--out profiles/bam_deflate_rate.json]

The default batch is the 32 768 reads of a wire batch of bench.py's configs[2].  After one warm-up call of each, the two forms are
called ALTERNATING --reps times into a buffer that fits the stored form; the medians are reported as one JSON line: the call's wall
time, bpsw_last_bam_times, bpsw_last_bam_deflate_times, the bytes out per read, the deflate kernel's payload GB/s (stream bytes over
the kernel's hipEvent time), and beside it zlib level 1 over the same payloads on a pool of 16 threads (raw deflate, memLevel 9), in
GB/s and as a fraction of the stored size.  Before anything is timed both outputs are walked with tests/bam_plain.py (every member's
BSIZE, CRC32, ISIZE) and must inflate to the same stream."""
import argparse
import ctypes as C
import json
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cloud-scale-bwamem_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import bam_plain as bp  # noqa: E402
import bpsw_hip  # noqa: E402
import fmi_util as fu  # noqa: E402
import seed_throughput as st  # noqa: E402
from sam_pe_throughput import make_pairs  # noqa: E402

P = 65280


def zlib1(block):
    c = zlib.compressobj(1, zlib.DEFLATED, -15, 9)
    return len(c.compress(block) + c.flush())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=8.0)
    ap.add_argument("--pairs", type=int, default=16384)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--sa-intv", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_deflate_rate.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(20261021)
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
    forms = {"stored": 0, "deflate": bpsw_hip.BAM_DEFLATE}
    buf = {f: np.zeros(cap, np.uint8) for f in forms}
    need = {f: C.c_size_t(0) for f in forms}
    rows = {f: [] for f in forms}
    for k in range(a.reps + 1):   # (the first round warms both up)
        for form, flags in forms.items():
            w0 = time.perf_counter()
            rc = ctx.lib.bpsw_bam_pe_batch(ctx.h, C.byref(opt), C.byref(topt), C.byref(s_regs), flags, bpsw_hip._ptr(buf[form]), cap,
                                           C.byref(need[form]), None)
            wall = time.perf_counter() - w0
            assert rc == 0, ctx.lib.bpsw_last_error()
            if k:
                rows[form].append([1e3 * wall, *bpsw_hip.last_bam_times(), *bpsw_hip.last_bam_deflate_times()])
        if k == 0:   # what is timed is right
            out = {f: buf[f][: need[f].value].tobytes() for f in forms}
            members = bp.bgzf_members(out["deflate"])
            stream = b"".join(m[0] for m in members)
            assert stream == bp.bgzf_inflate(out["stored"]), "the two forms hold different records"
            assert len(out["stored"]) == len(stream) + 31 * -(-len(stream) // P)
            kinds, deflate_bytes = [m[2][0] & 7 for m in members], sum(len(m[2]) for m in members)
    blocks = [stream[at: at + P] for at in range(0, len(stream), P)]
    with ThreadPoolExecutor(16) as pool:
        list(pool.map(zlib1, blocks))
        t0 = time.perf_counter()
        z = list(pool.map(zlib1, blocks))
        z_s = time.perf_counter() - t0
    res = {"genome_bases": l_pac, "pairs": n, "read_len": a.read_len, "reps": a.reps, "record_stream_bytes": len(stream), "blocks": len(blocks),
           "blocks_kept_stored": kinds.count(1),
           "zlib_level1_16_threads": {"GB_per_s": round(len(stream) / z_s / 1e9, 3), "of_stored": round(sum(z) / len(stream), 4)}}
    for form in forms:
        m = np.median(np.array(rows[form]), axis=0)
        d = {"call_ms": round(float(m[0]), 2), "bytes_out": int(need[form].value), "bytes_out_per_read": round(need[form].value / (2 * n), 1),
             "bam_len_kernel_ms": round(float(m[1]), 3), "bam_write_kernel_ms": round(float(m[2]), 3), "bgzf_frame_kernel_ms": round(float(m[3]), 3),
             "line_table_ms": round(float(m[4]), 2), "round_trip_ms": round(float(m[5]), 2),
             "bgzf_deflate_kernel_ms": round(float(m[6]), 3), "bgzf_pack_kernel_ms": round(float(m[7]), 3), "size_table_ms": round(float(m[8]), 3),
             "packed_copy_ms": round(float(m[9]), 3), "call_ms_all": [round(r[0], 2) for r in rows[form]]}
        if form == "deflate":
            d["deflate_bytes_of_stored"] = round(deflate_bytes / len(stream), 4)
            d["deflate_kernel_payload_GB_per_s"] = round(len(stream) / (1e-3 * float(m[6])) / 1e9, 3)
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
