#!/usr/bin/env python3
"""bpsw_bam_sort over the BAM output of several bpsw_bam_pe_batch calls, on the synthetic FR pairs of tools/sam_pe_throughput.py: what
sorting and indexing on the device costs, phase by phase.

    python tools/bam_sort_rate.py [--genome-mb 8] [--calls 8] [--pairs 16384] [--read-len 150] [--sa-intv 32] [--reps 5]
                                  [--out profiles/bam_sort_rate.json]

The default input is eight calls of 16 384 pairs of 2 x 150 bp, concatenated, with the calls' starts as seg_off.  After one warm-up
call of each, four forms are called ALTERNATING --reps times: stored and BPSW_BAM_DEFLATE output, each with the eight segments and
with one (no seg_off: bam_walk_kernel is then one wavefront following every block_size of the stream).  The medians are reported as one
JSON line: the call's wall time, the eight times of bpsw_last_bam_sort_times, the bytes in and out, the records per second; beside them
the time of tests/bam_sort_host's serial path (a plain -O2 build: walk, keys, std::stable_sort, gather, BAI in stored blocks) over the
same records, for scale.  Before anything is timed the stored output is checked against the yardstick (tests/bam_sort_plain.py)."""
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
import bam_sort_plain as sp  # noqa: E402
import bpsw_hip  # noqa: E402
import fmi_util as fu  # noqa: E402
import seed_throughput as st  # noqa: E402
from sam_pe_throughput import make_pairs  # noqa: E402
from test_bam_sort_core_host import build_host, run_host  # noqa: E402

P = 65280
SLOTS = ["inflate_ms", "walk_ms", "keys_ms", "sort_ms", "gather_ms", "frame_or_deflate_ms", "table_and_bai_ms", "round_trip_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=8.0)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--pairs", type=int, default=16384)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--sa-intv", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_sort_rate.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(20261021)
    l_pac = int(a.genome_mb * 1e6) | 1
    fwd = rng.integers(0, 4, l_pac).astype(np.uint8)
    idx, _ = st.build_index(fwd, a.sa_intv)
    n = a.pairs
    ctx = bpsw_hip.Context(0)
    ctx.ref_load(fu.pack_pac(fwd), l_pac)
    ctx.bns_load(np.array([0], np.int64), np.array([l_pac], np.int32), ["chrSynthetic"])
    ctx.fmi_load(idx)
    opt, so, topt = bpsw_hip.default_opt(), bpsw_hip.default_seed_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    parts = []
    for call in range(a.calls):
        rb = make_pairs(fwd, n, a.read_len, rng)
        cnt, regs = ctx.worker1_batch(opt, so, rb, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=bpsw_hip.C2A_SORT_DEDUP)
        pes = bpsw_hip.pe_stat(opt, topt, l_pac, cnt, regs)
        names = [b"call%d.%07d" % (call, i) for i in range(n)]
        name_off = np.zeros(n + 1, np.int64)
        name_off[1:] = np.cumsum([len(s) for s in names])
        g = bpsw_hip.TailGroupSoA(group_size=n, l_pac=l_pac, id0=2 * n * call, pes=pes, read_len=rb.read_len, read_off=rb.read_off,
                                  read_pool=rb.read_pool, qual_pool=rng.integers(35, 74, rb.read_pool.size).astype(np.uint8), name_off=name_off,
                                  name_pool=np.frombuffer(b"".join(names) + b"\0", np.uint8).copy(), reg_cnt=cnt, regs=regs,
                                  ann_off=None, ann_len=None, ann_name_off=None, ann_name_pool=None)
        parts.append(ctx.bam_pe_batch(opt, topt, g)[0])
    body = b"".join(parts)
    starts = np.cumsum([0] + [len(x) for x in parts[:-1]]).astype(np.int64)
    header = ctx.bam_header(flags=bpsw_hip.HDR_COORDINATE)

    # what is timed is right: the stored form against the yardstick
    out, bai, n_rec = ctx.bam_sort(body, seg_off=starts, file_off=len(header))
    records = bp.split_records(bp.bgzf_inflate(body))
    srt = sp.sort_records(records, 1)
    assert n_rec == len(records) and bp.split_records(bp.bgzf_inflate(out)) == srt, "the sorted records differ from the yardstick's"
    assert bai == sp.build_bai(srt, sp.offsets_of(srt)[0], sp.member_offsets(out), P, len(header), 1), "the BAI differs from the yardstick's"

    forms = {"stored_8_segments": (0, starts), "stored_1_segment": (0, None), "deflate_8_segments": (bpsw_hip.BAM_DEFLATE, starts),
             "deflate_1_segment": (bpsw_hip.BAM_DEFLATE, None)}
    cap, bai_cap = len(out) + 64, len(bai) + 64
    buf, ibuf = np.zeros(cap, np.uint8), np.zeros(bai_cap, np.uint8)
    need, bneed, cnt_out = C.c_size_t(0), C.c_size_t(0), C.c_int64(0)
    rows, sizes = {f: [] for f in forms}, {}
    for k in range(a.reps + 1):   # (the first round warms every form up)
        for form, (flags, seg) in forms.items():
            w0 = time.perf_counter()
            rc = ctx.lib.bpsw_bam_sort(ctx.h, body, len(body), bpsw_hip._ptr(seg), 0 if seg is None else len(seg), 0, None, len(header), flags,
                                       bpsw_hip._ptr(buf), cap, C.byref(need), bpsw_hip._ptr(ibuf), bai_cap, C.byref(bneed), C.byref(cnt_out))
            wall = time.perf_counter() - w0
            assert rc == 0, ctx.lib.bpsw_last_error()
            sizes[form] = (int(need.value), int(bneed.value))
            if k:
                rows[form].append([1e3 * wall, *bpsw_hip.last_bam_sort_times()])
    ctx.close()

    exe = build_host(False)
    stream = b"".join(records)
    _, host_ms = run_host(exe, [([l_pac], len(header), P, [0, len(stream)], stream)], "rate")   # (one run: it is there for scale)
    res = {"genome_bases": l_pac, "calls": a.calls, "pairs_per_call": n, "read_len": a.read_len, "reps": a.reps, "records": len(records),
           "bytes_in": len(body), "record_stream_bytes": len(stream), "host_serial_ms": round(float(host_ms[0]), 2)}
    for form in forms:
        m = np.median(np.array(rows[form]), axis=0)
        d = {"call_ms": round(float(m[0]), 2), "bytes_out": sizes[form][0], "bai_bytes": sizes[form][1],
             "records_per_s": round(len(records) / (1e-3 * float(m[0]))), "call_ms_all": [round(r[0], 2) for r in rows[form]]}
        d.update({name: round(float(m[1 + i]), 3) for i, name in enumerate(SLOTS)})
        res[form] = d
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
