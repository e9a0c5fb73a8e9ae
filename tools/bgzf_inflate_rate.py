#!/usr/bin/env python3
"""What reading FASTQ as BGZF costs: bgzf_inflate_kernel over the blocks of paired reads, the BGZF-to-SAM call against the plain-text
call of the same build, and zlib's inflate of the same blocks on 16 threads.

    python tools/bgzf_inflate_rate.py [--genome-mb 8] [--pairs 16384] [--read-len 150] [--sa-intv 32] [--reps 5]
                                      [--out profiles/bgzf_inflate_rate.json]

The reads are the synthetic FR pairs of tools/sam_pe_throughput.py as two four-line FASTQ texts, bgzipped at level 6 with 65 280
bytes a block.  After one warm-up call of each, the calls are made ALTERNATING --reps times and the medians are reported as one JSON
line: bpsw_bgzf_inflate over both texts' blocks (the kernel's hipEvent time in ms, per block, and in GB/s of text; the call's wall
time), bpsw_align_fastq_bgzf_pe and bpsw_align_fastq_pe (wall time of the call), and zlib.decompress over the same blocks on a pool
of 16 threads.  Before anything is timed the device's bytes must be the text, and the two SAM texts must be equal."""
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
import inflate_cases as ic  # noqa: E402
import seed_throughput as st  # noqa: E402
from sam_pe_throughput import make_pairs  # noqa: E402


def fastq_texts(rb, n, rng):
    """the pairs of a read batch as two FASTQ texts"""
    letters = np.frombuffer(b"ACGTN", np.uint8)
    out = ([], [])
    for i in range(2 * n):
        o, l = int(rb.read_off[i]), int(rb.read_len[i])
        seq = letters[rb.read_pool[o: o + l]].tobytes()
        qual = rng.integers(35, 74, l).astype(np.uint8).tobytes()
        out[i & 1].append(b"@synthetic.%07d/%d\n" % (i >> 1, 1 + (i & 1)) + seq + b"\n+\n" + qual + b"\n")
    return b"".join(out[0]), b"".join(out[1])


def inflate1(cdata):
    return len(zlib.decompress(cdata, -15))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=8.0)
    ap.add_argument("--pairs", type=int, default=16384)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--sa-intv", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_inflate_rate.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(20261021)
    l_pac = int(a.genome_mb * 1e6) | 1
    fwd = rng.integers(0, 4, l_pac).astype(np.uint8)
    idx, _ = st.build_index(fwd, a.sa_intv)
    n = a.pairs
    rb = make_pairs(fwd, n, a.read_len, rng)
    t1, t2 = fastq_texts(rb, n, rng)
    z1, z2 = ic.bgzip(t1, level=6), ic.bgzip(t2, level=6)
    both, text = z1 + z2, t1 + t2
    members = bp.bgzf_members(both)
    ctx = bpsw_hip.Context(0)
    ctx.ref_load(fu.pack_pac(fwd), l_pac)
    ctx.bns_load(np.array([0], np.int64), np.array([l_pac], np.int32), ["chrSynthetic"])
    ctx.fmi_load(idx)
    opt, so, topt = bpsw_hip.default_opt(), bpsw_hip.default_seed_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    F = bpsw_hip.FASTQ_FINAL
    cap, mr = 1024 * 2 * n, 2 * n
    sam = {f: np.zeros(cap, np.uint8) for f in ("plain", "bgzf")}
    off, need, nr, consumed, pes = np.zeros(mr + 1, np.int64), C.c_size_t(0), C.c_int64(0), np.zeros(2, np.int64), (bpsw_hip.PeStat * 4)()
    out = np.zeros(len(text), np.uint8)
    nb, used, needed = C.c_int64(0), C.c_int64(0), C.c_size_t(0)
    lib, ptr = ctx.lib, bpsw_hip._ptr

    def call_inflate():
        return lib.bpsw_bgzf_inflate(ctx.h, both, len(both), bpsw_hip.BGZF_FINAL, ptr(out), out.size, C.byref(needed), C.byref(nb), C.byref(used))

    def call_plain():
        return lib.bpsw_align_fastq_pe(ctx.h, C.byref(opt), C.byref(so), C.byref(topt), t1, len(t1), t2, len(t2), F, 0, None, bpsw_hip.ZDROP_BWA, 0,
                                       bpsw_hip.RESCUE_C, 0, ptr(sam["plain"]), cap, ptr(off), mr, C.byref(need), pes, C.byref(nr), ptr(consumed))

    def call_bgzf():
        return lib.bpsw_align_fastq_bgzf_pe(ctx.h, C.byref(opt), C.byref(so), C.byref(topt), z1, len(z1), 0, z2, len(z2), 0, F, 0, None,
                                            bpsw_hip.ZDROP_BWA, 0, bpsw_hip.RESCUE_C, 0, ptr(sam["bgzf"]), cap, ptr(off), mr, C.byref(need), pes,
                                            C.byref(nr), ptr(consumed))
    calls = {"inflate": call_inflate, "plain": call_plain, "bgzf": call_bgzf}
    rows = {k: [] for k in calls}
    sizes = {}
    for k in range(a.reps + 1):   # (the first round warms every call up)
        for name, call in calls.items():
            w0 = time.perf_counter()
            rc = call()
            wall = 1e3 * (time.perf_counter() - w0)
            assert rc == 0, lib.bpsw_last_error()
            if name != "inflate":
                sizes[name] = int(need.value)
            if k:
                rows[name].append([wall, *(bpsw_hip.last_bgzf_times() if name == "inflate" else bpsw_hip.last_fastq_times())])
        if k == 0:   # what is timed is right
            assert out.tobytes() == text and nb.value == len(members), "the device's bytes are not the text"
            assert sizes["plain"] == sizes["bgzf"] and np.array_equal(sam["plain"][: sizes["plain"]], sam["bgzf"][: sizes["bgzf"]]), "the SAM texts differ"
            assert nr.value == 2 * n
    cdata = [m[2] for m in members]
    with ThreadPoolExecutor(16) as pool:
        list(pool.map(inflate1, cdata))
        zs = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            assert sum(pool.map(inflate1, cdata)) == len(text)
            zs.append(time.perf_counter() - t0)
    m = {k: np.median(np.array(v), axis=0) for k, v in rows.items()}
    kernel_ms = float(m["inflate"][2])
    res = {"genome_bases": l_pac, "pairs": n, "read_len": a.read_len, "reps": a.reps, "text_bytes": len(text), "bgzf_bytes": len(both),
           "blocks": len(members), "level": 6,
           "bgzf_inflate": {"kernel_ms": round(kernel_ms, 3), "kernel_ms_per_65280_byte_block": round(kernel_ms, 3),
                            "kernel_text_GB_per_s": round(len(text) / (1e-3 * kernel_ms) / 1e9, 3), "walk_ms": round(float(m["inflate"][1]), 3),
                            "round_trip_ms": round(float(m["inflate"][3]), 2), "call_ms": round(float(m["inflate"][0]), 2),
                            "kernel_ms_all": [round(r[2], 3) for r in rows["inflate"]]},
           "align_fastq_pe": {"call_ms": round(float(m["plain"][0]), 2), "parse_round_trip_ms": round(float(m["plain"][5]), 2),
                              "call_ms_all": [round(r[0], 2) for r in rows["plain"]]},
           "align_fastq_bgzf_pe": {"call_ms": round(float(m["bgzf"][0]), 2), "parse_round_trip_ms": round(float(m["bgzf"][5]), 2),
                                   "call_ms_all": [round(r[0], 2) for r in rows["bgzf"]]},
           "zlib_inflate_16_threads": {"ms": round(1e3 * float(np.median(zs)), 2), "text_GB_per_s": round(len(text) / float(np.median(zs)) / 1e9, 3)}}
    ctx.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
