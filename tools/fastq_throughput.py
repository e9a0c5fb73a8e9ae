#!/usr/bin/env python3
"""What bpsw_fastq_parse costs the calling thread on the device path and under BPSW_FASTQ_HOST, and what the parse adds to the
fastq align entries, on synthetic 150-base reads written as four-line FASTQ, single-end and as pairs (two texts).

    python tools/fastq_throughput.py [--reads 100000] [--read-len 150] [--genome-mb 2] [--sa-intv 32] [--reps 5] [--rounds 3]
                                     [--no-align] [--out profiles/fastq_throughput.json]

Per round the two parse paths alternate (host, device), each with one warm-up call and the median of --reps calls: wall time and the
calling thread's CPU time (time.thread_time) of the C call alone, into arrays that fit; for the device path the five figures of
bpsw_last_fastq_times.  The outputs of the two paths are compared byte for byte.  Unless --no-align: the whole
bpsw_align_fastq_se / _pe call (parse on the device and on the host) against bpsw_align_se_batch / bpsw_align_pe_batch on pools parsed
beforehand, and the SAM texts compared.  One JSON line."""
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

F = bpsw_hip.FASTQ_FINAL
ARRAYS = ("read_len", "read_off", "read_pool", "qual_pool", "name_off", "name_pool")


def timed(reps, call):
    """one warm-up call, then `reps`: (median wall ms, median thread CPU ms, what call() returned last)"""
    wall, cpu, out = [], [], None
    for k in range(reps + 1):
        w0, c0 = time.perf_counter(), time.thread_time()
        out = call()
        w, c = time.perf_counter() - w0, time.thread_time() - c0
        if k:
            wall.append(1e3 * w)
            cpu.append(1e3 * c)
    return round(float(np.median(wall)), 3), round(float(np.median(cpu)), 3), out


def fastq_text(pool, quals, ln, reads, name_of):
    """reads (indices into the pool) as four-line FASTQ; name_of(k): read k's name"""
    letters = np.frombuffer(b"ACGTN", np.uint8)
    return b"".join(b"@%s\n%s\n+\n%s\n" % (name_of(k), letters[pool[k * ln:(k + 1) * ln]].tobytes(), quals[k * ln:(k + 1) * ln].tobytes()) for k in reads)


class Parser:
    """bpsw_fastq_parse into arrays allocated once: the C call alone is what is timed"""

    def __init__(self, ctx, t1, t2):
        self.ctx, self.t1, self.t2 = ctx, t1, t2
        size = len(t1) + len(t2 or b"")
        n = t1.count(b"\n") // 4 + (t2 or b"").count(b"\n") // 4
        self.a = dict(read_len=np.zeros(n + 1, np.int32), read_off=np.zeros(n + 1, np.int64), read_pool=np.zeros(size, np.uint8),
                      qual_pool=np.zeros(size, np.uint8), name_off=np.zeros(n + 2, np.int64), name_pool=np.zeros(size, np.uint8))
        self.n, self.consumed, self.needed = C.c_int64(0), np.zeros(2, np.int64), np.zeros(3, np.int64)
        self.max_reads, self.size = n, size

    def __call__(self, flags):
        p = bpsw_hip._ptr
        rc = self.ctx.lib.bpsw_fastq_parse(self.ctx.h, self.t1, len(self.t1), self.t2, len(self.t2 or b""), flags, self.max_reads, self.size, self.size,
                                           *(p(self.a[k]) for k in ARRAYS), C.byref(self.n), p(self.consumed), p(self.needed))
        assert rc == 0, self.ctx.lib.bpsw_last_error()
        n, pool, names = (int(x) for x in self.needed)
        pairs = self.t2 is not None
        return {"read_len": self.a["read_len"][:n].copy(), "read_off": self.a["read_off"][:n].copy(), "read_pool": self.a["read_pool"][:pool].copy(),
                "qual_pool": self.a["qual_pool"][:pool].copy(), "name_off": self.a["name_off"][: (n // 2 if pairs else n) + 1].copy(),
                "name_pool": self.a["name_pool"][:names].copy()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome-mb", type=float, default=2.0)
    ap.add_argument("--sa-intv", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-align", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastq_throughput.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(20261020)
    n, ln = a.reads & ~1, a.read_len
    l_pac = int(a.genome_mb * 1e6) | 1
    fwd = rng.integers(0, 4, l_pac).astype(np.uint8)
    rb = st.make_reads(fwd, n, ln, rng)
    quals = rng.integers(35, 74, rb.read_pool.size).astype(np.uint8)
    se_text = fastq_text(rb.read_pool, quals, ln, range(n), lambda k: b"synthetic.%07d" % k)
    pe_text = (fastq_text(rb.read_pool, quals, ln, range(0, n, 2), lambda k: b"synthetic.%07d/1" % (k // 2)),
               fastq_text(rb.read_pool, quals, ln, range(1, n, 2), lambda k: b"synthetic.%07d/2" % (k // 2)))
    ctx = bpsw_hip.Context(0)
    res = {"reads": n, "read_len": ln, "reps": a.reps, "rounds": a.rounds, "se_text_bytes": len(se_text), "pe_text_bytes": [len(t) for t in pe_text]}
    parsed = {}
    for key, t1, t2 in (("single_end", se_text, None), ("pairs", pe_text[0], pe_text[1])):
        parse = Parser(ctx, t1, t2)
        rounds = []
        for _ in range(a.rounds):
            r = {}
            for path, flag in (("host", bpsw_hip.FASTQ_HOST), ("device", 0)):
                wall, cpu, out = timed(a.reps, lambda: parse(F | flag))
                r[path] = {"wall_ms": wall, "thread_cpu_ms": cpu}
                if not flag:
                    t = bpsw_hip.last_fastq_times()
                    r[path]["kernels_ms"] = {"count": round(t[0], 3), "lines": round(t[1], 3), "record": round(t[2], 3), "emit": round(t[3], 3)}
                    r[path]["round_trip_ms"] = round(t[4], 3)
                parsed[(key, path)] = out
            rounds.append(r)
        for k in ARRAYS:
            assert np.array_equal(parsed[(key, "host")][k], parsed[(key, "device")][k]), (key, k)
        res[key] = {"rounds": rounds, "paths_equal": True}
    if not a.no_align:
        idx, _ = st.build_index(fwd, a.sa_intv)
        ctx.ref_load(fu.pack_pac(fwd), l_pac)
        ctx.bns_load(np.array([0], np.int64), np.array([l_pac], np.int32), ["chrSynthetic"])
        ctx.fmi_load(idx)
        opt, so, topt = bpsw_hip.default_opt(), bpsw_hip.default_seed_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
        cap = 1024 * n
        buf, off, need, got_n, consumed = np.zeros(cap, np.uint8), np.zeros(n + 1, np.int64), C.c_size_t(0), C.c_int64(0), np.zeros(2, np.int64)
        p = bpsw_hip._ptr
        d = parsed[("single_end", "host")]
        se = bpsw_hip.SeReadsSoA(read_len=d["read_len"], read_off=d["read_off"], read_pool=np.append(d["read_pool"], 0).astype(np.uint8),
                                 qual_pool=np.append(d["qual_pool"], 0).astype(np.uint8), name_off=d["name_off"],
                                 name_pool=np.append(d["name_pool"], 0).astype(np.uint8), id0=0, id_step=1)
        s_reads, keep, _ = bpsw_hip._se_struct(se, False)
        texts = {}

        def pools():
            rc = ctx.lib.bpsw_align_se_batch(ctx.h, C.byref(opt), C.byref(so), C.byref(topt), C.byref(s_reads), bpsw_hip.ZDROP_BWA, 0, 0, p(buf), cap,
                                             p(off), C.byref(need))
            assert rc == 0, ctx.lib.bpsw_last_error()
            return buf[: int(need.value)].tobytes()

        def from_text(flag):
            rc = ctx.lib.bpsw_align_fastq_se(ctx.h, C.byref(opt), C.byref(so), C.byref(topt), se_text, len(se_text), F | flag, 0, 1, bpsw_hip.ZDROP_BWA,
                                             0, 0, p(buf), cap, p(off), n, C.byref(need), C.byref(got_n), p(consumed))
            assert rc == 0 and got_n.value == n, ctx.lib.bpsw_last_error()
            return buf[: int(need.value)].tobytes()
        out = {}
        for name, call in (("align_se_batch_on_parsed_pools", pools), ("align_fastq_se_host_parse", lambda: from_text(bpsw_hip.FASTQ_HOST)),
                           ("align_fastq_se_device_parse", lambda: from_text(0))):
            wall, cpu, texts[name] = timed(a.reps, call)
            out[name] = {"wall_ms": wall, "thread_cpu_ms": cpu}
        assert len(set(texts.values())) == 1, "the SAM texts differ"
        res["align_single_end"] = out
        # pairs
        d = parsed[("pairs", "host")]
        st_pairs = bpsw_hip.Pairs()
        st_pairs.group_size, st_pairs.id0 = n // 2, 0
        keep_pe = [np.ascontiguousarray(d["read_len"]), np.ascontiguousarray(d["read_off"]), np.append(d["read_pool"], 0).astype(np.uint8),
                   np.append(d["qual_pool"], 0).astype(np.uint8), np.ascontiguousarray(d["name_off"]), np.append(d["name_pool"], 0).astype(np.uint8)]
        for field, arr in zip(("read_len", "read_off", "read_pool", "qual_pool", "name_off", "name_pool"), keep_pe):
            setattr(st_pairs, field, arr.ctypes.data)
        st_pairs.read_pool_bytes = int(d["read_pool"].size)
        pes = (bpsw_hip.PeStat * 4)()

        def pe_pools():
            rc = ctx.lib.bpsw_align_pe_batch(ctx.h, C.byref(opt), C.byref(so), C.byref(topt), C.byref(st_pairs), None, bpsw_hip.ZDROP_BWA, 0,
                                             bpsw_hip.RESCUE_C, 0, p(buf), cap, p(off), C.byref(need), pes)
            assert rc == 0, ctx.lib.bpsw_last_error()
            return buf[: int(need.value)].tobytes()

        def pe_from_text(flag):
            rc = ctx.lib.bpsw_align_fastq_pe(ctx.h, C.byref(opt), C.byref(so), C.byref(topt), pe_text[0], len(pe_text[0]), pe_text[1], len(pe_text[1]),
                                             F | flag, 0, None, bpsw_hip.ZDROP_BWA, 0, bpsw_hip.RESCUE_C, 0, p(buf), cap, p(off), n, C.byref(need), pes,
                                             C.byref(got_n), p(consumed))
            assert rc == 0 and got_n.value == n, ctx.lib.bpsw_last_error()
            return buf[: int(need.value)].tobytes()
        out, texts = {}, {}
        for name, call in (("align_pe_batch_on_parsed_pools", pe_pools), ("align_fastq_pe_host_parse", lambda: pe_from_text(bpsw_hip.FASTQ_HOST)),
                           ("align_fastq_pe_device_parse", lambda: pe_from_text(0))):
            wall, cpu, texts[name] = timed(a.reps, call)
            out[name] = {"wall_ms": wall, "thread_cpu_ms": cpu}
        assert len(set(texts.values())) == 1, "the paired SAM texts differ"
        res["align_pairs"] = out
    ctx.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
