#!/usr/bin/env python3
"""Which DP rows a bench-shaped extension batch sweeps, by what the row loops of csrc/bpsw_extend_rows.h care about: CPU only.
The host build of the sift arithmetic (tests/sift_n_host: flanks with N included) says which sides the exact shortcuts resolve; every other side is swept
row by row here (the recurrences of SWUtil.scala:61-230 in the kernels' parallel form, checked against the oracle's result) and
every row is binned by: columns per lane the band needs (1: <= 63 columns, 2), phase of h1 (live / dead), band end at the query
end, zero cell in the band (the trimming's slow path), row improved the maximum, row at or past the query end (tail).
Usage: python tools/row_mix_census.py [config] [n_tasks]"""
import collections
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("cloud-scale-bwamem_amd", "oracle", "tests", ""):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np  # noqa: E402
import bench  # noqa: E402
import bpsw_hip  # noqa: E402
import ext_rows_model as erm  # noqa: E402
import pyoracle as po  # noqa: E402

cfg = int(sys.argv[1]) if len(sys.argv) > 1 else 3
n_want = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
W = bench.WORKLOADS[cfg]
soa = bench.make_ext_soa(W, cfg, 0, 0)
wire = bpsw_hip.wire_pack(soa)
orc = po.Oracle()
mat = po.default_mat().reshape(5, 5).astype(np.int64)

# the host sift
here = os.path.join(ROOT, "tests", "sift_n_host")
so = os.path.join(here, "_build", "libsift_n_host.so")
os.makedirs(os.path.dirname(so), exist_ok=True)
hdr = os.path.join(ROOT, "cloud-scale-bwamem_amd", "csrc")
subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + hdr, "-o", so, os.path.join(here, "sift_n_host.cpp")], check=True)
lib = C.CDLL(so)
n = soa.n
out = np.zeros(10 * n, np.int16); flag = np.zeros(n, np.uint8); kinds = np.zeros(2 * n, np.uint8)
w32 = np.ascontiguousarray(wire).view(np.uint32)
lib.sift_n_host_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_int] * 1 + [C.c_int] * 6 + [C.c_void_p] * 3
qmax = 127 if W["read_len"] <= 150 else 0   # the sift kernel is not launched for batches with longer flanks
rc = lib.sift_n_host_batch(w32.ctypes.data, w32.size, n, 100, 3, 1, 5, 2, qmax, out.ctypes.data, flag.ctypes.data, kinds.ctypes.data)   # default matrix: a 1, dm 5, dn 2
assert rc == 0
SIFT_FORM = 2  # bpsw_extend_sift_core.h: SIFT_UNSEEN 0, SIFT_FAIL 1, SIFT_FORM 2


def sweep(q, t, h0, w, stats, end_bonus):
    """one SWExtend call (tests/ext_rows_model.py: the row-by-row model the named case tables are held to); returns
    (max, qle, tle, gtle, gscore, max_off) and bins its rows"""
    sc = erm.Scoring(o_del=soa.o_del, e_del=soa.e_del, o_ins=soa.o_ins, e_ins=soa.e_ins, w=w)
    qlen, amax = len(q), 1
    max_ins = max(1, int((qlen * amax + end_bonus - sc.o_ins) / sc.e_ins + 1.0)); w = min(w, max_ins)
    max_del = max(1, int((qlen * amax + end_bonus - sc.o_del) / sc.e_del + 1.0)); w = min(w, max_del)
    return erm.sweep(q, t, h0, sc, w, tail_bound=True, stats=stats, span_hist=span_hist).res


stats = collections.Counter()
span_hist = collections.Counter()
sides_dp = sides_all = rows = 0
rng = np.random.default_rng(1)
pick = rng.permutation(n)[:n_want]
for tsk in pick:
    reg = int(soa.reg_score[tsk])
    h = int(soa.h0[tsk])
    for side in (0, 1):
        ql = int((soa.right_qlen if side else soa.left_qlen)[tsk]); rl = int((soa.right_rlen if side else soa.left_rlen)[tsk])
        if ql <= 0:
            continue
        qo = int((soa.right_q_off if side else soa.left_q_off)[tsk]); ro = int((soa.right_r_off if side else soa.left_r_off)[tsk])
        q = soa.pool[qo:qo + ql].astype(np.int64); t = soa.pool[ro:ro + rl].astype(np.int64)
        hinit = reg if side else h
        want, _ = orc.sw_extend(q.astype(np.uint8), t.astype(np.uint8), po.default_mat(), soa.o_del, soa.e_del, soa.o_ins, soa.e_ins, soa.w, 5, 100, hinit)
        sides_all += 1
        if kinds[2 * tsk + side] != SIFT_FORM:  # the DP (a side the sift did not examine -- four deficit columns or more -- may still be resolved by ext_kernel's own forms: slight overcount)
            st = collections.Counter()
            got = sweep(q, t, hinit, soa.w, st, 5)
            # (the tail-row bound ends the sweep early without changing the result)
            assert np.array_equal(got, want), (tsk, side, got, want)
            stats.update(st); sides_dp += 1; rows += sum(st.values())
        reg = int(want[0])
print(f"config {cfg}: {len(pick)} tasks, {sides_all} sides, {sides_dp} on the DP ({100 * sides_dp / sides_all:.1f} %), {rows} DP rows = {rows / max(sides_dp, 1):.1f} per DP side, {rows / len(pick):.1f} per task")
tot = sum(stats.values())
for k, v in stats.most_common(24):
    print(f"  {100 * v / tot:5.1f} %  {' '.join(k)}")
for dim, names in ((0, ("cols1", "cols2")), (1, ("live", "dead")), (2, ("atend", "inner")), (3, ("tail", "body")), (4, ("zero", "nozero")), (5, ("imp", "noimp"))):
    print("  ", {nm: round(100 * sum(v for k, v in stats.items() if k[dim] == nm) / tot, 1) for nm in names})

tot_s = sum(span_hist.values())
acc = 0
print("band width of the swept rows (columns, cumulative share): " + " ".join(f"<={8 * k + 7}:{(acc := acc + span_hist[k]) / tot_s:.3f}" for k in sorted(span_hist)))
