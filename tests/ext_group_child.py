"""The child process of tests/test_ext_group_gpu.py (the switches it needs -- BPSW_STREAM_POOL=1, BPSW_EXT_SIFT_MIN=64, BPSW_EXT_RING=0,
BPSW_EXT_INJECT_DEFER -- are read once per process): extension calls queued behind the device's ONE pooled stream must ride one launch
chain (csrc/bpsw_ext_group.h) and return, each, exactly what pyoracle.Oracle().wire_extend computes for its batch.

How a group is MADE: six helper threads keep the stream busy with 32 768-task batches through the classify entry (calls that run
alone and queue like everybody else), k member threads with contexts of their own submit, and the main thread watches the library's gauge
(bpsw_ext_group_waiting).  A round in which it read k had all k members in the queue at one moment, so bpsw_ext_group_counts must show
them as one group (nine: one of eight and one of one).  A round in which a member slipped through before the others had arrived proves
nothing about grouping (its results are checked all the same) and is played again, a few times at most.

  python ext_group_child.py <scenario>      prints "EXTGROUP ok ..." and exits 0, or raises"""
import ctypes as C
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cloud-scale-bwamem_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import bpsw_hip  # noqa: E402
from bpsw_hip import synth  # noqa: E402
import pyoracle as po  # noqa: E402

orc = po.Oracle()
INJECT = int(os.environ.get("BPSW_EXT_INJECT_DEFER", "0") or 0)
SIFT_MIN = int(os.environ.get("BPSW_EXT_SIFT_MIN", "8192") or 8192)


HELPER_CTX = []  # the helper threads' contexts, made once


class Member:
    """a context of its own, a batch and the oracle's answer for it (computed once); how = batch | view | classify | coords | bad"""

    def __init__(self, wire, how="batch", mat=None, want=None, grouped=True):
        self.ctx = bpsw_hip.Context(0)
        self.wire, self.how, self.mat, self.grouped = np.ascontiguousarray(wire, np.uint8), how, mat, grouped
        if mat is not None:
            self.ctx.set_ext_scoring(mat, 100, bpsw_hip.ZDROP_SCALA)
        self.n = int(np.frombuffer(self.wire[8:12].tobytes(), "<i4")[0])
        if how == "bad":
            self.want = None
        elif want is not None:
            self.want = want
        else:
            self.want = orc.wire_extend(self.wire, po.default_mat() if mat is None else mat, 100, po.ZDROP_SCALA)[0]
        self.err = None
        self.relaunches = 0

    def prepare(self):
        self.before = self.ctx.stats().ext_full_relaunches

    def call(self):
        try:
            before = self.before
            if self.how == "view":
                got = self._view()
            elif self.how == "classify":
                got = self.ctx.extend_batch_classify(self.wire)[0]
            elif self.how == "bad":
                try:
                    self.ctx.extend_batch(self.wire)
                    self.err = "a malformed batch was accepted"
                except bpsw_hip.BpswError:
                    pass
                return
            else:
                got = self.ctx.extend_batch(self.wire)
            self.relaunches = self.ctx.stats().ext_full_relaunches - before
            if not np.array_equal(got, self.want):
                bad = np.nonzero((np.asarray(got).reshape(-1, 10) != self.want.reshape(-1, 10)).any(axis=1))[0]
                self.err = f"{bad.size}/{self.n} tasks differ from the oracle ({self.how}), first {bad[:5]}"
        except BaseException as e:  # noqa: BLE001
            self.err = repr(e)

    def _view(self):
        """bpsw_extend_stage / bpsw_extend_commit, as the JNI shim calls: the results are read where the kernel wrote them"""
        lib, h = self.ctx.lib, self.ctx.h
        lib.bpsw_extend_stage.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        lib.bpsw_extend_commit.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        buf = C.c_void_p()
        assert lib.bpsw_extend_stage(h, self.wire.size, C.byref(buf)) == 0
        C.memmove(buf, self.wire.ctypes.data, self.wire.size)
        out, n_out = C.c_void_p(), C.c_size_t()
        rc = lib.bpsw_extend_commit(h, self.wire.size, C.byref(out), C.byref(n_out))
        assert rc == 0, lib.bpsw_last_error()
        return np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_int16)), shape=(n_out.value,)).copy()


def play(members, probe, busy_wire, attempts=6):
    """the members' calls behind a busy stream; returns (observed, groups, summed, largest): the counts' change over the round in which
    the gauge read the number of grouped-plan members (observed), else over the last round"""
    k = sum(1 for m in members if m.grouped)
    for attempt in range(attempts):
        stop, go = threading.Event(), threading.Event()
        errs = []

        warm = []

        def keep_busy(cc):
            try:
                while not stop.is_set():
                    cc.extend_batch_classify(busy_wire)
                    warm.append(1)
            except BaseException as e:  # noqa: BLE001
                errs.append(repr(e))

        def member(m):
            m.prepare()
            go.wait()
            m.call()

        # (six: the queue is first in, first out, so a member that arrives has the calls of most of them in front of it -- several
        # milliseconds in which the other members arrive)
        while len(HELPER_CTX) < 6:
            HELPER_CTX.append(bpsw_hip.Context(0))
        helpers = [threading.Thread(target=keep_busy, args=(cc,)) for cc in HELPER_CTX]
        threads = [threading.Thread(target=member, args=(m,)) for m in members]
        for t in helpers + threads:
            t.start()
        # (the helpers' first calls allocate their arenas: the round begins when a few calls are behind them and both are in their loops)
        t_end = time.time() + 120
        while len(warm) < 18 and not errs and time.time() < t_end:
            time.sleep(0.001)
        c0 = probe.ext_group_counts()
        go.set()
        observed = False
        while any(t.is_alive() for t in threads) and time.time() < t_end:
            if probe.ext_group_waiting() == k and k > 0:
                observed = True
                break
            time.sleep(0.0001)  # (the members' threads need the interpreter to get into their calls)
        for t in threads:
            t.join(120)
        stop.set()
        for t in helpers:
            t.join(120)
        assert not errs, errs[:2]
        for m in members:
            assert m.err is None, m.err
        c1 = probe.ext_group_counts()
        if observed or k == 0:
            break
    return observed, c1[0] - c0[0], c1[1] - c0[1], c1[2]


def default_wire(n_reads, seed, **kw):
    return bpsw_hip.wire_pack(synth.ext_tasks(n_reads, read_len=150, seed=seed, **kw))


def subset_wire(soa, n):
    return bpsw_hip.wire_pack(soa.subset(np.arange(n)))


def perfect_wire(n, seed):
    """n tasks whose flanks match their targets base for base (the target runs on for a few bases): the sift resolves both sides of each"""
    rng = np.random.default_rng(seed)
    pool, f = [], {k: [] for k in ("left_qlen", "left_rlen", "right_qlen", "right_rlen", "left_q_off", "left_r_off", "right_q_off",
                                     "right_r_off", "reg_score", "q_beg", "h0", "idx")}
    for i in range(n):
        lq, rq = (list(rng.integers(0, 4, int(rng.integers(20, 100)))) for _ in range(2))
        for name, seq in (("left_q", lq), ("left_r", lq + list(rng.integers(0, 4, 12))), ("right_q", rq), ("right_r", rq + list(rng.integers(0, 4, 12)))):
            f[name + "_off"].append(len(pool))
            f[name.replace("_q", "_qlen").replace("_r", "_rlen")].append(len(seq))
            pool.extend(int(c) for c in seq)
        f["reg_score"].append(30); f["h0"].append(30); f["q_beg"].append(len(lq)); f["idx"].append(i)
    kw = {k: np.array(v, np.int64 if k.endswith("_off") else np.int32) for k, v in f.items()}
    return bpsw_hip.wire_pack(bpsw_hip.ExtTaskSoA(pool=np.array(pool + [0], np.uint8), **kw))


def main(scenario):
    probe = bpsw_hip.Context(0)
    busy_wire = default_wire(36000, 901)
    assert int(np.frombuffer(busy_wire[8:12].tobytes(), "<i4")[0]) >= 32768
    soa = synth.ext_tasks(1200, read_len=150, seed=902)
    assert soa.n >= 1000
    if scenario == "sizes":
        # k = 1, 2, 8, 9 members of 200 tasks; nine are one group of eight and one of one
        wire = subset_wire(soa, 200)
        want = orc.wire_extend(wire)[0]
        pool = [Member(wire, want=want) for _ in range(9)]
        largest_so_far = 0
        for k in (1, 2, 8, 9):
            obs, groups, summed, largest = play(pool[:k], probe, busy_wire)
            assert obs, f"the gauge never read {k}"
            largest_so_far = max(largest_so_far, min(k, 8))
            assert (groups, summed, largest) == (1 if k <= 8 else 2, k, largest_so_far), (k, groups, summed, largest)
            if INJECT:
                assert all(m.relaunches == 1 for m in pool[:k]), [m.relaunches for m in pool[:k]]
        for m in pool:
            m.ctx.close()
    elif scenario == "mixed":
        # members of 1 (with BPSW_EXT_SIFT_MIN=64 below the sift threshold: alone; with 1 in the group), 64, 65, 200 and 1 000 tasks; other gap costs and another matrix; one read through the
        # view; one every task of which the sift finishes (error-free 100 bp reads: no ticket, its slice still resets its queue and posts a
        # zero); a coordinate batch, a classify call, a 300-base flank and a malformed batch among them: those run alone
        mat2 = po.default_mat().copy().reshape(5, 5)
        for i in range(4):
            for j in range(4):
                mat2[i, j] = 1 if i == j else -3
        mat2 = mat2.reshape(-1)
        w_gap = subset_wire(soa, 300).copy()
        w_gap[0:4] = [5, 2, 4, 2]  # oDel, eDel, oIns, eIns of the batch's header
        perfect = perfect_wire(300, 903)
        long_flank = bpsw_hip.wire_pack(synth.ext_tasks(150, read_len=400, seed=904))
        l_pac = 60_013
        pac, bases = synth.random_pac(l_pac, seed=905)
        chains = synth.read_chains(120, bases, l_pac, read_len=150, seed=906)
        co, by = synth.coord_ext_tasks(chains, bases, seed=907)
        probe.ref_load(pac, l_pac)
        bad = subset_wire(soa, 100).copy()
        bad[32:34] = [0xff, 0xff]  # a negative left query length in the first record
        members = [Member(subset_wire(soa, 64)), Member(subset_wire(soa, 65)), Member(subset_wire(soa, 200)), Member(subset_wire(soa, 1000)),
                   Member(w_gap, mat=mat2), Member(subset_wire(soa, 333), how="view"), Member(perfect),
                   Member(subset_wire(soa, 1), grouped=SIFT_MIN <= 1), Member(bpsw_hip.wire_coords_pack(co), how="coords", want=orc.wire_extend(bpsw_hip.wire_pack(by))[0], grouped=False),
                   Member(subset_wire(soa, 150), how="classify", grouped=False), Member(long_flank, grouped=False), Member(bad, how="bad", grouped=False)]
        k = sum(1 for m in members if m.grouped)
        assert k == (8 if SIFT_MIN <= 1 else 7)
        # three consecutive groups of the same contexts, in another order each: a stale queue word of one round would spoil the next
        seen = 0
        for order in (list(range(12)), list(reversed(range(12))), [3, 8, 0, 9, 6, 11, 1, 10, 5, 2, 7, 4]):
            obs, groups, summed, largest = play([members[i] for i in order], probe, busy_wire)
            if obs:
                seen += 1
                assert (groups, summed) == (1, k), (groups, summed, largest)
            if INJECT:
                # (a task the sift finishes never reaches the short kernel, so the hook cannot defer it: the member the sift finishes
                # whole makes no late launch, and the 1-task member only if its one task needs a sweep)
                assert all(m.relaunches == (0 if m is members[6] else 1) for m in members if m.grouped and m is not members[7]), [m.relaunches for m in members]
                assert members[7].relaunches <= 1
        assert seen >= 1, "no round had all grouped-plan members waiting at once"
        for m in members:
            m.ctx.close()
    elif scenario == "off":
        # BPSW_EXT_GROUP_MAX=1: nobody is grouped, whatever waits
        wire = subset_wire(soa, 200)
        want = orc.wire_extend(wire)[0]
        pool = [Member(wire, want=want) for _ in range(4)]
        play(pool, probe, busy_wire, attempts=1)
        assert probe.ext_group_counts()[2] <= 1
        for m in pool:
            m.ctx.close()
    else:
        raise SystemExit("unknown scenario")
    assert probe.ext_group_waiting() == 0
    for cc in HELPER_CTX:
        cc.close()
    probe.close()
    print("EXTGROUP ok", scenario)


if __name__ == "__main__":
    main(sys.argv[1])
