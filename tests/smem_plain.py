"""Test helper (numpy only): seeding without a BWT.  A plain restatement of what bpsw_seed_batch computes (csrc/bpsw_seed.hip:
bwt_smem1, mem_insert_seed's smem_next2 loop, bwt_sa) over the FULL suffix array of the doubled text plus sentinel
(fmi_util.suffix_array): no occurrence counts, no 128-base blocks, no `primary`, no sampling.  Every "extend" of the algorithm is
a bisection for the longer substring over the sorted suffixes, so nothing the kernels get wrong about the index's layout can be
wrong here in the same way.

The bi-interval of a substring p = q[b:e] is (x0, x1, x2): x0 the first row whose suffix starts with p, x1 the same for the reverse
complement of p, x2 the number of such rows (equal for both, the text being its own reverse complement).  Where p does not occur
both x0 and x1 are insertion points: the row at which p would be inserted.  The algorithm keeps such a zero-width interval only as
the start interval of a base that does not occur at all; its x0 is then L2[q[b]] + 1, which is that base's insertion point.

The control flow -- forward sweep, reversal, backward sweep, the condition on `mem`, re-seeding from the middle of the longest SMEM,
the ordered merge, the `sub` filter -- follows the algorithm as the kernel's comments describe it; tests/test_smem_plain.py pins
this module on recordings of the reference and, where it is built, on the live reference.  It is not the code under test."""
import bisect
import hashlib

import numpy as np

import fmi_util as fu
from bpsw_hip import fmi

_RC = bytes([3, 2, 1, 0, 4]) + bytes(range(5, 256))


class PlainIndex:
    def __init__(self, fwd: np.ndarray, sa_full: np.ndarray | None = None):
        self.fwd = np.asarray(fwd, np.uint8)
        self.l_pac = int(self.fwd.size)
        text = fu.doubled(self.fwd)
        self.seq_len = int(text.size)
        self.sa_full = fu.suffix_array(text) if sa_full is None else sa_full
        self.L2 = np.zeros(5, np.int64)
        self.L2[1:] = np.cumsum(np.bincount(text, minlength=4))
        self._text = text.tobytes()
        self._sa = [int(v) for v in self.sa_full]
        self._rows = range(self.seq_len + 1)
        self._memo = {}

    def _rows_of(self, p: bytes):
        """(first row whose suffix starts with p -- or where p would be inserted --, number of such rows).  A suffix cut off by the
        end of the text is a proper prefix of p at most, and sorts before it: the sentinel is the smallest symbol."""
        got = self._memo.get(p)
        if got is None:
            t, sa, m = self._text, self._sa, len(p)
            key = lambda r: t[sa[r]: sa[r] + m]  # noqa: E731
            lo = bisect.bisect_left(self._rows, p, key=key)
            got = self._memo[p] = (lo, bisect.bisect_right(self._rows, p, lo=lo, key=key) - lo)
        return got

    def interval(self, q: bytes, b: int, e: int):
        p = q[b:e]
        x0, n = self._rows_of(p)
        x1, n_rc = self._rows_of(p[::-1].translate(_RC))
        assert n == n_rc, (p, n, n_rc)
        if n == 0 and self.L2[q[b] + 1] == self.L2[q[b]]:
            assert x0 == self.L2[q[b]] + 1
        return x0, x1, n


def _smem1(ix: PlainIndex, q: bytes, x: int, min_intv: int):
    """the SMEMs through position x -> (list of (x0, x1, x2, qbeg, qend) by qbeg, where the next search starts)"""
    n = len(q)
    if q[x] > 3:
        return [], x + 1
    min_intv = max(min_intv, 1)
    ik, end = ix.interval(q, x, x + 1), x + 1
    curr = []
    i = x + 1
    while i < n:  # forward: the interval of q[x:i + 1]; remember an interval when the next base shrinks it
        if q[i] > 3:
            curr.append(ik + (end,))
            break
        ok = ix.interval(q, x, i + 1)
        if ok[2] != ik[2]:
            curr.append(ik + (end,))
            if ok[2] < min_intv:
                break
        ik, end = ok, i + 1
        i += 1
    if i == n:
        curr.append(ik + (end,))
    curr.reverse()  # longest first
    ret = curr[0][3]
    prev, mem = curr, []
    for i in range(x - 1, -2, -1):  # backward: every remembered end, extended to start at i
        usable = i >= 0 and q[i] < 4
        curr = []
        for p in prev:
            ok = ix.interval(q, i, p[3]) if usable else None
            if ok is None or ok[2] < min_intv:
                if not curr and (not mem or i + 1 < mem[-1][3]):  # no longer end survives and none was reported from this start
                    mem.append(p[:3] + (i + 1, p[3]))
            elif not curr or ok[2] != curr[-1][2]:
                curr.append(ok + (p[3],))
        if not curr:
            break
        prev = curr
    mem.reverse()
    return mem, ret


def split_len0(opt) -> int:
    return int(float(np.float32(opt["min_seed_len"]) * np.float32(opt["split_factor"])) + .499)


def intervals(ix: PlainIndex, opt: dict, read) -> np.ndarray:
    """every bi-interval in visiting order with the filter's verdict (fmi.SMEM_DTYPE)"""
    q = np.ascontiguousarray(read, np.uint8).tobytes()
    n = len(q)
    out = []
    if n < opt["min_seed_len"]:
        return np.zeros(0, fmi.SMEM_DTYPE)
    split_len = min(split_len0(opt), n)
    start_width = 2 if opt["no_exact"] else 1
    start = 0
    while True:
        while start < n and q[start] > 3:
            start += 1
        if start >= n:
            break
        ori_start = start
        mem, start = _smem1(ix, q, ori_start, start_width)
        if not mem:
            continue
        longest = max(mem, key=lambda p: p[4] - p[3])  # (max returns the first of equals)
        mx = longest[4] - longest[3]
        if split_len > 0 and mx >= split_len and longest[2] <= opt["split_width"]:
            sub, _ = _smem1(ix, q, (longest[3] + longest[4]) >> 1, longest[2] + 1)
            key = lambda p: p[3] << 32 | (n - p[4])  # noqa: E731
            i = j = 0
            while i < len(mem) and j < len(sub):
                if key(mem[i]) < key(sub[j]):
                    out.append(mem[i]); i += 1
                else:
                    if sub[j][4] - sub[j][3] >= mx >> 1 and sub[j][4] > ori_start:
                        out.append(sub[j])
                    j += 1
            out += mem[i:]
            out += [s for s in sub[j:] if s[4] - s[3] >= mx >> 1 and s[4] > ori_start]
        else:
            out += mem
    a = np.zeros(len(out), fmi.SMEM_DTYPE)
    for k, (x0, x1, x2, qb, qe) in enumerate(out):
        a[k] = (x0, x1, x2, qb, qe, int(not (qe - qb < opt["min_seed_len"] or x2 > opt["max_occ"])), 0)
    return a


def all_seeds(ix: PlainIndex, iv: np.ndarray) -> np.ndarray:
    """the occurrences of the kept intervals, row by row (fmi.SEED_DTYPE), bridging ones included"""
    kept = iv[iv["kept"] != 0]
    total = int(kept["x2"].sum())
    out = np.zeros(total, fmi.SEED_DTYPE)
    at = 0
    for p in kept:
        m = int(p["x2"])
        out["rbeg"][at: at + m] = ix.sa_full[int(p["x0"]): int(p["x0"]) + m]
        out["qbeg"][at: at + m] = p["qbeg"]
        out["len"][at: at + m] = p["qend"] - p["qbeg"]
        at += m
    return out


def seeds(ix: PlainIndex, iv: np.ndarray) -> np.ndarray:
    s = all_seeds(ix, iv)
    return s[~((s["rbeg"] < ix.l_pac) & (ix.l_pac < s["rbeg"] + s["len"]))]


def digest(records: np.ndarray) -> np.uint64:
    """the first 8 bytes of SHA-256 over the records' bytes"""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(records).tobytes()).digest()[:8], "<u8")[0]
