"""Test helper (numpy only): the FM-index of a small genome, built the way `bwa index` would -- doubled sequence (forward +
reverse complement), suffix array with sentinel, BWT with the sentinel removed and `primary` recorded, L2, the interleaved
128-base blocks of bwt_bwtupdate_core, the suffix array sampled every sa_intv rows -- plus ctypes mirrors of the reference's
bwt_t / mem_opt_t and thin callers of its seeding functions (oracle/_ref/libbwaref.so), so that the reference itself can be run
on such an index.  tests/test_fmi_builder.py pins this builder on the reference; it is not the code under test."""
import ctypes as C
import os

import numpy as np

from bpsw_hip import fmi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seed_chain_small.npz")


def doubled(fwd: np.ndarray) -> np.ndarray:
    fwd = np.asarray(fwd, np.uint8)
    return np.concatenate([fwd, (3 - fwd[::-1]).astype(np.uint8)])


def pack_pac(fwd: np.ndarray) -> np.ndarray:
    """the 2-bit .pac: base k = pac[k >> 2] >> ((~k & 3) << 1) & 3"""
    n = int(fwd.shape[0])
    b = np.zeros((n + 3) // 4 * 4, np.uint8)
    b[:n] = fwd
    b = b.reshape(-1, 4)
    return (b[:, 0] << 6 | b[:, 1] << 4 | b[:, 2] << 2 | b[:, 3]).astype(np.uint8)


def unpack_pac(pac: np.ndarray, l_pac: int) -> np.ndarray:
    k = np.arange(l_pac)
    return (pac[k >> 2] >> ((~k & 3) << 1) & 3).astype(np.uint8)


def suffix_array(text: np.ndarray) -> np.ndarray:
    """suffix array of text + sentinel (the sentinel sorts first) by prefix doubling; length len(text) + 1"""
    n = int(text.shape[0]) + 1
    rank = np.concatenate([text.astype(np.int64) + 1, [0]])
    k = 1
    while True:
        second = np.zeros(n, np.int64)
        second[: n - k] = rank[k:] + 1
        order = np.lexsort((second, rank))
        key = rank[order] * (n + 2) + second[order]
        new = np.zeros(n, np.int64)
        new[order] = np.concatenate([[0], np.cumsum(key[1:] != key[:-1])])
        rank = new
        if int(rank.max()) == n - 1:
            return order.astype(np.int64)
        k <<= 1


def build_index(fwd: np.ndarray, sa_intv: int, sa_full: np.ndarray | None = None):
    """-> (fmi.FmIndex, full suffix array)"""
    text = doubled(fwd)
    seq_len = int(text.shape[0])
    sa = suffix_array(text) if sa_full is None else sa_full
    primary = int(np.nonzero(sa == 0)[0][0])
    rows = sa[sa != 0]
    bwt = text[rows - 1]                       # the sentinel's row removed: seq_len bases
    L2 = np.zeros(5, np.int64)
    L2[1:] = np.cumsum(np.bincount(text, minlength=4))
    # the interleaved array: per 128 bases four 64-bit counts of what came before, then the bases 16 to a word, first base in
    # the top bits; one more set of counts after the last base word
    n_words = (seq_len + 15) // 16
    padded = np.zeros(n_words * 16, np.uint32)
    padded[:seq_len] = bwt
    words = np.zeros(n_words, np.uint32)
    for j in range(16):
        words |= padded[j::16] << np.uint32(30 - 2 * j)
    onehot = np.zeros((seq_len + 1, 4), np.int64)
    onehot[1:][np.arange(seq_len), bwt] = 1
    cum = np.cumsum(onehot, axis=0)            # cum[i] = counts in bwt[:i]
    out = []
    for i in range(0, seq_len, 128):
        out.append(cum[i].astype("<u8").view("<u4"))
        out.append(words[i // 16: min(i // 16 + 8, n_words)])
    out.append(cum[seq_len].astype("<u8").view("<u4"))
    arr = np.ascontiguousarray(np.concatenate(out), np.uint32)
    assert arr.size == (seq_len + 15) // 16 + ((seq_len + 127) // 128 + 1) * 8
    samp = sa[::sa_intv].astype(np.int64).copy()
    samp[0] = -1
    assert samp.size == (seq_len + sa_intv) // sa_intv
    return fmi.FmIndex(primary=primary, L2=L2, seq_len=seq_len, bwt=arr, sa_intv=sa_intv, sa=samp), sa


# ---- the reference's records ---------------------------------------------------------------------------------------------
class BwtT(C.Structure):  # bwt_t, native/bwt.h:46-58
    _fields_ = [("primary", C.c_uint64), ("L2", C.c_uint64 * 5), ("seq_len", C.c_uint64), ("bwt_size", C.c_uint64),
                ("bwt", C.c_void_p), ("cnt_table", C.c_uint32 * 256), ("sa_intv", C.c_int), ("n_sa", C.c_uint64), ("sa", C.c_void_p)]


class BwtIntv(C.Structure):  # bwtintv_t
    _fields_ = [("x", C.c_uint64 * 3), ("info", C.c_uint64)]


class BwtIntvV(C.Structure):
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.POINTER(BwtIntv))]


class MemOptT(C.Structure):  # mem_opt_t, native/bwamem.h:21-47
    _fields_ = [(n, C.c_int) for n in ("a", "b", "o_del", "e_del", "o_ins", "e_ins", "pen_unpaired", "pen_clip5", "pen_clip3", "w", "zdrop",
                                        "T", "flag", "min_seed_len")] + \
               [("split_factor", C.c_float), ("split_width", C.c_int), ("max_occ", C.c_int), ("max_chain_gap", C.c_int),
                ("n_threads", C.c_int), ("chunk_size", C.c_int), ("mask_level", C.c_float), ("chain_drop_ratio", C.c_float),
                ("mask_level_redun", C.c_float), ("mapQ_coef_len", C.c_float), ("mapQ_coef_fac", C.c_int), ("max_ins", C.c_int),
                ("max_matesw", C.c_int), ("mat", C.c_int8 * 25)]


class MemSeedT(C.Structure):
    _fields_ = [("rbeg", C.c_int64), ("qbeg", C.c_int32), ("len", C.c_int32)]


class MemChainT(C.Structure):
    _fields_ = [("n", C.c_int), ("m", C.c_int), ("pos", C.c_int64), ("seeds", C.POINTER(MemSeedT))]


class MemChainV(C.Structure):
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.POINTER(MemChainT))]


MEM_F_NO_EXACT = 0x40
SEED_OPT_FIELDS = ("min_seed_len", "max_occ", "split_width", "max_chain_gap", "no_exact", "split_factor", "chain_drop_ratio", "mask_level")


def ref_bwt(idx) -> BwtT:
    """a bwt_t over the arrays of an fmi.FmIndex (which must outlive it)"""
    b = BwtT()
    b.primary = idx.primary
    for i in range(5):
        b.L2[i] = int(idx.L2[i])
    b.seq_len, b.bwt_size, b.bwt = idx.seq_len, idx.bwt.size, idx.bwt.ctypes.data
    for i in range(256):  # bwt_gen_cnt_table
        x = 0
        for j in range(4):
            x |= (((i & 3) == j) + ((i >> 2 & 3) == j) + ((i >> 4 & 3) == j) + ((i >> 6) == j)) << (j << 3)
        b.cnt_table[i] = x
    b.sa_intv, b.n_sa = idx.sa_intv, idx.sa.size
    b._sa_u64 = np.ascontiguousarray(idx.sa).view(np.uint64)
    b.sa = b._sa_u64.ctypes.data
    return b


class RefSeeding:
    """mem_chain's pieces of the reference, called one by one so that every intermediate list can be recorded"""

    def __init__(self, path):
        lib = C.CDLL(path)
        lib.mem_opt_init.restype = C.POINTER(MemOptT)
        lib.smem_itr_init.restype = C.c_void_p
        lib.smem_itr_init.argtypes = [C.c_void_p]
        lib.smem_itr_destroy.argtypes = [C.c_void_p]
        lib.smem_set_query.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.smem_next2.restype = C.POINTER(BwtIntvV)
        lib.smem_next2.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        lib.bwt_sa.restype = C.c_uint64
        lib.bwt_sa.argtypes = [C.c_void_p, C.c_uint64]
        lib.bwt_match_exact.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.mem_chain.restype = MemChainV
        lib.mem_chain.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
        lib.mem_chain_flt.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        self.lib = lib
        self.libc = C.CDLL(None)
        self.libc.free.argtypes = [C.c_void_p]

    def opt(self, sopt=None, w=None):
        """mem_opt_init with the seeding fields of a bpsw seed-option record (or dict) written over it; free with libc.free"""
        o = self.lib.mem_opt_init()
        if sopt is not None:
            get = (lambda k: sopt[k]) if isinstance(sopt, dict) else (lambda k: getattr(sopt, k))
            for k in SEED_OPT_FIELDS:
                if k == "no_exact":
                    o.contents.flag = (o.contents.flag & ~MEM_F_NO_EXACT) | (MEM_F_NO_EXACT if get(k) else 0)
                else:
                    setattr(o.contents, k, get(k))
        if w is not None:
            o.contents.w = w
        return o

    def default_seed_fields(self):
        o = self.lib.mem_opt_init()
        d = {k: getattr(o.contents, k) for k in SEED_OPT_FIELDS if k != "no_exact"}
        d["no_exact"] = 1 if o.contents.flag & MEM_F_NO_EXACT else 0
        d["w"] = o.contents.w
        self.libc.free(o)
        return d

    def intervals(self, bwt: BwtT, o, read: np.ndarray) -> np.ndarray:
        """every bi-interval of mem_insert_seed's smem_next2 loop in visiting order, with the filter's verdict (fmi.SMEM_DTYPE)"""
        oc = o.contents
        read = np.ascontiguousarray(read, np.uint8)
        out = []
        if read.size < oc.min_seed_len:
            return np.zeros(0, fmi.SMEM_DTYPE)
        itr = self.lib.smem_itr_init(C.addressof(bwt))
        self.lib.smem_set_query(itr, read.size, read.ctypes.data)
        split_len = min(int(np.float32(oc.min_seed_len) * np.float32(oc.split_factor) + .499), read.size)
        sw = 2 if oc.flag & MEM_F_NO_EXACT else 1
        while True:
            a = self.lib.smem_next2(itr, split_len, oc.split_width, sw)
            if not a:
                break
            for i in range(a.contents.n):
                p = a.contents.a[i]
                qb, qe = p.info >> 32, p.info & 0xffffffff
                out.append((p.x[0], p.x[1], p.x[2], qb, qe, int(not (qe - qb < oc.min_seed_len or p.x[2] > oc.max_occ)), 0))
        self.lib.smem_itr_destroy(itr)
        return np.array(out, fmi.SMEM_DTYPE) if out else np.zeros(0, fmi.SMEM_DTYPE)

    def seeds(self, bwt: BwtT, intervals: np.ndarray, l_pac: int) -> np.ndarray:
        """mem_insert_seed's seed loop over the kept intervals (fmi.SEED_DTYPE), bridging seeds dropped"""
        out = []
        for p in intervals:
            if not p["kept"]:
                continue
            for k in range(int(p["x2"])):
                rb = int(self.lib.bwt_sa(C.addressof(bwt), int(p["x0"]) + k))
                ln = int(p["qend"] - p["qbeg"])
                if rb < l_pac < rb + ln:
                    continue
                out.append((rb, int(p["qbeg"]), ln))
        return np.array(out, fmi.SEED_DTYPE) if out else np.zeros(0, fmi.SEED_DTYPE)

    def _take(self, v, n):
        cnt, seeds = [], []
        for i in range(n):
            c = v.a[i]
            cnt.append(c.n)
            seeds += [(c.seeds[j].rbeg, c.seeds[j].qbeg, c.seeds[j].len) for j in range(c.n)]
        return np.array(cnt, np.int32), (np.array(seeds, fmi.SEED_DTYPE) if seeds else np.zeros(0, fmi.SEED_DTYPE))

    def chains(self, bwt: BwtT, o, l_pac: int, read: np.ndarray):
        """mem_chain, then mem_chain_flt on its result -> ((cnt, seeds) before, (cnt, seeds) after)"""
        read = np.ascontiguousarray(read, np.uint8)
        v = self.lib.mem_chain(o, C.addressof(bwt), l_pac, read.size, read.ctypes.data)
        before = self._take(v, v.n)
        n = self.lib.mem_chain_flt(o, v.n, v.a) if v.n else 0
        after = self._take(v, n)
        for i in range(n):
            self.libc.free(v.a[i].seeds)
        if v.a:
            self.libc.free(v.a)
        return before, after


def sopt_from(d):
    import bpsw_hip
    o = bpsw_hip.default_seed_opt()
    for k in SEED_OPT_FIELDS:
        setattr(o, k, d[k])
    return o


def flat(lists, dtype):
    """list of arrays -> (counts, concatenation)"""
    cnt = np.array([len(a) for a in lists], np.int32)
    return cnt, (np.concatenate(lists).astype(dtype) if len(lists) and cnt.sum() else np.zeros(0, dtype))


def split(cnt, arr):
    at = np.concatenate([[0], np.cumsum(cnt)])
    return [arr[at[i]: at[i + 1]] for i in range(len(cnt))]
