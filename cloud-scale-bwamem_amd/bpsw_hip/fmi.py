"""The FM-index as the aligner's .bwt / .sa files hold it, and the records of the seeding entries (include/bpsw.h:
bpsw_fmi_load, bpsw_seed_batch, bpsw_seed_batch_ex, bpsw_chain_seeds, bpsw_worker1_batch).  Data carriers only: nothing is computed here."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

SEED_MAX_QLEN = 256

SMEM_DTYPE = np.dtype([("x0", "<i8"), ("x1", "<i8"), ("x2", "<i8"), ("qbeg", "<i4"), ("qend", "<i4"), ("kept", "<i4"), ("pad_", "<i4")])
SEED_DTYPE = np.dtype([("rbeg", "<i8"), ("qbeg", "<i4"), ("len", "<i4")])
assert SMEM_DTYPE.itemsize == 40 and SEED_DTYPE.itemsize == 16


class SeedOpt(C.Structure):  # bpsw_seed_opt_t
    _fields_ = [(n, C.c_int32) for n in ("min_seed_len", "max_occ", "split_width", "max_chain_gap", "no_exact")] + \
               [(n, C.c_float) for n in ("split_factor", "chain_drop_ratio", "mask_level")]


class Reads(C.Structure):  # bpsw_reads_t
    _fields_ = [("n_reads", C.c_int32), ("read_len", C.c_void_p), ("read_off", C.c_void_p), ("read_pool", C.c_void_p),
                ("read_pool_bytes", C.c_size_t)]


@dataclass
class FmIndex:
    """bwt_t as BWTType loads it: `bwt` is the interleaved uint32 array (every 128 bases four 64-bit occurrence counts, then eight
    words of 2-bit bases), `sa` the suffix array sampled every sa_intv rows with sa[0] == -1."""
    primary: int
    L2: np.ndarray      # int64 [5], L2[0] == 0, L2[4] == seq_len
    seq_len: int
    bwt: np.ndarray     # uint32
    sa_intv: int
    sa: np.ndarray      # int64 [(seq_len + sa_intv) // sa_intv]

    @property
    def n_sa(self) -> int:
        return int(self.sa.shape[0])


def read_index_files(bwt_path: str, sa_path: str) -> FmIndex:
    """The .bwt and .sa files of `bwa index` (bwt_restore_bwt / bwt_restore_sa, native/bwt.c:389-430)."""
    raw = np.fromfile(bwt_path, dtype="<u4")
    head = raw[:10].view("<i8")
    L2 = np.concatenate([[0], head[1:5]]).astype(np.int64)
    bwt = np.ascontiguousarray(raw[10:])
    s = np.fromfile(sa_path, dtype="<i8")
    if int(s[0]) != int(head[0]) or int(s[6]) != int(L2[4]):
        raise ValueError("SA-BWT inconsistency: primary or seq_len differ")
    sa_intv = int(s[5])
    sa = np.concatenate([[-1], s[7:]]).astype(np.int64)
    return FmIndex(primary=int(head[0]), L2=L2, seq_len=int(L2[4]), bwt=bwt, sa_intv=sa_intv, sa=sa)


def write_index_files(idx: FmIndex, bwt_path: str, sa_path: str) -> None:
    """The inverse of read_index_files: the .bwt and .sa files as bwt_dump_bwt / bwt_dump_sa write them (native/bwt.c).  .bwt: primary,
    L2[1..4] (five 64-bit words), then the uint32 array.  .sa: primary, L2[1..4], sa_intv, seq_len (seven 64-bit words), then the
    samples from the second on (the first, -1, is not stored)."""
    L2 = np.asarray(idx.L2, np.int64)
    head = np.concatenate([[int(idx.primary)], L2[1:5]]).astype("<i8")
    with open(bwt_path, "wb") as f:
        f.write(head.tobytes())
        f.write(np.ascontiguousarray(idx.bwt, "<u4").tobytes())
    with open(sa_path, "wb") as f:
        f.write(head.tobytes())
        f.write(np.array([int(idx.sa_intv), int(idx.seq_len)], "<i8").tobytes())
        f.write(np.ascontiguousarray(idx.sa[1:], "<i8").tobytes())


class BuildShape(C.Structure):  # bpsw_fmi_shape_t
    _fields_ = [("primary", C.c_int64), ("L2", C.c_int64 * 5), ("seq_len", C.c_int64), ("bwt_size", C.c_int64), ("n_sa", C.c_int64),
                ("sa_intv", C.c_int32), ("pad_", C.c_int32)]


@dataclass
class ReadBatch:
    read_len: np.ndarray   # int32 [n]
    read_off: np.ndarray   # int64 [n]
    read_pool: np.ndarray  # uint8, codes 0..4

    @property
    def n_reads(self) -> int:
        return int(self.read_len.shape[0])

    @staticmethod
    def from_list(reads) -> "ReadBatch":
        ln = np.array([len(r) for r in reads], np.int32)
        off = np.concatenate([[0], np.cumsum(ln[:-1], dtype=np.int64)]).astype(np.int64) if len(reads) else np.zeros(0, np.int64)
        pool = np.concatenate([np.asarray(r, np.uint8) for r in reads] + [np.zeros(0, np.uint8)])
        return ReadBatch(ln, off, np.ascontiguousarray(pool))

    def as_struct(self) -> Reads:
        st = Reads()
        st.n_reads = self.n_reads
        for f, dt in (("read_len", np.int32), ("read_off", np.int64), ("read_pool", np.uint8)):
            a = getattr(self, f)
            assert a.dtype == dt and a.flags.c_contiguous, f
            setattr(st, f, a.ctypes.data)
        st.read_pool_bytes = self.read_pool.size
        return st
