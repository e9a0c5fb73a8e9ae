"""Test helper (numpy only): the genomes the FM-index construction (bpsw_fmi_build, csrc/bpsw_index.hip, and its host twin
tests/index_host) is tested on -- deterministic, nothing stored.  Every genome's property is asserted on the index that
fmi_util.build_index makes of it (tests/test_fmi_builder.py pins that builder on the reference), so a changed builder or generator cannot
quietly lose a case.

The sort's tile is TILE suffixes a workgroup (stats slot 4 of bpsw_last_fmi_build_stats; the GPU test asserts that it still is).  The
suffix count seq_len + 1 == 2 l_pac + 1 is odd and the tile is even, so of tile - 1, tile, tile + 1 and 3 tile + 1 suffixes the second
cannot be had from any genome; the twin, whose tile is settable to any number, runs a case with the tile equal to the suffix count."""
import ctypes as C
import functools
import os

import numpy as np

import fmi_util as fu
import index_cases as ic
from bpsw_hip import fmi

REF_SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libbwaref.so")

TILE = 4096
SA_INTVS = (1, 8, 32)


def _rng(seed, n):
    return np.random.default_rng(seed).integers(0, 4, n).astype(np.uint8)


def _make(name):
    if name in ic.GENOMES:
        return np.array(ic.genome(name)[0])
    if name.startswith("len"):                       # l_pac 1, 2, 3, 4, 5, 7: partial pac bytes, seq_len below one word
        return _rng(40 + int(name[3:]), int(name[3:]))
    if name == "palindrome":                         # x || revcomp(x): the doubled text is the same strand twice
        x = _rng(7, 2048)
        return np.concatenate([x, ic.revcomp(x)]).astype(np.uint8)
    if name == "a5000":
        return np.zeros(5000, np.uint8)
    if name == "acg5000":
        return np.tile(np.array([0, 1, 2], np.uint8), 1667)[:5000]
    if name == "random150k":
        return _rng(11, 150_000)
    if name == "tile_minus_1":                       # TILE - 1 suffixes: one workgroup, its last step a lane short
        return _rng(12, (TILE - 2) // 2)
    if name == "tile_plus_1":                        # TILE + 1: a second workgroup for one suffix
        return _rng(13, TILE // 2)
    if name == "three_tiles_plus_1":
        return _rng(14, 3 * TILE // 2)
    raise KeyError(name)


SMALL = tuple("len%d" % n for n in (1, 2, 3, 4, 5, 7))
LONG_ROUNDS = ("palindrome", "a5000", "acg5000")     # 13 doubling rounds from a one-base first key
TILE_EDGES = ("tile_minus_1", "tile_plus_1", "three_tiles_plus_1")
NAMES = tuple(ic.GENOMES) + SMALL + LONG_ROUNDS + ("random150k",) + TILE_EDGES


def _holds(name, g, idx):
    n, t = idx.seq_len, fu.doubled(g)
    if name in ic.GENOMES:
        return n == 2 * g.size                      # (index_cases.genome has asserted the genome's own property)
    if name in SMALL:
        return n == 2 * int(name[3:]) and n < 16
    if name == "palindrome":
        return n == 8192 and np.array_equal(t[:4096], t[4096:])
    if name == "a5000":
        return n == 10000 and idx.L2[1] == 5000 and idx.L2[3] == 5000 and idx.L2[4] == 10000
    if name == "acg5000":
        return n == 10000 and np.array_equal(g[:6], [0, 1, 2, 0, 1, 2]) and np.array_equal(g[3:], g[:-3])
    if name == "random150k":
        return n == 300_000 and n + 1 >= 3 * TILE
    return {"tile_minus_1": n + 1 == TILE - 1, "tile_plus_1": n + 1 == TILE + 1, "three_tiles_plus_1": n + 1 == 3 * TILE + 1}[name]


@functools.lru_cache(maxsize=None)
def genome(name):
    """-> (bases, packed pac bytes, full suffix array of the doubled text plus sentinel)"""
    g = _make(name)
    idx, sa = fu.build_index(g, 8)
    assert _holds(name, g, idx), (name, idx.seq_len, idx.primary, idx.L2)
    pac = fu.pack_pac(g)
    for a in (g, pac, sa):
        a.setflags(write=False)
    return g, pac, sa


@functools.lru_cache(maxsize=None)
def expected(name, sa_intv):
    """fmi_util.build_index's index of a genome at a sampling interval (the suffix array is made once a genome)"""
    g, _, sa = genome(name)
    idx, _ = fu.build_index(g, sa_intv, sa_full=sa)
    for a in (idx.L2, idx.bwt, idx.sa):
        a.setflags(write=False)
    return idx


def one_sample_intv(name):
    """a power of two above seq_len: the sampled suffix array is its first entry alone"""
    n = 2 * genome(name)[0].size
    v = 1
    while v <= n:
        v <<= 1
    return v


def differences(got, want):
    """the fields in which two fmi.FmIndex differ (none, if all is well)"""
    bad = []
    if (int(got.primary), int(got.seq_len), int(got.sa_intv)) != (int(want.primary), int(want.seq_len), int(want.sa_intv)):
        bad.append(("primary/seq_len/sa_intv", (got.primary, got.seq_len, got.sa_intv), (want.primary, want.seq_len, want.sa_intv)))
    if not np.array_equal(np.asarray(got.L2, np.int64), want.L2):
        bad.append(("L2", list(got.L2), list(want.L2)))
    for f in ("bwt", "sa"):
        a, b = getattr(got, f), getattr(want, f)
        if a.shape != b.shape or a.dtype != b.dtype:
            bad.append((f, a.shape, b.shape))
        elif not np.array_equal(a, b):
            at = int(np.nonzero(a != b)[0][0])
            bad.append((f, "first at %d of %d: %d != %d" % (at, a.size, a[at], b[at])))
    return bad


# ---- the files ------------------------------------------------------------------------------------------------------------------------
def files_round_trip(idx, tmp_path, full_sa=None):
    """write_index_files, then read_index_files gives the index back; with the reference's library also bwt_restore_bwt + bwt_restore_sa on
    the files and bwt_sa over every row against the suffix array (the host test on build_index's arrays, the GPU test on a built index)"""
    b, s = str(tmp_path / "x.bwt"), str(tmp_path / "x.sa")
    fmi.write_index_files(idx, b, s)
    assert os.path.getsize(b) == 40 + 4 * idx.bwt.size and os.path.getsize(s) == 56 + 8 * (idx.sa.size - 1)
    back = fmi.read_index_files(b, s)
    assert not differences(back, idx)
    if full_sa is None or not os.path.exists(REF_SO):
        return False
    lib = C.CDLL(REF_SO)
    lib.bwt_restore_bwt.restype = C.c_void_p
    lib.bwt_restore_bwt.argtypes = [C.c_char_p]
    lib.bwt_restore_sa.argtypes = [C.c_char_p, C.c_void_p]
    lib.bwt_sa.restype = C.c_uint64
    lib.bwt_sa.argtypes = [C.c_void_p, C.c_uint64]
    lib.bwt_destroy.argtypes = [C.c_void_p]
    p = lib.bwt_restore_bwt(b.encode())
    lib.bwt_restore_sa(s.encode(), p)
    rows = np.array([lib.bwt_sa(p, r) for r in range(1, idx.seq_len + 1)], np.int64)
    lib.bwt_destroy(p)
    assert np.array_equal(rows, full_sa[1:])
    return True
