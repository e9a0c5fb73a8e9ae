"""tests/fmi_util.py builds the FM-index the seeding tests load; it is a helper, not the code under test, so it is pinned here on the
reference's own C (oracle/_ref/libbwaref.so): bwt_sa over EVERY row gives back the suffix array, and bwt_match_exact counts what a
brute-force scan of the doubled text counts.  The parts that need no reference (the suffix array itself, the block layout) run always."""
import ctypes as C
import os

import numpy as np
import pytest

import fmi_util as fu
import pyoracle

needs_ref = pytest.mark.skipif(not os.path.exists(pyoracle.REF_SO), reason="oracle/_ref/libbwaref.so not built (reference tree absent)")


def _genome(l_pac, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, l_pac).astype(np.uint8)
    g[100:160] = np.tile(np.array([0, 1], np.uint8), 30)   # a low-complexity stretch: long common prefixes in the sort
    g[400:480] = g[200:280]                                 # and a repeat
    return g


def test_suffix_array_is_sorted_and_complete():
    g = _genome(701, 1)
    text = fu.doubled(g)
    sa = fu.suffix_array(text)
    assert sorted(sa.tolist()) == list(range(text.size + 1)) and sa[0] == text.size
    b = text.tobytes()
    suf = [b[i:] for i in sa[1:]]
    assert all(suf[i] < suf[i + 1] for i in range(len(suf) - 1))


@pytest.mark.parametrize("sa_intv", [1, 8, 32])
def test_block_layout_and_sampling(sa_intv):
    g = _genome(701, 2)
    idx, sa = fu.build_index(g, sa_intv)
    assert idx.seq_len == 1402 and idx.seq_len % 128 and idx.L2[4] == idx.seq_len
    assert idx.bwt.size == (idx.seq_len + 15) // 16 + ((idx.seq_len + 127) // 128 + 1) * 8
    assert idx.sa[0] == -1 and np.array_equal(idx.sa[1:], sa[sa_intv::sa_intv]) and idx.n_sa == (idx.seq_len + sa_intv) // sa_intv
    # the counts in front of block b are the occurrences in the first 128 b bases of the BWT string, read back from the base words
    words = []
    for blk in range((idx.seq_len + 127) // 128):
        words.append(idx.bwt[blk * 16 + 8: min(blk * 16 + 16, idx.bwt.size - 8)])
    w = np.concatenate(words)
    bases = np.array([(int(w[i >> 4]) >> ((~i & 15) << 1)) & 3 for i in range(idx.seq_len)])
    for blk in (0, 1, 5, idx.seq_len >> 7):
        cnt = idx.bwt[blk * 16: blk * 16 + 8].view("<u8")
        assert cnt.tolist() == np.bincount(bases[: blk * 128], minlength=4).tolist()
    assert np.bincount(bases, minlength=4).tolist() == np.diff(idx.L2).tolist()


@needs_ref
@pytest.mark.parametrize("l_pac,sa_intv", [(701, 1), (701, 8), (1333, 32)])
def test_reference_bwt_sa_over_every_row_gives_the_suffix_array(l_pac, sa_intv):
    idx, sa = fu.build_index(_genome(l_pac, 3), sa_intv)
    ref = fu.RefSeeding(pyoracle.REF_SO)
    bwt = fu.ref_bwt(idx)
    got = [ref.lib.bwt_sa(C.addressof(bwt), k) for k in range(1, idx.seq_len + 1)]
    assert got == sa[1:].tolist()


@needs_ref
def test_reference_bwt_match_exact_counts_like_brute_force():
    g = _genome(1333, 4)
    idx, _ = fu.build_index(g, 8)
    text = fu.doubled(g)
    ref = fu.RefSeeding(pyoracle.REF_SO)
    bwt = fu.ref_bwt(idx)
    rng = np.random.default_rng(5)
    b = text.tobytes()
    subs = [text[p: p + ln] for p, ln in zip(rng.integers(0, text.size - 40, 60), rng.integers(1, 40, 60))]
    subs += [text[110:118], text[205:260], text[:12], text[-12:], np.array([3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3], np.uint8)]
    for s in subs:
        s = np.ascontiguousarray(s, np.uint8)
        pat, brute, at = s.tobytes(), 0, -1
        while (at := b.find(pat, at + 1)) >= 0:
            brute += 1
        assert ref.lib.bwt_match_exact(C.addressof(bwt), s.size, s.ctypes.data, None, None) == brute, s
