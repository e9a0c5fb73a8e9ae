"""Test helper (numpy only): generated seed lists for the chain core (csrc/bpsw_chain_core.h) and the chain kernel
(csrc/bpsw_chain_dev.hip), shared by tests/test_chain_core_host.py and tests/test_chain_dev_gpu.py.  Every list is a case
(name, seed-option overrides, w, l_pac, seeds); the expected chains are always bpsw_chain_seeds' (csrc/bpsw_chain.cpp, which
tests/test_chain_host.py pins on the reference).  Fixed RNG seeds: the lists are the same in every run."""
import numpy as np

from bpsw_hip import fmi

L_PAC = 1_000_000_000
FAR = 20_011          # further apart than max_chain_gap (10 000): every seed founds a chain of its own


def _seeds(rbeg, qbeg, ln):
    s = np.zeros(len(rbeg), fmi.SEED_DTYPE)
    s["rbeg"], s["qbeg"], s["len"] = rbeg, qbeg, ln
    return s


def distinct(n, order, rng, ln=None, qspan=120):
    """n chains of one seed each on distinct pos, inserted in the given order of pos"""
    pos = 5_000 + FAR * np.arange(n, dtype=np.int64)
    if order == "descending":
        pos = pos[::-1].copy()
    elif order == "shuffled":
        pos = rng.permutation(pos)
    qbeg = rng.integers(0, qspan, n)
    ln = rng.integers(19, 70, n) if ln is None else ln
    return _seeds(pos, qbeg, ln)


def clustered(n, rng, l_pac=L_PAC, spots=None, both_strands=True):
    """seeds of a few loci and diagonals: merges, contained seeds, several seeds a chain"""
    spots = max(2, n // 6) if spots is None else spots
    locus = rng.integers(1_000, 400_000, spots)
    strand = rng.integers(0, 2, spots) * (l_pac if both_strands else 0)
    k = rng.integers(0, spots, n)
    qbeg = rng.integers(0, 200, n)
    ln = rng.integers(19, 60, n)
    rbeg = locus[k] + strand[k] + qbeg + rng.integers(-3, 4, n)
    return _seeds(rbeg, qbeg, ln)


def cases():
    rng = np.random.default_rng(20240611)
    out = []

    def add(name, seeds, w=100, l_pac=L_PAC, **opt):
        out.append((name, opt, w, l_pac, np.ascontiguousarray(seeds)))
    for n in (0, 1, 2, 3, 16, 17, 18):
        add(f"clustered_{n}", clustered(n, rng, spots=3))
        add(f"distinct_{n}", distinct(n, "shuffled", rng))
    for n in (16, 128, 300, 2000):                       # root split, second level, height 3
        for order in ("ascending", "descending", "shuffled"):
            add(f"distinct_{n}_{order}", distinct(n, order, rng))
    for n in (30, 300, 900):                             # a third of the chains on a pos another chain has (the other strand's
        s = distinct(n, "shuffled", rng)                 # test keeps them apart: first seed below l_pac, the next at or above it)
        dup = rng.choice(n, n // 3, replace=False)
        t = s[dup].copy()
        t["qbeg"] = (t["qbeg"] + 150) % 256              # not contained, too far off the diagonal to merge
        both = np.concatenate([s, t])
        add(f"equal_pos_{n}", both[rng.permutation(both.size)], w=20)
    for n in (17, 40, 500):                              # all weights equal: the introsort's ties
        add(f"equal_weight_{n}", distinct(n, "shuffled", rng, ln=np.full(n, 31), qspan=40))
    for n in (40, 700):                                  # weights already sorted / reverse sorted in tree order
        add(f"weights_ascending_{n}", distinct(n, "ascending", rng, ln=19 + np.arange(n), qspan=30))
        add(f"weights_descending_{n}", distinct(n, "ascending", rng, ln=19 + np.arange(n)[::-1], qspan=30))
    for l_pac in (50_000, 200_000):                      # both strands around l_pac
        s = clustered(150, rng, l_pac=l_pac, spots=12)
        s["rbeg"][:50] = l_pac - 60 + rng.integers(0, 90, 50)
        s = s[~((s["rbeg"] < l_pac) & (l_pac < s["rbeg"] + s["len"]))]     # (bridging seeds never reach bpsw_chain_seeds)
        add(f"around_l_pac_{l_pac}", s[rng.permutation(s.size)], l_pac=l_pac)
    for gap, w in ((25, 100), (10_000, 1), (30, 2)):     # merges fail on the gap / on the band
        add(f"tight_gap{gap}_w{w}", clustered(220, rng, spots=9), w=w, max_chain_gap=gap)
    add("filter_other_levels", clustered(260, rng, spots=30), mask_level=0.2, chain_drop_ratio=0.9)
    add("long_3000", clustered(3000, rng, spots=400))
    return out


def sopt(opt):
    import bpsw_hip
    o = bpsw_hip.default_seed_opt()
    for k, v in opt.items():
        setattr(o, k, v)
    return o
