"""Writes tests/golden/seed_chain_small.npz from the reference's own C (oracle/_ref/libbwaref.so): two small genomes, their reads,
and per read what mem_chain goes through -- the bi-intervals of every smem_next2 call, the seeds, the chains before and after
mem_chain_flt -- under three settings (mem_opt_init; max_occ lowered; MEM_F_NO_EXACT).  Run from the repository root:
    python tests/golden/make_seed_golden.py
It prints how many reads show each case the tests rely on, and refuses to write a fixture in which one is missing."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "cloud-scale-bwamem_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import fmi_util as fu  # noqa: E402
import pyoracle  # noqa: E402
from bpsw_hip import fmi  # noqa: E402

W = 100  # mem_opt_init's band width: the chimeric read's filler must be longer


def genome(l_pac, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, l_pac).astype(np.uint8)
    rep = rng.integers(0, 4, 300).astype(np.uint8)
    third = l_pac // 3
    rep_at = [200, third + 150, 2 * third + 100]
    for a in rep_at:                     # one 300-base repeat, three copies
        g[a: a + 300] = rep
    low_at = third - 260                 # one low-complexity stretch: (AC) x 120
    g[low_at: low_at + 240] = np.tile(np.array([0, 1], np.uint8), 120)
    return g, rep_at, low_at


def reads_for(g, rep_at, low_at, sa, seed, n_random):
    rng = np.random.default_rng(seed)
    l_pac = g.size
    text = fu.doubled(g)

    def rc(r):
        r = np.asarray(r, np.uint8)[::-1]
        return np.where(r > 3, 4, 3 - r).astype(np.uint8)
    out, tag = [], []

    def add(r, t):
        out.append(np.asarray(r, np.uint8).copy()); tag.append(t)
    a = 1200 if l_pac > 4000 else 900
    add(g[a: a + 150], "exact")                                   # exact full-length match: re-seeding
    add(g[a: a + 256], "exact256")
    add(g[a: a + 18], "short")                                    # shorter than min_seed_len
    add(g[a: a + 19], "len19")
    add(np.full(60, 4), "allN")
    r = g[a + 300: a + 400].copy(); r[0] = 4; r[-1] = 4; add(r, "N_ends")
    r = g[a + 300: a + 420].copy(); r[60] = 4; add(r, "N_mid")
    r = g[a + 300: a + 420].copy(); r[40:43] = 4; add(rc(r), "N_mid_rev")
    add(rc(g[a + 50: a + 200]), "rev_exact")
    add(text[l_pac - 40: l_pac + 40], "bridge")                   # across the forward/reverse boundary: bridging seeds dropped
    add(text[l_pac - 25: l_pac + 60], "bridge2")
    for row, t in ((1, "row_first"), (text.size, "row_last")):    # the smallest and the largest suffix: rows 1 and seq_len
        p = int(sa[row])
        add(text[max(0, p - 12): p + 40], t)
        add(text[p: p + 40], t + "_bare")
    add(g[0:80], "text_start"); add(g[l_pac - 80:], "fwd_end"); add(text[text.size - 70:], "text_end")
    filler = rng.integers(0, 4, W + 25).astype(np.uint8)
    ca = a + 500
    filler[0] = (g[ca + 50] + 1) & 3; filler[-1] = (g[ca - 1] + 1) & 3
    add(np.concatenate([g[ca: ca + 50], filler, g[ca: ca + 50]]), "chimeric")  # two chains with one pos
    for k in range(3):
        o = 20 + 60 * k
        add(g[rep_at[0] + o: rep_at[0] + o + 100], "repeat")      # three copies: chains of equal weight
        add(rc(g[rep_at[1] + o: rep_at[1] + o + 120]), "repeat_rev")
    add(g[rep_at[1] - 40: rep_at[1] + 110], "repeat_edge")
    add(g[low_at + 10: low_at + 50], "lowcomplex")                # interval above a lowered max_occ
    add(g[low_at + 100: low_at + 200], "lowcomplex_long")
    add(g[low_at - 30: low_at + 60], "lowcomplex_edge")
    r = np.concatenate([g[rep_at[2] + 10: rep_at[2] + 90], g[a: a + 60], g[rep_at[2] + 150: rep_at[2] + 230]]); add(r, "three_part")
    for _ in range(n_random):
        ln = int(rng.integers(19, 257))
        p = int(rng.integers(0, l_pac - ln))
        r = g[p: p + ln].copy()
        for _m in range(int(rng.integers(0, 5))):                 # a few substitutions, sometimes an indel or an N
            q = int(rng.integers(0, ln)); r[q] = (r[q] + int(rng.integers(1, 4))) & 3
        if rng.random() < 0.2:
            q = int(rng.integers(5, ln - 5)); r = np.delete(r, q) if rng.random() < 0.5 else np.insert(r, q, rng.integers(0, 4))
        if rng.random() < 0.15:
            r[int(rng.integers(0, r.size))] = 4
        add(rc(r) if rng.random() < 0.5 else r, "random")
    return out, tag


def main():
    ref = fu.RefSeeding(pyoracle.REF_SO)
    defaults = ref.default_seed_fields()
    variants = [dict(defaults), dict(defaults, max_occ=50), dict(defaults, no_exact=1)]
    out = {"opt_default_names": np.array(list(fu.SEED_OPT_FIELDS) + ["w"]),
           "opt_default_values": np.array([float(defaults[k]) for k in list(fu.SEED_OPT_FIELDS) + ["w"]], np.float64)}
    cases = {"reseed": 0, "equal_pos": 0, "tie": 0, "over_occ": 0, "bridge": 0, "many_chains": 0, "filtered": 0}
    configs = []
    for gi, (l_pac, seed, n_random) in enumerate(((3019, 11, 70), (9043, 12, 75))):
        g, rep_at, low_at = genome(l_pac, seed)
        idx, sa = fu.build_index(g, 8)
        assert (2 * l_pac) % 128 and idx.primary % 128, (l_pac, idx.primary)
        reads, tags = reads_for(g, rep_at, low_at, sa, 100 + seed, n_random)
        rl, rp = fu.flat(reads, np.uint8)
        out[f"g{gi}_pac"] = fu.pack_pac(g); out[f"g{gi}_l_pac"] = np.int64(l_pac)
        out[f"g{gi}_read_len"] = rl; out[f"g{gi}_read_pool"] = rp; out[f"g{gi}_tags"] = np.array(tags)
        bwt = fu.ref_bwt(idx)
        for vi in ((0,) if gi == 0 else (0, 1, 2)):
            o = ref.opt(variants[vi])
            iv, sd, c0, s0, c1, s1, nc0, nc1 = [], [], [], [], [], [], [], []
            for r, t in zip(reads, tags):
                i = ref.intervals(bwt, o, r)
                s_all = sum(int(p["x2"]) for p in i if p["kept"])
                s = ref.seeds(bwt, i, l_pac)
                (bc, bs), (ac, as_) = ref.chains(bwt, o, l_pac, r)
                iv.append(i); sd.append(s); nc0.append(len(bc)); nc1.append(len(ac))
                c0.append(bc); s0.append(bs); c1.append(ac); s1.append(as_)
                # the cases the tests rely on
                lens = i["qend"] - i["qbeg"]
                if len(i) and np.any((lens[:, None] < lens[None, :]) & (i["qbeg"][:, None] >= i["qbeg"][None, :]) & (i["qend"][:, None] <= i["qend"][None, :])):
                    cases["reseed"] += 1
                pos = [int(ch["rbeg"][0]) for ch in fu.split(bc, bs)]
                cases["equal_pos"] += len(pos) != len(set(pos))
                wts = [int(ch["len"].sum()) for ch in fu.split(bc, bs)]
                cases["tie"] += len(wts) > 2 and len(set(wts)) < len(wts)
                cases["over_occ"] += bool(np.any(i["x2"] > o.contents.max_occ)) if len(i) else 0
                cases["bridge"] += len(s) < s_all
                cases["many_chains"] += len(bc) > 15
                cases["filtered"] += len(ac) < len(bc)
            ref.libc.free(o)
            key = f"c{len(configs)}"
            configs.append((gi, vi))
            out[key + "_opt"] = np.array([float(variants[vi][k]) for k in fu.SEED_OPT_FIELDS], np.float64)
            out[key + "_intv_cnt"], out[key + "_intv"] = fu.flat(iv, fmi.SMEM_DTYPE)
            out[key + "_seed_cnt"], out[key + "_seeds"] = fu.flat(sd, fmi.SEED_DTYPE)
            out[key + "_chain_cnt"] = np.array(nc0, np.int32)
            out[key + "_chain_seed_cnt"] = np.concatenate(c0 + [np.zeros(0, np.int32)]).astype(np.int32)
            out[key + "_chain_seeds"] = fu.flat(s0, fmi.SEED_DTYPE)[1]
            out[key + "_flt_cnt"] = np.array(nc1, np.int32)
            out[key + "_flt_seed_cnt"] = np.concatenate(c1 + [np.zeros(0, np.int32)]).astype(np.int32)
            out[key + "_flt_seeds"] = fu.flat(s1, fmi.SEED_DTYPE)[1]
    out["configs"] = np.array(configs, np.int32)
    print(cases, "reads:", [int(out[f"g{g}_read_len"].size) for g in (0, 1)])
    missing = [k for k, v in cases.items() if not v]
    assert not missing, f"the reference does not produce these cases on this data: {missing}"
    np.savez_compressed(fu.GOLDEN, **out)
    print(fu.GOLDEN, os.path.getsize(fu.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
