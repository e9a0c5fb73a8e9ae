"""The job tables of tests/test_ring_pull_gpu.py, and the child process that runs them: `python ring_pull_tables.py OUT.npz` sends every
table through Context.swalign2_batch / matesw_group in THIS process's environment (the switches of csrc/bpsw_sw_runtime.cpp are read
once per process) and writes the results, with what the counters said about each call, to OUT.npz.  Plain numpy from fixed seeds;
the shapes are built around constants of csrc/bpsw_swalign.hip, csrc/bpsw_ring.h and csrc/bpsw_ring_pull_core.h, restated here:
  * a batch with mates of at most 150 bases goes to ring class 3 (a pair per worker) below 8 units = 15 jobs and to the half-wave
    class (two pairs per worker) from there on; a longer mate (up to 256) makes it class 5;
  * the resident kernels take windows of up to 1 024 rows (class 3, half-wave) / 1 536 rows (class 5); one row more is a launch;
  * a worker's slice holds any class-3 / class-5 pair, and a half-wave quartet of up to 4 352 bytes."""
import sys

import numpy as np

import sw_cases as sc



def _case(rng, ql, tl, rev=0, n_at=None):
    mate = sc._r(rng, ql)
    w = sc._embed(rng, mate, tl, second=tl > 2 * ql + 50)
    if n_at is not None and tl:
        w[min(n_at, tl - 1)] = 4
    return (sc._rc(mate) if rev else mate, w, rev)


def _jobs(pairs, tight_t_pool=False):
    j = sc.jobs_from(pairs)
    if tight_t_pool:   # the last window ends on the pool's last byte (jobs_from pads both pools by sixteen bytes)
        end = int(j["t_off"][-1] + j["t_len"][-1])
        assert end % 16 == 0
        j["t_pool"] = j["t_pool"][:end].copy()
    return j


def tables():
    """name -> (jobs, expect), expect in ('pull', 'launch'): how the batch must have gone with the pull on"""
    out = {}
    rng = np.random.default_rng(20260)
    # jobs per batch: the trailing single pair, the upper half off, and the unit count at which the half-wave class takes over
    for n in (1, 2, 3, 4, 5, 15, 16, 17):
        pairs = [_case(rng, 150, int(rng.integers(300, 760)), rev=k % 2, n_at=200 if k == 1 else None) for k in range(n)]
        out[f"n{n}"] = (_jobs(pairs), "pull")
    # class 5: every edge mate with every edge window (the longest mate, 256 bases, makes the class); an N in one of them; q_rev both ways
    pairs = []
    for tl in (1, 255, 256, 257, 1535, 1536):
        for ql in (1, 149, 150, 151, 256):
            pairs.append(_case(rng, ql, tl, rev=len(pairs) % 2, n_at=130 if len(pairs) % 7 == 3 else None))
    out["class5_edges"] = (_jobs(pairs), "pull")
    out["class5_edges_tight"] = (_jobs(pairs[:-1] + [_case(rng, 256, 1536)], tight_t_pool=True), "pull")
    # ... and one row more: a launch of its own
    out["class5_1537"] = (_jobs(pairs[:6] + [_case(rng, 256, 1537)]), "launch")
    # class 3 (fewer than fifteen jobs) with its own longest windows
    pairs = [_case(rng, ql, tl, rev=k % 2) for k, (ql, tl) in enumerate(
        [(1, 1), (149, 1024), (150, 1023), (151, 257), (150, 1024), (150, 1024), (149, 255), (1, 256), (171, 1024), (150, 1), (151, 700)])]
    out["class3_edges"] = (_jobs(pairs), "pull")
    out["class3_1025"] = (_jobs(pairs[:5] + [_case(rng, 150, 1025)]), "launch")
    # the half-wave class (eighteen jobs): quartets of the edge windows that fit the slice, a window with an N, q_rev both ways
    pairs = []
    for k in range(18):
        ql = (1, 149, 150)[k % 3]
        tl = (1, 255, 256, 257, 700, 869)[(k // 3 + k) % 6]
        pairs.append(_case(rng, ql, tl, rev=k % 2, n_at=99 if k == 4 else None))
    out["halves_edges"] = (_jobs(pairs), "pull")
    # one mate used by the four jobs of a quartet (and of two class-3 pairs)
    for name, n in (("shared_mate_halves", 16), ("shared_mate_class3", 4)):
        mate = sc._r(rng, 150)
        pairs = [(mate, sc._embed(rng, mate, int(rng.integers(300, 700)), second=False), 0) for _ in range(n)]
        j = _jobs(pairs)
        for k in range(n):
            j["q_off"][k] = j["q_off"][4 * (k // 4)]
        out[name] = (j, "pull")
    # the half-wave class once more with the last window on the pool's last byte
    pairs = [_case(rng, 150, 500) for _ in range(15)] + [_case(rng, 150, 16 * 30)]
    out["halves_tight"] = (_jobs(pairs, tight_t_pool=True), "pull")
    return out


def groups():
    """name -> (read_len, n_pairs, seed, coordinate mode)"""
    return {"group150": (150, 64, 9101, False), "group250": (250, 64, 9102, False), "group150_coords": (150, 64, 9103, True)}


L_PAC = 300_007


def make_group(name):
    from bpsw_hip import synth
    read_len, n_pairs, seed, coords = groups()[name]
    if not coords:
        return synth.rescue_group(n_pairs, read_len=read_len, seed=seed, p_resc=0.4), None
    pac, bases = synth.random_pac(L_PAC, seed=seed)
    return synth.rescue_group(n_pairs, read_len=read_len, seed=seed, l_pac=L_PAC, p_resc=0.4, ref_bases=bases), pac


def main(path):
    import dataclasses
    import time
    import bpsw_hip
    out = {}
    c = bpsw_hip.Context(0)
    opt = sc.apply(bpsw_hip.default_opt(), sc.DEFAULT)
    for name, (jobs, _) in tables().items():
        time.sleep(0.03)
        s0, r0 = c.stats(), c.ring_stats()[1]
        res = c.swalign2_batch(opt, sc.XTRA, **jobs)
        s1, r1 = c.stats(), c.ring_stats()[1]
        out[name] = res
        out[name + ".how"] = np.array([s1.sw_ring_calls - s0.sw_ring_calls, r1 - r0, s1.sw_h2d_ms - s0.sw_h2d_ms], np.float64)
    for name in groups():
        g, pac = make_group(name)
        if pac is not None:
            c.ref_load(pac, L_PAC)
            g = dataclasses.replace(g, ref_pool=None, ref_len=None, ref_off=None)
        s0 = c.stats()
        cnt, regs = c.matesw_group(bpsw_hip.default_opt(), g)
        s1 = c.stats()
        out[name + ".cnt"] = cnt
        out[name + ".regs"] = regs
        out[name + ".how"] = np.array([s1.sw_ring_calls - s0.sw_ring_calls, s1.sw_calls - s0.sw_calls, s1.sw_h2d_ms - s0.sw_h2d_ms], np.float64)
        if pac is not None:
            c.ref_unload()
    out["integrity"] = np.array(c.ring_integrity(), np.int64)
    c.close()
    np.savez(path, **out)


if __name__ == "__main__":
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (os.path.join(root, "cloud-scale-bwamem_amd"), os.path.join(root, "oracle"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    main(sys.argv[1])
