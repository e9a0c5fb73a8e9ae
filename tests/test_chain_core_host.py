"""The chain kernel's algorithm (csrc/bpsw_chain_core.h: the kbtree over a node pool, the traversal over an explicit stack, the
chain weight, the filter with ks_introsort's comparison and swap sequence over indices) compiled for the HOST
(tests/chain_host/chain_host.cpp) and held against (a) the reference's chains as recorded in tests/golden/seed_chain_small.npz and
(b) bpsw_chain_seeds (csrc/bpsw_chain.cpp) on generated seed lists (tests/chain_lists.py).  No GPU: the same header is what
chain_kernel compiles.  Also a stand-alone build of the core under -fsanitize=address,undefined, run as a child."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bpsw_hip
import chain_lists as cl
import fmi_util as fu
from bpsw_hip import fmi
from test_chain_host import _configs, _opt, _same, _weight

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "chain_host", "chain_host.cpp")
HDR = os.path.join(ROOT, "cloud-scale-bwamem_amd", "csrc", "bpsw_chain_core.h")
OUT = os.path.join(HERE, "chain_host", "_build")
INC = ["-I" + os.path.dirname(HDR), "-I" + os.path.join(ROOT, "include")]
ERR_POOL = -100


def _fresh(target):
    return os.path.exists(target) and os.path.getmtime(target) >= max(os.path.getmtime(SRC), os.path.getmtime(HDR))


@pytest.fixture(scope="module")
def core():
    os.makedirs(OUT, exist_ok=True)
    so = os.path.join(OUT, "libchain_host.so")
    if not _fresh(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror"] + INC + ["-o", so, SRC], check=True)
    lib = C.CDLL(so)
    lib.chain_core_seeds.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    lib.chain_core_seeds_ex.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                        C.c_int32, C.c_void_p]
    return lib


def _core(lib, so, w, l_pac, seeds, filt, drop=False, node_cap=-1):
    seeds = np.ascontiguousarray(seeds, fmi.SEED_DTYPE)
    n = int(seeds.shape[0])
    cnt, out = np.zeros(n + 1, np.int32), np.zeros(n + 1, fmi.SEED_DTYPE)
    nc = lib.chain_core_seeds_ex(C.byref(so), w, l_pac, n, seeds.ctypes.data, int(filt), int(drop), node_cap, cnt.ctypes.data, n, out.ctypes.data)
    if nc < 0:
        return nc, None
    return cnt[:nc].copy(), out[: int(cnt[:nc].sum())].copy()


def test_core_against_the_golden(core):
    """every read of every config, filter off and on, field by field; the fixture's four marker families counted as
    test_chain_host.py counts them"""
    w = bpsw_hip.default_opt().w
    seen = {"equal_pos": 0, "many": 0, "ties": 0, "dropped": 0}
    gold = np.load(fu.GOLDEN)
    for key, gi, od in _configs(gold):
        so, l_pac = _opt(od), int(gold[f"g{gi}_l_pac"])
        seeds = fu.split(gold[key + "_seed_cnt"], gold[key + "_seeds"])
        at0 = np.concatenate([[0], np.cumsum(gold[key + "_chain_cnt"])])
        at1 = np.concatenate([[0], np.cumsum(gold[key + "_flt_cnt"])])
        cs0 = fu.split(gold[key + "_chain_seed_cnt"], gold[key + "_chain_seeds"])
        cs1 = fu.split(gold[key + "_flt_seed_cnt"], gold[key + "_flt_seeds"])
        for r, s in enumerate(seeds):
            for filt, at, cs, cnts in ((False, at0, cs0, gold[key + "_chain_seed_cnt"]), (True, at1, cs1, gold[key + "_flt_seed_cnt"])):
                cnt, out = _core(core, so, w, l_pac, s, filt)
                assert np.array_equal(cnt, cnts[at[r]: at[r + 1]]), (key, r, filt)
                assert _same(out, np.concatenate(cs[at[r]: at[r + 1]] + [np.zeros(0, fmi.SEED_DTYPE)])), (key, r, filt)
            pos = [int(c["rbeg"][0]) for c in cs0[at0[r]: at0[r + 1]]]
            seen["equal_pos"] += len(pos) != len(set(pos))
            seen["many"] += len(pos) > 15
            seen["dropped"] += at1[r + 1] - at1[r] < len(pos)
            wts = [_weight(c) for c in cs0[at0[r]: at0[r + 1]]]
            seen["ties"] += len(wts) > 2 and len(set(wts)) < len(wts)
    assert seen["equal_pos"] and seen["many"] and seen["dropped"] and seen["ties"], seen


@pytest.fixture(scope="module")
def lists():
    return cl.cases()


def test_core_against_chain_seeds_on_generated_lists(core, lists):
    met = {"chains": 0, "multi_seed": 0, "dropped": 0, "equal_pos": 0}
    for name, od, w, l_pac, seeds in lists:
        so = cl.sopt(od)
        for filt in (False, True):
            want_cnt, want = bpsw_hip.chain_seeds(so, w, l_pac, seeds, filter=filt)
            cnt, out = _core(core, so, w, l_pac, seeds, filt)
            assert np.array_equal(cnt, want_cnt), (name, filt)
            assert _same(out, want), (name, filt)
            if not filt:
                n_all = cnt.size
                first = out["rbeg"][np.concatenate([[0], np.cumsum(cnt)[:-1]])] if cnt.size else np.zeros(0, np.int64)
                met["equal_pos"] += first.size != np.unique(first).size
                met["multi_seed"] += int((cnt > 1).sum())
            else:
                met["dropped"] += cnt.size < n_all
        met["chains"] = max(met["chains"], n_all)
    assert met["chains"] >= 2000 and met["multi_seed"] and met["dropped"] and met["equal_pos"], met


def test_bridging_seeds_are_dropped_by_the_core(core):
    rng = np.random.default_rng(5)
    l_pac = 80_000
    s = cl.clustered(200, rng, l_pac=l_pac, spots=10)
    s["rbeg"][::3] = l_pac - 50 + rng.integers(0, 80, s["rbeg"][::3].size)
    bridging = (s["rbeg"] < l_pac) & (l_pac < s["rbeg"] + s["len"])
    assert 5 < bridging.sum() < s.size
    so = bpsw_hip.default_seed_opt()
    for filt in (False, True):
        want_cnt, want = bpsw_hip.chain_seeds(so, 100, l_pac, s[~bridging], filter=filt)
        cnt, out = _core(core, so, 100, l_pac, s, filt, drop=True)
        assert np.array_equal(cnt, want_cnt) and _same(out, want)


def test_bad_seeds_are_refused(core):
    so = bpsw_hip.default_seed_opt()
    good = cl.clustered(5, np.random.default_rng(1), spots=2)
    for field, v in (("len", 0), ("qbeg", -1)):
        bad = good.copy()
        bad[field][3] = v
        assert _core(core, so, 100, cl.L_PAC, bad, True)[0] == -1


def test_node_pool_bound(core, lists):
    """The pool of m / 7 + 2 nodes holds the 2 000-chain tree (ascending insertion: every node but the rightmost of a level stays
    at its minimum of 7 keys, the tree that takes the most nodes); a pool one node smaller is refused with the error flag."""
    so = bpsw_hip.default_seed_opt()
    name, od, w, l_pac, seeds = next(c for c in lists if c[0] == "distinct_2000_ascending")
    m = int(seeds.shape[0])
    cnt, _ = _core(core, so, w, l_pac, seeds, False, node_cap=m // 7 + 2)
    assert cnt.size == 2000
    assert _core(core, so, w, l_pac, seeds, False, node_cap=m // 7 + 1)[0] == ERR_POOL
    assert _core(core, so, w, l_pac, seeds, True, node_cap=1)[0] == ERR_POOL


def test_core_under_address_and_undefined_sanitizers():
    """a program of its own (no Python in the process): the core over 4 000 generated lists, every workspace malloc'd at exactly
    work_bytes()"""
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "chain_host_san")
    if not _fresh(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan",
                        "-DCHAIN_HOST_MAIN"] + INC + ["-o", exe, SRC], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "chain core:" in p.stdout
