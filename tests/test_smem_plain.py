"""The plain reference of seeding (tests/smem_plain.py: bisection over the full suffix array, no BWT) against the reference's own C:
the counts and digests of tests/golden/seed_index_edges.npz for every genome, option set and read of tests/index_cases.py, the
records themselves where oracle/_ref/libbwaref.so is built, and the intervals and seeds that tests/golden/seed_chain_small.npz
holds for its two genomes.  Also the census: the conditions on the input that tests/test_seed_index_edges_gpu.py rests on.
No GPU: this pins the yardstick, not the kernels."""
import os

import numpy as np
import pytest

import fmi_util as fu
import index_cases as ic
import pyoracle
import smem_plain
from bpsw_hip import fmi

check_recording = ic.check_recording


@pytest.fixture(scope="module")
def rec():
    return ic.recording()


def test_option_defaults_are_the_reference_s():
    gold = np.load(fu.GOLDEN)
    d = dict(zip(gold["opt_default_names"], gold["opt_default_values"]))
    assert {k: float(v) for k, v in ic.DEFAULTS.items()} == {k: float(d[k]) for k in ic.DEFAULTS}


@pytest.mark.parametrize("name", ic.GENOMES)
def test_plain_reference_gives_the_recording(rec, name):
    assert ic.reads_digest(name) == rec[f"{name}_reads"], f"{name}: the recording was made from other inputs (make_seed_edges_golden.py)"
    for optset in ic.OPTION_SETS:
        check_recording(rec, f"{name}_{optset}", *ic.expected(name, optset))
    check_recording(rec, f"{name}_every_row_one", *ic.expected(name, "every_row", True))


def test_every_row_is_the_suffix_array(rec):
    """the yardstick of the GPU test's every-row walk: under every_row a one-base read's seeds are the suffix array's rows of that base"""
    for name in ic.GENOMES:
        ix = ic.plain_index(name)
        iv, sd = ic.expected(name, "every_row", True)
        for c in range(4):
            rows = ix.sa_full[ix.L2[c] + 1: ix.L2[c + 1] + 1]
            # (a base that does not occur: x2 == 0 <= split_width == 0, so the re-seeding pass emits the empty interval once more)
            assert len(iv[c]) == (1 if rows.size else 2), (name, c, iv[c])
            assert np.all(iv[c]["x0"] == ix.L2[c] + 1) and np.all(iv[c]["x2"] == rows.size) and np.all(iv[c]["kept"] == 1)
            assert np.array_equal(sd[c]["rbeg"], rows) and np.all(sd[c]["len"] == 1), (name, c)
        assert sum(len(s) for s in sd) == ix.seq_len   # no one-base seed bridges: every row from 1 to seq_len, once


@pytest.mark.skipif(not os.path.exists(pyoracle.REF_SO), reason="oracle/_ref/libbwaref.so not built (reference tree absent)")
@pytest.mark.parametrize("name", ic.GENOMES)
def test_plain_reference_against_the_live_reference(name):
    ref = fu.RefSeeding(pyoracle.REF_SO)
    g, sa = ic.genome(name)
    idx, _ = fu.build_index(g, 8, sa_full=sa)
    bwt = fu.ref_bwt(idx)
    for optset, od in ic.OPTION_SETS.items():
        o = ref.opt(od)
        try:
            for one in (False, True) if optset == "every_row" else (False,):
                iv, sd = ic.expected(name, optset, one)
                for k, r in enumerate(ic.ONE_BASE if one else ic.reads(name)):
                    wi = ref.intervals(bwt, o, r)
                    ws = ref.seeds(bwt, wi, g.size)
                    for got, want, what in ((iv[k], wi, "intervals"), (sd[k], ws, "seeds")):
                        assert got.shape == want.shape and got.tobytes() == want.tobytes(), \
                            f"{name} / {optset} / read {k} {r.tolist()}: {what}\nplain {got}\nreference {want}"
        finally:
            ref.libc.free(o)


@pytest.mark.parametrize("ci", [0, 1, 2, 3])
def test_plain_reference_on_the_older_fixture(ci):
    """seed_chain_small.npz: two genomes of 3 019 and 9 043 bases with repeats, recorded in full"""
    gold = np.load(fu.GOLDEN)
    gi = int(gold["configs"][ci][0])
    l_pac = int(gold[f"g{gi}_l_pac"])
    ix = smem_plain.PlainIndex(fu.unpack_pac(gold[f"g{gi}_pac"], l_pac))
    key = f"c{ci}"
    opt = {k: (float(v) if k in ("split_factor", "chain_drop_ratio", "mask_level") else int(v)) for k, v in zip(fu.SEED_OPT_FIELDS, gold[key + "_opt"])}
    reads = fu.split(gold[f"g{gi}_read_len"], gold[f"g{gi}_read_pool"])
    iv = [smem_plain.intervals(ix, opt, r) for r in reads]
    icnt, ivs = fu.flat(iv, fmi.SMEM_DTYPE)
    scnt, sds = fu.flat([smem_plain.seeds(ix, i) for i in iv], fmi.SEED_DTYPE)
    assert np.array_equal(icnt, gold[key + "_intv_cnt"]) and np.array_equal(scnt, gold[key + "_seed_cnt"])
    for got, want in ((ivs, gold[key + "_intv"]), (sds, gold[key + "_seeds"])):
        for f in got.dtype.names:
            assert np.array_equal(got[f], want[f]), (key, f)


def test_census():
    """what the GPU tests rest on is a property of the input: counted here, on the plain reference's output"""
    assert ic.census_failures() == []
    g, o = ic.ROW_LIMIT_BATCH
    assert ic.census(g, o)["over16"] > 64
    iv, _ = ic.expected("runs", "every_row")
    reads = ic.reads("runs")
    assert all(any(len(r) == 256 and np.array_equal(r, w) for r in reads) for w in ic.limit_reads())
    assert max(len(i) for i in ic.expected("one_block", "every_row")[0]) >= 200
    # a kept zero-width interval is the start interval of a base that does not occur, with x0 that base's first row
    for name in ("no_cg", "a_only"):
        ix = ic.plain_index(name)
        for i, r in zip(ic.expected(name, "defaults")[0], ic.reads(name)):
            for p in i[i["x2"] == 0]:
                c = int(r[p["qbeg"]])
                assert ix.L2[c + 1] == ix.L2[c] and p["x0"] == ix.L2[c] + 1
