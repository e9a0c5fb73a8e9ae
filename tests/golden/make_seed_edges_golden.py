"""Writes tests/golden/seed_index_edges.npz from the reference's own C (oracle/_ref/libbwaref.so): for every genome, option set and
read of tests/index_cases.py the number of bi-intervals and of seeds that mem_insert_seed's two loops give on
fmi_util.build_index(genome, 8), and the first 8 bytes of SHA-256 over the records of each list (fmi.SMEM_DTYPE, fmi.SEED_DTYPE).
Digests, not records: the records come to megabytes.  Run from the repository root, after `make -C oracle ref`:
    python tests/golden/make_seed_edges_golden.py
It prints the census of the cases the tests rest on and refuses to write a fixture in which one is missing."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "cloud-scale-bwamem_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import fmi_util as fu  # noqa: E402
import index_cases as ic  # noqa: E402
import pyoracle  # noqa: E402
import smem_plain  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "seed_index_edges.npz")


def main():
    ref = fu.RefSeeding(pyoracle.REF_SO)
    out = {}
    for name in ic.GENOMES:
        g, sa = ic.genome(name)
        idx, _ = fu.build_index(g, 8, sa_full=sa)
        bwt = fu.ref_bwt(idx)
        out[f"{name}_reads"] = ic.reads_digest(name)
        for optset, od in ic.OPTION_SETS.items():
            o = ref.opt(od)
            for tag, reads in (("", ic.reads(name)),) + ((("_one", ic.ONE_BASE),) if optset == "every_row" else ()):
                iv = [ref.intervals(bwt, o, r) for r in reads]
                sd = [ref.seeds(bwt, i, g.size) for i in iv]
                key = f"{name}_{optset}{tag}"
                out[key + "_intv_cnt"] = np.array([len(i) for i in iv], np.int32)
                out[key + "_seed_cnt"] = np.array([len(s) for s in sd], np.int32)
                out[key + "_intv_dig"] = np.array([smem_plain.digest(i) for i in iv], np.uint64)
                out[key + "_seed_dig"] = np.array([smem_plain.digest(s) for s in sd], np.uint64)
            ref.libc.free(o)
    table = {(g, o): ic.census(g, o) for g in ic.GENOMES for o in ic.OPTION_SETS}
    for k, c in table.items():
        print(k, c)
    missing = ic.census_failures(table)
    assert not missing, f"the cases do not hold what the tests rest on: {missing}"
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
