"""The FM-index construction on the CPU: csrc/bpsw_index_core.h played serially by its host twin, against fmi_util.build_index.

tests/index_host/index_host.cpp is a program of its own under -fsanitize=address,undefined (no Python in the sanitized process, nothing
preloaded); its arrays are heap blocks of exactly their size.  It runs every kernel of csrc/bpsw_index.hip lane by lane and tile by
tile: the first keys, the radix sort with the wavefront ranking of its scatter, the flags, the head tables, the new ranks, the BWT words,
the block counts, the packing and the sampling.  The file round trip of fmi.write_index_files is tested here as well, on build_index's
arrays and through the reference's own readers."""
import os
import struct
import subprocess

import numpy as np
import pytest

import fmi_build_cases as bc
from bpsw_hip import fmi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "index_host", "index_host.cpp")
CSRC = os.path.join(ROOT, "cloud-scale-bwamem_amd", "csrc")
HDR = os.path.join(CSRC, "bpsw_index_core.h")
OUT = os.path.join(HERE, "index_host", "_build")


def build_host():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "index_host_san")
    if not (os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(SRC), os.path.getmtime(HDR))):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-O1", "-g", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + CSRC, "-o", exe,
                        SRC], check=True)
    return exe


def run_host(jobs, tag):
    """jobs: [(genome name, sa_intv, first key, tile)] -> per job (fmi.FmIndex, dict(rounds, unresolved_first, passes, tiles))"""
    exe = build_host()
    src, dst = os.path.join(OUT, tag + ".in"), os.path.join(OUT, tag + ".out")
    with open(src, "wb") as f:
        for name, sa_intv, k0, tile in jobs:
            g, pac, _ = bc.genome(name)
            f.write(struct.pack("<q4i", g.size, sa_intv, k0, tile, 0) + pac.tobytes())
    r = subprocess.run([exe, "run", src, dst], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    blob, at, out = open(dst, "rb").read(), 0, []
    for name, sa_intv, k0, tile in jobs:
        head = struct.unpack_from("<13q", blob, at)
        at += 104
        bwt = np.frombuffer(blob, "<u4", head[7], at).copy()
        at += 4 * head[7]
        sa = np.frombuffer(blob, "<i8", head[8], at).copy()
        at += 8 * head[8]
        idx = fmi.FmIndex(primary=head[0], L2=np.array(head[1:6], np.int64), seq_len=head[6], bwt=bwt, sa_intv=sa_intv, sa=sa)
        out.append((idx, dict(rounds=head[9], unresolved_first=head[10], passes=head[11], tiles=head[12])))
    assert at == len(blob)
    return out


def _check(jobs, got):
    bad = []
    for (name, sa_intv, k0, tile), (idx, st) in zip(jobs, got):
        d = bc.differences(idx, bc.expected(name, sa_intv))
        if d:
            bad.append((name, sa_intv, k0, tile, d))
    assert not bad, bad[:4]


def test_twin_default_first_key():
    jobs = [(n, v, 0, 0) for n in bc.NAMES for v in bc.SA_INTVS]
    got = run_host(jobs, "default")
    _check(jobs, got)
    st = {j[0]: s for j, (_, s) in zip(jobs, got)}
    assert st["random150k"]["passes"] >= 8 and st["random150k"]["tiles"] >= 3   # 63 bits of first key: eight passes


def test_twin_one_base_first_key():
    jobs = [(n, v, 1, 0) for n in bc.NAMES for v in bc.SA_INTVS]
    got = run_host(jobs, "one_base")
    _check(jobs, got)
    st = {j[0]: s for j, (_, s) in zip(jobs, got)}
    for n in bc.LONG_ROUNDS:
        assert st[n]["rounds"] >= 12 and st[n]["unresolved_first"] > 0, (n, st[n])
    assert st["random150k"]["rounds"] >= 4 and st["random150k"]["unresolved_first"] > 0, st["random150k"]


def test_twin_tile_of_64_suffixes():
    """a few hundred suffixes span several tiles; 150 000 bases are left to the tests above"""
    names = [n for n in bc.NAMES if n != "random150k"]
    jobs = [(n, v, k0, 64) for n in names for v in bc.SA_INTVS for k0 in (0, 1)]
    got = run_host(jobs, "tile64")
    _check(jobs, got)
    st = {j[0]: s for j, (_, s) in zip(jobs, got)}
    assert st["p_first"]["tiles"] == 4 and st["one_block"]["tiles"] == 3 and st["len1"]["tiles"] == 1


def test_twin_tile_equal_to_the_suffix_count_and_around_it():
    """2 l_pac + 1 suffixes on a tile of exactly as many, one fewer and one more (an odd tile: the twin's alone)"""
    jobs = []
    for name in ("p_first", "tiny", "runs"):
        n = 2 * bc.genome(name)[0].size + 1
        jobs += [(name, 8, k0, t) for t in (n - 1, n, n + 1) for k0 in (0, 1)]
    got = run_host(jobs, "tile_n")
    _check(jobs, got)
    assert [s["tiles"] for _, s in got[:6]] == [2, 2, 1, 1, 1, 1]


@pytest.mark.parametrize("name,sa_intv", [("runs", 8), ("p_block_start", 32), ("len3", 1), ("tiny", 64)])
def test_index_files_round_trip_of_build_index(tmp_path, name, sa_intv):
    bc.files_round_trip(bc.expected(name, sa_intv), tmp_path, bc.genome(name)[2])
