"""csrc/bpsw_bam_sort_core.h -- the walk's step, the record checks, the key and the BAI of bpsw_bam_sort -- on the HOST.

tests/bam_sort_host/bam_sort_host.cpp is a program of its own under -fsanitize=address,undefined (no Python in the sanitized process):
it applies the rules serially to streams this file writes, each copied to a heap block of exactly its size, and writes the records'
offsets, their keys, std::stable_sort's permutation by the key and the BAI.  Here they are compared with the yardstick
(tests/bam_sort_plain.py): the offsets with the records' own lengths, the keys with the documented packing, the permutation with Python's
stable sort, the BAI byte for byte.  The last test compiles bpsw_bam_sort.hip for gfx950 and asserts that no kernel uses scratch."""
import os
import random
import re
import shutil
import struct
import subprocess

import pytest

import bam_plain as bp
import bam_sort_cases as bc
import bam_sort_plain as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "bam_sort_host", "bam_sort_host.cpp")
CSRC = os.path.join(ROOT, "cloud-scale-bwamem_amd", "csrc")
HDRS = [os.path.join(CSRC, h) for h in ("bpsw_bam_sort_core.h", "bpsw_bam_core.h", "bpsw_sam_core.h")]
OUT = os.path.join(HERE, "bam_sort_host", "_build")
P0 = 65280


def build_host(sanitize=True):
    """-> the program's path (built when it is older than its sources)"""
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "bam_sort_host_san" if sanitize else "bam_sort_host")
    if not (os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(p) for p in [SRC] + HDRS)):
        san = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
               "-static-libubsan"] if sanitize else ["-O2"]
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function"] + san + ["-I" + CSRC, "-o", exe, SRC], check=True)
    return exe


def run_host(exe, cases, tag):
    """cases: [(lens, file_off, P, bounds, stream)] -> per case ("ok", offsets, keys, perm, bai) | ("chain", segment, offset) |
    ("record", index, reason); and the milliseconds the program printed"""
    src, dst = os.path.join(OUT, tag + ".in"), os.path.join(OUT, tag + ".out")
    with open(src, "wb") as f:
        for lens, file_off, p, bounds, stream in cases:
            f.write(struct.pack("<I%di" % len(lens), len(lens), *lens) + struct.pack("<qII", file_off, p, len(bounds)))
            f.write(struct.pack("<%dq" % len(bounds), *bounds) + struct.pack("<Q", len(stream)) + stream)
    r = subprocess.run([exe, "run", src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    blob, at, out = open(dst, "rb").read(), 0, []
    for _ in cases:
        verdict = struct.unpack_from("<I", blob, at)[0]
        at += 4
        if verdict:
            out.append((("chain", "record")[verdict - 1],) + struct.unpack_from("<QQ", blob, at))
            at += 16
            continue
        n = struct.unpack_from("<Q", blob, at)[0]
        cols = [list(struct.unpack_from("<%d%s" % (n, t), blob, at + 8 + 8 * n * k)) for k, t in enumerate("qQq")]
        at += 8 + 24 * n
        m = struct.unpack_from("<Q", blob, at)[0]
        out.append(("ok", cols[0], cols[1], cols[2], blob[at + 8: at + 8 + m]))
        at += 8 + m
    assert at == len(blob)
    return out, [float(x) for x in r.stdout.split()]


def whole(records, lens, p=P0, file_off=0, bounds=None):
    stream = b"".join(records)
    return (lens, file_off, p, bounds or [0, len(stream)], stream)


def check(result, records, lens, p=P0, file_off=0):
    kind, off, keys, perm, bai = result
    assert kind == "ok"
    assert off == sp.offsets_of(records)[0]
    assert keys == [bc.key_of(r, lens) for r in records] and all(k < 1 << bc.key_bits(lens) for k in keys)
    assert perm == sorted(range(len(records)), key=lambda i: sp.sort_key(records[i], len(lens)))
    srt, want = bc.expect(records, lens, p, file_off)
    assert [records[i] for i in perm] == srt
    assert bai == want


@pytest.fixture(scope="module")
def exe():
    return build_host(True)


def test_counts_around_a_wavefront_and_a_sort_tile(exe):
    lens = [100000, 3000]
    sets = [bc.random_records(n, lens, 100 + n) for n in (0, 1, 2, 63, 64, 65, 4095, 4096, 4097)]
    out, _ = run_host(exe, [whole(r, lens) for r in sets], "counts")
    for res, recs in zip(out, sets):
        check(res, recs, lens)


def test_ties_and_orders(exe):
    lens = [5000, 70000]
    base = bc.random_records(300, lens, 7)
    same = [bc.with_pos(bc.with_ref_id(r, 1), 1234) for r in base if sp.fields(r)[0] >= 0 and not sp.fields(r)[3] & 16]
    unplaced = bc.random_records(50, lens, 8, unplaced_every=1)
    srt = sp.sort_records(base, 2)
    strands = bc.records_of([bc.placed(b"s%d" % k, 0, 77, 100, random.Random(k), flag=(16, 0)[k % 2]) for k in range(10)], 2)
    sets = [same, unplaced, srt, srt[::-1], strands]
    out, _ = run_host(exe, [whole(r, lens) for r in sets], "ties")
    for res, recs in zip(out, sets):
        check(res, recs, lens)
    assert out[0][3] == list(range(len(same))) and out[1][3] == list(range(50)) and out[2][3] == list(range(300))
    assert out[4][3] == [1, 3, 5, 7, 9, 0, 2, 4, 6, 8]


@pytest.mark.parametrize("n_ref", [1, 255, 256, 257])
def test_key_widths_by_the_number_of_contigs(exe, n_ref):
    lens = [1, 255, 65536, 1 << 29][: min(n_ref, 4)] + [1000] * max(0, n_ref - 4)
    recs = bc.random_records(400, lens, n_ref) + bc.edge_records(lens, n_ref + 1)
    (res,), _ = run_host(exe, [whole(recs, lens, 1021, 12345)], "width%d" % n_ref)
    check(res, recs, lens, 1021, 12345)
    refs, _ = sp.parse_bai(res[4])
    if n_ref >= 4:
        assert 4680 + (((1 << 29) - 1) >> 14) + 1 in refs[3][0] and len(refs[3][2]) == 1 << 15     # the top bin, the last linear window


@pytest.mark.parametrize("longest", [1, 255, 65536, 1 << 29])
def test_key_widths_by_the_longest_contig(exe, longest):
    lens = [longest, 1]
    recs = bc.random_records(200, lens, longest % 1000) + bc.edge_records(lens, 3)
    (res,), _ = run_host(exe, [whole(recs, lens, 256)], "longest%d" % longest)
    check(res, recs, lens, 256)
    assert bc.key_bits(lens) == 2 + longest.bit_length() + 1


def test_segments(exe):
    lens = [40000, 900]
    recs = bc.random_records(130, lens, 21)
    off, size = sp.offsets_of(recs)
    cases = [whole(recs, lens, bounds=[0, size]), whole(recs, lens, bounds=[0, off[70], size]),
             whole(recs, lens, bounds=[0] + off[2::2] + [size]), whole(recs, lens, bounds=[0, 0, off[5], off[5], size, size])]
    assert len(cases[2][3]) == 66
    out, _ = run_host(exe, cases, "segments")
    for res in out:
        check(res, recs, lens)


def test_block_edges_and_file_offsets(exe):
    lens = [300000]
    recs = bc.random_records(40, lens, 5, unplaced_every=0)
    size = sum(len(r) for r in recs)
    cases = [(p, f) for p in (64, 256, 1021, P0, size - 1, size, size + 1) for f in (0, 4242)]
    out, _ = run_host(exe, [whole(recs, lens, p, f) for p, f in cases], "edges")
    for res, (p, f) in zip(out, cases):
        check(res, recs, lens, p, f)


def test_refusals(exe):
    lens = [40000, 900]
    recs = bc.random_records(20, lens, 33)
    off, size = sp.offsets_of(recs)
    stream = b"".join(recs)
    short = bc.with_block_size(recs[4], 31)
    least = 32 + recs[5][12] + 4 * struct.unpack_from("<H", recs[5], 16)[0] + (struct.unpack_from("<I", recs[5], 20)[0] + 1) // 2 \
        + struct.unpack_from("<I", recs[5], 20)[0]
    header = bp.bam_header_stream(bp.sam_header_text([b"c0", b"c1"], lens), [b"c0", b"c1"], lens)
    placed = next(k for k, r in enumerate(recs) if sp.fields(r)[0] == 1)
    cases = [
        whole(recs, lens, bounds=[0, off[7] + 9, size]),                                    # a segment that ends inside a record
        whole(recs, lens, bounds=[0, size - 2]),                                            # ... inside the last length field's record
        (lens, 0, P0, [0, len(header) + size], header + stream),                            # a header in front
        whole(recs[:3] + [bc.with_ref_id(recs[3], 2)] + recs[4:], lens),                    # refID = n_seqs
        whole(recs[:3] + [bc.with_ref_id(recs[3], -2)] + recs[4:], lens),
        whole(recs[:4] + [short] + recs[5:], lens),                                         # a block_size of 31
        whole(recs[:5] + [bc.with_block_size(recs[5], least - 1)] + recs[6:], lens),        # one byte less than its fields need
        whole(recs[:5] + [bc.with_block_size(recs[5], least)] + recs[6:], lens),            # exactly what they need: fine (no tags)
        whole(recs[:placed] + [bc.with_pos(recs[placed], 900)] + recs[placed + 1:], lens),  # pos = the contig's length
        whole(recs[:placed] + [bc.with_pos(recs[placed], -2)] + recs[placed + 1:], lens),
        whole(recs[:placed] + [bc.with_pos(bc.with_ref_id(recs[placed], -1), 5)] + recs[placed + 1:], lens),   # a pos without a contig
    ]
    out, _ = run_host(exe, cases, "refusals")
    assert out[0] == ("chain", 0, off[7]) and out[1] == ("chain", 0, off[-1])
    assert out[2][0] == "chain" and out[2][1:] == (0, 0)
    assert out[3] == ("record", 3, 2) and out[4] == ("record", 3, 2)
    assert out[5] == ("record", 4, 1) and out[6] == ("record", 5, 1) and out[7][0] == "ok"
    assert out[8] == ("record", placed, 3) and out[9] == ("record", placed, 3) and out[10] == ("record", placed, 3)


def test_kernels_compile_for_gfx950_without_scratch():
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} not found: the device build of bpsw_bam_sort_core.h cannot be checked")
    os.makedirs(OUT, exist_ok=True)
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-c",
                        "-Rpass-analysis=kernel-resource-usage", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o",
                        os.path.join(OUT, "bpsw_bam_sort_gfx950.o"), os.path.join(CSRC, "bpsw_bam_sort.hip")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    for kernel in ("bam_walk_kernel", "bam_key_kernel", "bam_len_kernel", "bam_gather_kernel"):
        m = re.search(r"Function Name: \S*" + kernel + r".*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)", p.stderr, re.S)
        assert m, f"no resource remark for {kernel}:\n{p.stderr[-2000:]}"
        assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (0, 0, 0), f"{kernel}: scratch {m.group(1)}, spills {m.group(2)} / {m.group(3)}"
