"""csrc/bpsw_bam_core.h -- the bytes of a BAM record, the CRC-32 with its combine, the bytes around a BGZF payload -- on the HOST, and the
host-only header entries through the library.

tests/bam_host/bam_host.cpp is a program of its own under -fsanitize=address,undefined (no Python in the sanitized process): it runs
the core over the line records in pairs that tests/sam_pe_host generates (that file is included, not copied), every record into a heap
block of exactly its length and into one a byte short, and dumps per line the SAM text sam_line_write gives and the record's bytes.
Here tests/bam_plain.py -- the specification in plain Python, which parses the text and knows nothing of the line table -- is applied
to the text and compared byte for byte, and the dumped CRCs are held against zlib.crc32.  The same file must compile for gfx950 with
no scratch in any kernel."""
import os
import re
import shutil
import struct
import subprocess
import zlib

import pytest

import bam_plain as bp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "bam_host", "bam_host.cpp")
GEN = os.path.join(HERE, "sam_pe_host", "sam_pe_host.cpp")
CSRC = os.path.join(ROOT, "cloud-scale-bwamem_amd", "csrc")
HDRS = [os.path.join(CSRC, "bpsw_bam_core.h"), os.path.join(CSRC, "bpsw_sam_core.h")]
OUT = os.path.join(HERE, "bam_host", "_build")
INC = ["-I" + CSRC]


def _fresh(target):
    return os.path.exists(target) and os.path.getmtime(target) >= max(os.path.getmtime(p) for p in [SRC, GEN] + HDRS)


@pytest.fixture(scope="module")
def dumps():
    """builds and runs the program once -> (the path of the record dump, the path of the CRC dump, its stdout)"""
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "bam_host_san")
    if not _fresh(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"] + INC +
                       ["-o", exe, SRC], check=True)
    rec, crc = os.path.join(OUT, "records.bin"), os.path.join(OUT, "crc.txt")
    p = subprocess.run([exe, rec, crc], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    return rec, crc, p.stdout


def _blobs(data):
    at = 0

    def u32():
        nonlocal at
        v = struct.unpack_from("<I", data, at)[0]
        at += 4
        return v

    def blob():
        nonlocal at
        n = u32()
        b = data[at: at + n]
        at += n
        return b
    return u32, blob, lambda: at


def test_records_equal_the_specification_applied_to_the_text(dumps):
    rec, _, out = dumps
    assert "bam core:" in out and "short ends hold" in out, out
    data = open(rec, "rb").read()
    u32, blob, where = _blobs(data)
    lines = 0
    seen = {"odd": 0, "hidden": 0, "no_qual": 0, "rev": 0, "unplaced": 0, "next": 0, "sa": 0, "hard": 0, "wide_tag": 0, "far_bin": 0}
    for _ in range(u32()):
        have_qual = u32()
        names = [blob() for _ in range(u32())]
        ref_id = {}
        for rid, n in enumerate(names):
            ref_id.setdefault(n, rid)
        for _ in range(u32()):
            text, got = blob(), blob()
            f = text.rstrip(b"\n").split(b"\t")
            # a generated table may name two contigs alike; a line that names one of those cannot be mapped back to an index
            if any(c not in (b"*", b"=") and names.count(c) > 1 for c in (f[2], f[6])):
                continue
            if have_qual and f[10] == b"*" and len(f[9]) == 1 and f[9] != b"*":
                continue   # (one base of quality '*': the text cannot say whether that is a quality or none)
            want = bp.sam_to_bam(text, ref_id)
            assert got == want, f"{text!r}\n got {got.hex()}\nwant {want.hex()}"
            lines += 1
            flag = int(f[1])
            seen["odd"] += f[9] != b"*" and len(f[9]) & 1
            seen["hidden"] += f[9] == b"*"
            seen["no_qual"] += f[9] != b"*" and f[10] == b"*"
            seen["rev"] += bool(flag & 0x10) and f[9] != b"*"
            seen["unplaced"] += f[2] == b"*"
            seen["next"] += f[6] not in (b"*", b"=")
            seen["sa"] += any(t.startswith(b"SA:Z:") for t in f[11:])
            seen["hard"] += b"H" in f[5]
            seen["wide_tag"] += any(t[:5] in (b"AS:i:", b"XS:i:") and int(t[5:]) > 255 for t in f[11:])
            seen["far_bin"] += f[2] != b"*" and int(f[3]) > (1 << 29)
    assert where() == len(data)
    assert lines > 20000, lines
    assert all(v >= 50 for v in seen.values()), seen


def test_crc_and_its_combine_equal_zlib(dumps):
    _, crc, _ = dumps
    rows = open(crc).read().split("\n")
    assert rows[0].startswith("buf ")
    buf = bytes.fromhex(rows[0][4:])
    n = {"crc": 0, "comb": 0, "fold": 0}
    lens = set()
    for row in rows[1:]:
        if not row:
            continue
        w = row.split()
        v = [int(x) for x in w[1:]]
        if w[0] == "crc":
            assert zlib.crc32(buf[v[0]: v[0] + v[1]]) == v[2], row
            lens.add(v[1])
        elif w[0] == "comb":   # crc32_combine(crc(p[:k]), crc(p[k:len]), len - k)
            assert zlib.crc32(buf[v[0]: v[0] + v[1]]) == v[3], row
        elif w[0] == "fold":   # the 64-slice fold of bgzf_frame_kernel
            assert zlib.crc32(buf[v[0]: v[0] + v[1]]) == v[2], row
        else:
            raise AssertionError(row)
        n[w[0]] += 1
    assert lens == set(range(0, 71)) | set(range(1016, 1025))
    assert n["crc"] == 4 * 80 and n["comb"] > 4 * 2500 and n["fold"] == 4 * 12, n


def test_core_compiles_for_gfx950_without_scratch():
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} not found: the device build of bpsw_bam_core.h cannot be checked")
    os.makedirs(OUT, exist_ok=True)
    obj = os.path.join(OUT, "bam_host_gfx950.o")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-x", "hip", "-c",
                        "-Rpass-analysis=kernel-resource-usage"] + INC + ["-o", obj, SRC], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    remarks = p.stderr
    for kernel in ("bam_len_kernel", "bam_write_kernel", "bgzf_crc_kernel"):
        m = re.search(r"Function Name: \S*" + kernel + r".*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)", remarks, re.S)
        assert m, f"no resource remark for {kernel}:\n{remarks[-2000:]}"
        assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (0, 0, 0), f"{kernel}: scratch {m.group(1)}, spills {m.group(2)} / {m.group(3)}"


# ---- the header entries: host only, through the library ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import bpsw_hip
    bpsw_hip.load_library()
    return bpsw_hip


TABLE = (["chr1", "", "a-long-name:with,marks"], [248956422, 5, 2147483647])
EXTRA = b"@RG\tID:g1\tSM:s\n@PG\tID:bpsw\tPN:bpsw\n"


def test_sam_header_text(lib):
    names, lens = TABLE
    assert lib.sam_header(lens, names, EXTRA) == bp.sam_header_text(names, lens, EXTRA)
    assert lib.sam_header(lens, None) == bp.sam_header_text(["", "", ""], lens)
    assert lib.sam_header([], []) == b"@HD\tVN:1.6\tSO:unsorted\n"


@pytest.mark.parametrize("payload", [0, 1, 7, 64, 65280])
def test_bam_header_blocks(lib, payload):
    names, lens = TABLE
    assert lib.bam_set_block_payload(payload) == 0
    try:
        got = lib.bam_header(lens, names, EXTRA)
    finally:
        assert lib.bam_set_block_payload(0) == 0
    want = bp.bam_header_stream(bp.sam_header_text(names, lens, EXTRA), names, lens)
    members = bp.bgzf_members(got)   # (BSIZE, CRC32 and ISIZE of every member)
    p = payload or 65280
    assert [len(m[0]) for m in members] == [p] * (len(want) // p) + ([len(want) % p] if len(want) % p else [])
    assert len(got) == len(want) + 31 * len(members)
    assert b"".join(m[0] for m in members) == want
    text, refs, at = bp.parse_bam_header(want)
    assert refs == [(b"chr1", lens[0]), (b"ctg2", lens[1]), (names[2].encode(), lens[2])] and at == len(want)


def test_eof_block_and_capacities(lib):
    assert lib.bam_eof() == bp.EOF_BLOCK == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    assert bp.bgzf_inflate(lib.bam_eof()) == b""
    for call in (lambda cap: lib.bam_eof(cap=cap), lambda cap: lib.sam_header([5], ["c"], cap=cap), lambda cap: lib.bam_header([5], ["c"], cap=cap)):
        whole = call(None)
        with pytest.raises(lib.BpswError, match="too small"):
            call(len(whole) - 1)
        assert call(len(whole)) == whole


def test_block_payload_setter_refuses_what_bgzf_cannot_hold(lib):
    assert lib.bam_set_block_payload(65281) == -1 and lib.bam_set_block_payload(-1) == -1
    assert lib.bam_set_block_payload(65280) == 0 and lib.bam_set_block_payload(1) == 0 and lib.bam_set_block_payload(0) == 0
    assert lib.BGZF_PAYLOAD == 65280
