"""csrc/bpsw_inflate_core.h -- the header walk of a BGZF chunk and the inflate of its blocks -- on the HOST.

tests/inflate_host/inflate_host.cpp is a program of its own under -fsanitize=address,undefined (no Python in the sanitized process,
nothing preloaded): it runs bgzf_walk and inflate_serial, the twin of bgzf_inflate_kernel that plays the 64 lanes in a loop, over the
case table of tests/inflate_cases.py.  The chunk, every block's deflate data and the output stand in heap blocks of exactly their size,
so a read outside a block's data or a write past ISIZE is a sanitizer report.  The yardsticks are zlib, bam_plain.bgzf_members and
fastq_plain; the library's own HOST flags are run through libbPSW_hip.so without a context."""
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import bam_plain as bp
import bpsw_hip
import fastq_cases as fc
import inflate_cases as ic

CSRC = ic.CSRC
ROOT = ic.ROOT


@pytest.fixture(scope="module")
def exe():
    return ic.build_host(True)


@pytest.fixture(scope="module")
def results(exe):
    cs = ic.cases()
    return dict(zip((c.name for c in cs), ic.run_host(exe, [c.chunk for c in cs], "cases")))


def test_the_table_has_a_case_for_every_reason():
    seen = {c.bad[1] for c in ic.refused()}
    assert seen == set(range(1, len(ic.REASONS))), sorted(set(range(1, len(ic.REASONS))) - seen)
    assert len(ic.accepted()) >= 30


@pytest.mark.parametrize("case", ic.cases(), ids=repr)
def test_twin_gives_zlibs_bytes_or_the_reason(results, case):
    r = results[case.name]
    assert r["n_blocks"] == case.n_blocks
    if case.bad is None:
        assert r["reason"] == 0 and r["bad_block"] == -1, (ic.REASONS[r["reason"]], r["bad_block"])
        assert r["data"] == case.want and r["total"] == len(case.want)
        assert r["consumed"] == case.consumed
    else:
        assert (r["bad_block"], ic.REASONS[r["reason"]]) == (case.bad[0], ic.REASONS[case.bad[1]])
        assert r["header"] == case.header


def test_walk_against_bgzf_members(results):
    for case in ic.accepted():
        r = results[case.name]
        members = bp.bgzf_members(case.chunk[: r["consumed"]])
        assert len(members) == r["n_blocks"]
        at = out = 0
        for (payload, total, cdata), (coff, data_off, data_len, isize, crc, out_off) in zip(members, r["blocks"]):
            assert coff == at and out_off == out and isize == len(payload) and data_len == len(cdata)
            assert case.chunk[data_off: data_off + data_len] == cdata
            assert int.from_bytes(case.chunk[coff + total - 8: coff + total - 4], "little") == crc
            at, out = at + total, out + len(payload)
        assert at == r["consumed"] and out == r["total"]


def test_every_truncation_ends_in_a_reason(exe, results):
    """the deflate data of every accepted one-block stream cut short: at every byte for the small ones, at 64 random bytes for the
    large.  Every cut must be refused, and no cut may make the twin read outside the bytes it was given (ASan is the judge)"""
    rng, items = random.Random(17), []
    for case in ic.accepted():
        r = results[case.name]
        if r["n_blocks"] != 1 or r["consumed"] != len(case.chunk):
            continue
        n = r["blocks"][0][2]
        cuts = list(range(n)) if n <= 600 else sorted(rng.sample(range(n), 62) + [0, n - 1])
        items.append((case, cuts))
    assert len(items) >= 25
    got = ic.run_trunc(exe, [(c.chunk, cuts) for c, cuts in items], "trunc")
    for (case, cuts), reasons in zip(items, got):
        assert all(reasons), (case.name, [k for k, x in zip(cuts, reasons) if not x])
        assert ic.R["DATA_ENDS"] in reasons, case.name


def test_reason_texts_are_fixed(exe):
    r = subprocess.run([exe, "text"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    got = dict(line.split(" ", 1) for line in r.stdout.splitlines())
    assert got == {str(ic.R[name]): text for name, text in ic.REASON_TEXT.items()}
    assert "plain gzip, not BGZF" in ic.REASON_TEXT["NO_BC"]


def test_kernel_compiles_for_gfx950_without_scratch():
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} not found: the device build of bpsw_inflate_core.h cannot be checked")
    os.makedirs(ic.OUT, exist_ok=True)
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-c",
                        "-Rpass-analysis=kernel-resource-usage", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o",
                        os.path.join(ic.OUT, "bpsw_bgzf_in_gfx950.o"), os.path.join(CSRC, "bpsw_bgzf_in.hip")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"Function Name: \S*bgzf_inflate_kernel.*?ScratchSize \[bytes/lane\]: (\d+).*?VGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)",
                  p.stderr, re.S)
    assert m, f"no resource remark for bgzf_inflate_kernel:\n{p.stderr[-2000:]}"
    assert (int(m.group(1)), int(m.group(2))) == (0, 0), f"scratch {m.group(1)}, VGPR spills {m.group(2)}"
    assert int(m.group(3)) <= 80 * 1024, "two workgroups no longer fit the 160 KiB of a CU"


# ---- the library's HOST flags, without a context -------------------------------------------------------------------------------------------
def test_bgzf_inflate_host_over_the_table():
    for case in ic.cases():
        if case.bad is None:
            data, n_blocks, consumed = bpsw_hip.bgzf_inflate(case.chunk, bpsw_hip.BGZF_HOST)
            assert (data, n_blocks, consumed) == (case.want, case.n_blocks, case.consumed), case.name
            assert bpsw_hip.last_bgzf_times() == (0.0, 0.0, 0.0)
        else:
            with pytest.raises(bpsw_hip.BgzfError) as e:
                bpsw_hip.bgzf_inflate(case.chunk, bpsw_hip.BGZF_HOST)
            assert e.value.rc == -1, case.name
            assert str(e.value).endswith(f"bgzf_inflate: block {case.bad[0]}: {ic.REASON_TEXT[ic.REASONS[case.bad[1]]]}"), (case.name, str(e.value))


def test_bgzf_inflate_host_refusals_and_capacity():
    text = ic.fastq_like(3000)
    chunk = ic.bgzip(text, 1000)
    H = bpsw_hip.BGZF_HOST

    def refused(rc, words, *a, **kw):
        with pytest.raises(bpsw_hip.BgzfError) as e:
            bpsw_hip.bgzf_inflate(*a, **kw)
        assert e.value.rc == rc and str(e.value).endswith(words), str(e.value)
        return e.value
    e = refused(-3, "bgzf_inflate: out has room for fewer bytes than the blocks hold (*out_needed)", chunk, H, cap=2999)
    assert (e.needed, e.n_blocks, e.consumed) == (3000, 3, len(chunk))
    assert bpsw_hip.bgzf_inflate(chunk, H, cap=3000)[0] == text
    refused(-1, "bgzf_inflate: 5 bytes behind the last whole block (BPSW_BGZF_FINAL)", chunk + chunk[:5], H | bpsw_hip.BGZF_FINAL)
    assert bpsw_hip.bgzf_inflate(chunk + chunk[:5], H) == (text, 3, len(chunk))
    assert bpsw_hip.bgzf_inflate(chunk, H | bpsw_hip.BGZF_FINAL) == (text, 3, len(chunk))
    refused(-1, "bgzf_inflate: unknown flag", chunk, H | 4)
    refused(-1, "bgzf_inflate: null argument", chunk, 0)                      # no context and no BGZF_HOST
    # a malformed header wins over a capacity; malformed data is met only once the capacity holds
    bad_header = chunk + b"XYZ" + bytes(20)
    refused(-1, "bgzf_inflate: block 3: " + ic.REASON_TEXT["MAGIC"], bad_header, H, cap=0)
    crc_case = next(c for c in ic.cases() if c.name == "crc")
    refused(-3, "(*out_needed)", chunk + crc_case.chunk, H, cap=10)
    refused(-1, "bgzf_inflate: block 3: " + ic.REASON_TEXT["CRC"], chunk + crc_case.chunk, H)
    # the inflated total at 2^31: 32 768 blocks of 65 536 zeros
    zeros = ic.frame(bytes(65536), ic.deflate(bytes(65536), 6))
    refused(-4, "bgzf_inflate: 2^31 inflated bytes or more", zeros * 32768, H, cap=0)


def _same_reads(a, b):
    assert a.n_reads == b.n_reads and a.needed == b.needed
    for f in ("read_len", "read_off", "read_pool", "qual_pool", "name_off", "name_pool"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def virtual(chunk, u):
    """the virtual offset of inflated offset u of a chunk, by bgzf_members"""
    at = out = 0
    for payload, total, _ in bp.bgzf_members(chunk):
        if out + len(payload) > u:
            return at << 16 | (u - out)
        at, out = at + total, out + len(payload)
    return at << 16


@pytest.mark.parametrize("payload", [64, 1021, 65280])
def test_fastq_bgzf_parse_host_equals_the_plain_parse(payload):
    H = bpsw_hip.FASTQ_HOST
    for name, (t1, t2, flags) in fc.CASES.items():
        want = bpsw_hip.fastq_parse(t1, t2, flags | H)
        z1, z2 = ic.bgzip(t1, payload, eof=True), None if t2 is None else ic.bgzip(t2, payload)
        got = bpsw_hip.fastq_bgzf_parse(z1, z2, flags | H)
        _same_reads(got, want)
        assert got.consumed[0] == virtual(z1, want.consumed[0]), name
        if t2 is not None:
            assert got.consumed[1] == virtual(z2, want.consumed[1]), name


def test_fastq_bgzf_parse_host_refusals():
    H = bpsw_hip.FASTQ_HOST | bpsw_hip.FASTQ_FINAL
    text = fc.CASES["count_65"][0]
    z = ic.bgzip(text, 300)

    def refused(rc, words, *a, **kw):
        with pytest.raises(bpsw_hip.FastqError) as e:
            bpsw_hip.fastq_bgzf_parse(*a, **kw)
        assert e.value.rc == rc and str(e.value).endswith(words), str(e.value)
    refused(-1, "fastq_bgzf_parse: text 1: the text ends inside a BGZF block", z + z[:9], None, H)
    refused(-1, "fastq_bgzf_parse: text 2: the text ends inside a BGZF block", z, z[:-1], H)
    first = len(bp.bgzf_members(z)[0][0])
    refused(-1, "fastq_bgzf_parse: text 1: skip is not within the first block's bytes", z, None, H, skip=(first + 1, 0))
    refused(-1, "fastq_bgzf_parse: text 1: skip is not within the first block's bytes", z, None, H, skip=(-1, 0))
    refused(-1, "fastq_bgzf_parse: text 1: skip is not within the first block's bytes", b"", None, H, skip=(1, 0))
    plain = next(c for c in ic.cases() if c.name == "header_plain_gzip").chunk
    refused(-1, "fastq_bgzf_parse: text 1: block 0: " + ic.REASON_TEXT["NO_BC"], plain, None, H)
    # an inflate refusal in front of a malformed record: block 2 of a text whose first record is no FASTQ
    bad_text = b"no at sign\nACGT\n+\nIIII\n" + text
    zb = ic.bgzip(bad_text, 300)
    members = bp.bgzf_members(zb)
    at = members[0][1] + members[1][1]
    broken = zb[: at + members[2][1] - 8] + bytes(4) + zb[at + members[2][1] - 4:]
    refused(-1, "fastq_bgzf_parse: record 0 of text 1: the header line does not begin with '@' (not four-line FASTQ)", zb, None, H)
    refused(-1, "fastq_bgzf_parse: text 1: block 2: " + ic.REASON_TEXT["CRC"], broken, None, H)
    # a skip: the parse begins where an earlier call stopped
    rec0 = text.index(b"\n@") + 1
    assert rec0 <= first
    _same_reads(bpsw_hip.fastq_bgzf_parse(z, None, H, skip=(rec0, 0)), bpsw_hip.fastq_parse(text[rec0:], None, H))
