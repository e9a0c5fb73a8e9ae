"""FASTQ parsing as far as it can be held without a device.

1. The yardsticks against each other: the plain Python parser (tests/fastq_plain.py) on the recording of the reference's own bseq_read
   (tests/golden/fastq_cases.npz), the recording against the live bseq_read where oracle/_ref/libbwaref.so exists, and the case texts
   against what their names claim (a '\\n' at byte 15, 16, 1023, 1024, 4095, 4096; lengths 1023, 1024, 1025).
2. csrc/bpsw_fastq_core.h compiled for the HOST in a program of its own (tests/fastq_host/fastq_host.cpp) under
   -fsanitize=address,undefined: every recorded case, then a few thousand generated records against an independent splitter.
3. csrc/bpsw_fastq.hip compiles for gfx950 without scratch memory.
4. BPSW_FASTQ_HOST through the built library, without a context, against both yardsticks and with the refusals' exact words."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bpsw_hip
import fastq_cases as fc
import fastq_plain as fp
import pyoracle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "cloud-scale-bwamem_amd", "csrc")
SRC = os.path.join(HERE, "fastq_host", "fastq_host.cpp")
HDR = os.path.join(CSRC, "bpsw_fastq_core.h")
OUT = os.path.join(HERE, "fastq_host", "_build")
INC = ["-I" + CSRC, "-I" + os.path.join(ROOT, "include")]
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ARRAYS = ("read_len", "read_off", "read_pool", "qual_pool", "name_off", "name_pool")
H = bpsw_hip.FASTQ_HOST


@pytest.fixture(scope="module")
def recorded():
    return fc.load()


def _fresh(target, *deps):
    return os.path.exists(target) and os.path.getmtime(target) >= max(os.path.getmtime(d) for d in deps)


# ---- 1. the yardsticks ------------------------------------------------------------------------------------------------------------------
def test_the_case_texts_are_what_their_names_claim(recorded):
    for p in (15, 16, 1023, 1024, 4095, 4096):
        assert fc.CASES[f"newline_at_{p}"][0][p: p + 1] == b"\n"
    for n in (1023, 1024, 1025):
        assert len(fc.CASES[f"length_{n}"][0]) == n
    assert b"\n" not in fc.CASES["long_header"][0][:1024] and fc.CASES["long_header"][0].index(b"\n") == 1100
    assert set(recorded) == set(fc.CASES) | set(fc.CUT_CASES)
    for name, (t1, t2, _) in fc.CASES.items():
        assert recorded[name]["text1"] == t1 and recorded[name]["text2"] == t2, name
    assert os.path.getsize(fc.GOLDEN) < 200_000


@pytest.mark.parametrize("name", list(fc.CASES))
def test_plain_parser_on_the_recording(recorded, name):
    t1, t2, flags = fc.CASES[name]
    r, p = recorded[name], fp.parse(t1, t2, flags)
    n = p["n_reads"]
    pairs = t2 is not None or bool(flags & fp.PAIR_NAMES)
    assert n == (len(r["l_seq"]) & ~1 if flags & fp.INTERLEAVED else len(r["l_seq"]))
    assert list(p["read_len"]) == list(r["l_seq"][:n]) and p["reads"] == r["seqs"][:n] and p["quals"] == r["quals"][:n]
    assert p["names"] == r["names"][:n:2 if pairs else 1]
    assert not pairs or r["names"][0:n:2] == r["names"][1:n:2]


@pytest.mark.parametrize("name", list(fc.CUT_CASES))
def test_plain_parser_stops_where_the_reference_stops(recorded, name):
    with pytest.raises(fp.Refused) as e:
        fp.parse(fc.CUT_CASES[name], None, fp.FINAL)
    assert e.value.record == len(recorded[name]["l_seq"]) and e.value.key in ("len_diff", "truncated")


@pytest.mark.skipif(not os.path.exists(pyoracle.REF_SO), reason="oracle/_ref/libbwaref.so not built (reference tree absent)")
def test_the_recording_is_what_the_reference_returns(recorded):
    for name, r in recorded.items():
        got = fc.ref_bseq_read(pyoracle.REF_SO, r["text1"], r["text2"])
        assert [g[0] for g in got] == list(r["l_seq"]) and [g[1] for g in got] == r["names"], name
        assert [g[2] for g in got] == r["seqs"] and [g[3] for g in got] == r["quals"], name


# ---- 2. the core under the sanitizers ------------------------------------------------------------------------------------------------------
def _cases_file(path, recorded):
    def put(b):
        return struct.pack("<q", len(b)) + b
    out = [struct.pack("<q", len(recorded))]
    for name, r in recorded.items():
        flags = fc.CASES[name][2] if name in fc.CASES else fp.FINAL
        stops = -1 if name in fc.CASES else len(r["l_seq"])
        n = len(r["l_seq"]) & ~1 if flags & fp.INTERLEAVED else len(r["l_seq"])
        out += [put(name.encode()), struct.pack("<qqq", flags, r["text2"] is not None, stops), put(r["text1"]), put(r["text2"] or b""),
                struct.pack("<q", 0 if stops >= 0 else n)]
        if stops < 0:
            for k in range(n):
                out += [put(r["names"][k]), put(r["seqs"][k]), put(r["quals"][k])]
    with open(path, "wb") as f:
        f.write(b"".join(out))


def test_core_under_address_and_undefined_sanitizers(recorded):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "fastq_host_san")
    if not _fresh(exe, SRC, HDR):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"] + INC + ["-o", exe, SRC], check=True)
    cases = os.path.join(OUT, "cases.bin")
    _cases_file(cases, recorded)
    p = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"fastq core: (\d+) recorded cases, (\d+) reads: equal", p.stdout)
    assert m and int(m.group(1)) == len(recorded) and int(m.group(2)) > 600, p.stdout
    m = re.search(r"fastq core: (\d+) generated records in (\d+) texts \((\d+) of pairs\), (\d+) cut, (\d+) refused: equal", p.stdout)
    assert m, p.stdout
    records, texts, pair_texts, cut, refused = (int(x) for x in m.groups())
    assert records > 3000 and texts == 400 and pair_texts == 200 and cut > 150 and refused > 150


# ---- 3. the kernels' resources --------------------------------------------------------------------------------------------------------------
def test_the_fastq_kernels_compile_for_gfx950_without_scratch():
    os.makedirs(OUT, exist_ok=True)
    src = os.path.join(CSRC, "bpsw_fastq.hip")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Werror", "-Rpass-analysis=kernel-resource-usage"] + INC +
                       ["-c", src, "-o", os.path.join(OUT, "bpsw_fastq.o")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    names = re.findall(r"Function Name: (\S+)", p.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stderr)]
    for k in ("fastq_count_kernel", "fastq_lines_kernel", "fastq_record_kernel", "fastq_emit_kernel"):
        assert any(k in nm for nm in names), (k, names)
    assert len(scratch) == len(names) and not any(scratch), list(zip(names, scratch))


# ---- 4. BPSW_FASTQ_HOST through the library: no device, no context ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.CASES))
def test_host_flag_against_both_yardsticks(recorded, name):
    t1, t2, flags = fc.CASES[name]
    want, r = fp.parse(t1, t2, flags), recorded[name]
    got = bpsw_hip.fastq_parse(t1, t2, flags | H)
    assert got.n_reads == want["n_reads"] and got.consumed == want["consumed"]
    for k in ARRAYS:
        assert np.array_equal(getattr(got, k), want[k]), k
    n = got.n_reads
    assert list(got.read_len) == list(r["l_seq"][:n]) and bytes(got.qual_pool) == b"".join(r["quals"][:n])
    step = 2 if (t2 is not None or flags & fp.PAIR_NAMES) else 1
    assert bytes(got.name_pool) == b"".join(r["names"][:n:step])
    assert bpsw_hip.last_fastq_times()[:4] == (0.0, 0.0, 0.0, 0.0)


GOOD = fc.rec(b"g0", b"ACGT") + fc.rec(b"g1", b"TTGACA")
REFUSALS = [   # (what, text1, text2, flags, kwargs, code, the exact error text)
    ("missing @", GOOD + b"r2\nACGT\n+\nIIII\n", None, 1, {}, -1, "fastq_parse: record 2 of text 1: the header line does not begin with '@' (not four-line FASTQ)"),
    ("missing +", GOOD + b"@r2\nACGT\nx\nIIII\n", None, 1, {}, -1, "fastq_parse: record 2 of text 1: the third line does not begin with '+' (not four-line FASTQ)"),
    ("lengths differ", GOOD + b"@r2\nACGT\n+\nIII\n", None, 1, {}, -1, "fastq_parse: record 2 of text 1: the quality line is not as long as the read"),
    ("empty read", b"@r0\n\n+\n\n", None, 1, {}, -1, "fastq_parse: record 0 of text 1: the read is empty"),
    ("empty name", b"@\tc\nA\n+\nI\n", None, 1, {}, -1, "fastq_parse: record 0 of text 1: the name is empty"),
    ("- in a read", GOOD + b"@r2\nAC-T\n+\nIIII\n", None, 0, {}, -1, "fastq_parse: record 2 of text 1: '-' in the read"),
    ("byte below 4", GOOD + b"@r2\n\x00CGT\n+\nIIII\n", None, 0, {}, -1, "fastq_parse: record 2 of text 1: a byte below 4 in the read"),
    ("the lower of two", b"@a\nA-\n+\nII\n" + GOOD + b"x\nA\n+\nI\n", None, 1, {}, -1, "fastq_parse: record 0 of text 1: '-' in the read"),
    ("text ends in a record", GOOD + b"@r2\nACGT\n", None, 1, {}, -1, "fastq_parse: record 2 of text 1: the text ends inside the record (not four-line FASTQ)"),
    ("pair names", GOOD, GOOD.replace(b"@g1", b"@g2"), 1, {}, -1, "fastq_parse: record 1 of text 2 (pair 1): the name differs from the first end's"),
    ("5 000 bare newlines", b"\n" * 5000, None, 1, {"max_reads": 4}, -1,
     "fastq_parse: record 0 of text 1: the header line does not begin with '@' (not four-line FASTQ)"),
    ("unknown flag", GOOD, None, 32, {}, -1, "fastq_parse: unknown flag"),
    ("interleaved and two texts", GOOD, GOOD, 2, {}, -1, "fastq_parse: BPSW_FASTQ_INTERLEAVED with two texts"),
    ("max_reads one short", GOOD, None, 1, {"max_reads": 1}, -3, "fastq_parse: the outputs are too small (needed: 2 reads, 10 pool bytes, 4 name bytes)"),
    ("pool_cap one short", GOOD, None, 1, {"pool_cap": 9}, -3, "fastq_parse: the outputs are too small (needed: 2 reads, 10 pool bytes, 4 name bytes)"),
    ("name_cap one short", GOOD, None, 1, {"name_cap": 3}, -3, "fastq_parse: the outputs are too small (needed: 2 reads, 10 pool bytes, 4 name bytes)"),
]


@pytest.mark.parametrize("what,t1,t2,flags,kw,code,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_host_flag_refusals_in_fixed_words(what, t1, t2, flags, kw, code, text):
    with pytest.raises(bpsw_hip.FastqError) as e:
        bpsw_hip.fastq_parse(t1, t2, flags | H, **kw)
    assert e.value.rc == code and str(e.value) == f"bpsw_fastq_parse failed ({code}): {text}"
    if code == -3:
        assert e.value.needed == (2, 10, 4) == bpsw_hip.fastq_parse(t1, t2, flags | H, max_reads=2, pool_cap=10, name_cap=4).needed
    elif flags < 16 and not (flags & 2 and t2):   # the plain parser refuses the same record for the same reason
        with pytest.raises(fp.Refused) as plain:
            fp.parse(t1, t2, flags)
        assert plain.value.message("fastq_parse") == text


def test_host_flag_streams_and_needs_no_context():
    whole = fc.CASES["count_65"][0]
    want = fp.parse(whole, None, fp.FINAL)
    carry, lens = b"", []
    for a, b in ((0, 700), (700, 1024), (1024, len(whole))):
        chunk = carry + whole[a:b]
        r = bpsw_hip.fastq_parse(chunk, None, H | (fp.FINAL if b == len(whole) else 0))
        lens += list(r.read_len)
        carry = chunk[r.consumed[0]:]
    assert carry == b"" and lens == list(want["read_len"])
    with pytest.raises(bpsw_hip.FastqError, match="null argument"):   # without the flag a context is needed: no quiet fall-back
        bpsw_hip.fastq_parse(whole, None, fp.FINAL)
