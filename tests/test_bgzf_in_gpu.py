"""FASTQ in as BGZF on the DEVICE: bgzf_inflate_kernel (csrc/bpsw_bgzf_in.hip) against the host twin and zlib over the case table
of tests/inflate_cases.py, bpsw_bgzf_inflate's contract, and the five bpsw_*_bgzf_* FASTQ entries against their plain-text twins.

The yardsticks: zlib and bam_plain.bgzf_members for the bytes, tests/inflate_host (inflate_serial, built without sanitizers here) for
the (block, reason) of a refusal, bpsw_hip.fastq_parse / align_fastq_* on the plain text for the records, the SAM text and the BAM."""
import numpy as np
import pytest

import bam_plain as bp
import bpsw_hip
import fastq_cases as fc
import fastq_plain as fp
import inflate_cases as ic
from test_fastq_gpu import _fastq_of
from test_sam_pe_gpu import PAIR_ORDER
from test_sam_se_gpu import _contig_tables, _load, fixture_reads, gold  # noqa: F401
from test_worker1_gpu import _opt

pytestmark = pytest.mark.gpu

ARRAYS = ("read_len", "read_off", "read_pool", "qual_pool", "name_off", "name_pool")
PATHS = (0, bpsw_hip.FASTQ_HOST)
PAYLOADS = (64, 1021, 65280)


@pytest.fixture(scope="module")
def twin():
    """every case of the table through inflate_serial, once"""
    cs = ic.cases()
    return dict(zip((c.name for c in cs), ic.run_host(ic.build_host(False), [c.chunk for c in cs], "gpu_cases")))


def _refusal(ctx, chunk, flags=0, **kw):
    with pytest.raises(bpsw_hip.BgzfError) as e:
        ctx.bgzf_inflate(chunk, flags, **kw)
    return e.value


def _block_reason(message):
    """'... bgzf_inflate: block N: text' -> (N, reason name)"""
    head, text = message.split("bgzf_inflate: block ", 1)[1].split(": ", 1)
    return int(head), next(name for name, t in ic.REASON_TEXT.items() if t == text)


# ---- device against twin and zlib ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ic.cases(), ids=repr)
def test_device_equals_twin_and_zlib(ctx, twin, case):
    t = twin[case.name]
    if case.bad is None:
        data, n_blocks, consumed = ctx.bgzf_inflate(case.chunk)
        assert data == t["data"] == case.want
        assert (n_blocks, consumed) == (t["n_blocks"], t["consumed"]) == (case.n_blocks, case.consumed)
    else:
        e = _refusal(ctx, case.chunk)
        assert e.rc == -1
        assert _block_reason(str(e)) == (t["bad_block"], ic.REASONS[t["reason"]]) == (case.bad[0], ic.REASONS[case.bad[1]])


# ---- chunk sizes, the place of a bad block, ISIZE at the edges of a 16-byte line --------------------------------------------------------------
def _blocks_of_sizes(sizes, seed=5):
    rng = np.random.default_rng(seed)
    pays = [bytes(rng.integers(65, 70, n, dtype=np.uint8)) for n in sizes]
    return pays, [ic.frame(p, ic.deflate(p, 6)) for p in pays]


@pytest.mark.parametrize("n_blocks", [0, 1, 2, 65, 300])
def test_chunks_of_many_blocks(ctx, n_blocks):
    sizes = [(0, 1, 15, 16, 17, 65535, 65536, 300, 4096)[k % 9] if k < 18 else 100 + 7 * k for k in range(n_blocks)]
    pays, frames = _blocks_of_sizes(sizes)
    chunk = b"".join(frames)
    assert ctx.bgzf_inflate(chunk) == (b"".join(pays), n_blocks, len(chunk))
    assert ctx.bgzf_inflate(chunk, bpsw_hip.BGZF_HOST) == (b"".join(pays), n_blocks, len(chunk))
    if n_blocks < 2:
        return
    # a bad block first, in the middle and last -- and all three at once: the lowest is the one reported
    def broken(k):
        f = frames[k]
        return f[:-8] + bytes([f[-8] ^ 1]) + f[-7:]
    for bad in ([0], [n_blocks // 2], [n_blocks - 1], [n_blocks - 1, n_blocks // 2], [n_blocks // 2, 0, n_blocks - 1]):
        bad_chunk = b"".join(broken(k) if k in bad else f for k, f in enumerate(frames))
        want = (min(bad), "CRC")
        assert _block_reason(str(_refusal(ctx, bad_chunk))) == want
        assert _block_reason(str(_refusal(ctx, bad_chunk, bpsw_hip.BGZF_HOST))) == want


@pytest.mark.parametrize("isize", [0, 1, 15, 16, 17, 65535, 65536])
def test_isize_at_the_edges(ctx, isize):
    """blocks of these sizes behind one another and behind a block of 3 bytes, so that each begins off a 16-byte line of the output"""
    pays, frames = _blocks_of_sizes([3, isize, isize, 5], seed=isize)
    assert ctx.bgzf_inflate(b"".join(frames))[0] == b"".join(pays)


# ---- the entry's contract -------------------------------------------------------------------------------------------------------------------
def test_capacity_limit_flags_and_times(ctx):
    text = ic.fastq_like(200000)
    chunk = ic.bgzip(text)
    e = _refusal(ctx, chunk, cap=len(text) - 1)
    assert e.rc == -3 and (e.needed, e.n_blocks, e.consumed) == (len(text), 4, len(chunk))
    assert ctx.bgzf_inflate(chunk, cap=len(text)) == (text, 4, len(chunk))
    walk, kernel, trip = bpsw_hip.last_bgzf_times()
    assert walk >= 0 and kernel > 0 and trip >= kernel
    assert ctx.bgzf_inflate(chunk, bpsw_hip.BGZF_HOST)[0] == text and bpsw_hip.last_bgzf_times() == (0.0, 0.0, 0.0)
    # trailing bytes: left alone without BGZF_FINAL, refused with it
    assert ctx.bgzf_inflate(chunk + chunk[:100]) == (text, 4, len(chunk))
    e = _refusal(ctx, chunk + chunk[:100], bpsw_hip.BGZF_FINAL)
    assert e.rc == -1 and str(e).endswith("bgzf_inflate: 100 bytes behind the last whole block (BPSW_BGZF_FINAL)")
    assert ctx.bgzf_inflate(chunk + bp.EOF_BLOCK, bpsw_hip.BGZF_FINAL) == (text, 5, len(chunk) + 28)
    # empty chunks
    assert ctx.bgzf_inflate(b"") == (b"", 0, 0) and ctx.bgzf_inflate(bp.EOF_BLOCK) == (b"", 1, 28)
    # a malformed header wins over the capacity; the inflated total at 2^31 is the limit, before anything is launched
    e = _refusal(ctx, chunk + b"BAM\1" + bytes(20), cap=0)
    assert e.rc == -1 and _block_reason(str(e)) == (4, "MAGIC")
    zeros = ic.frame(bytes(65536), ic.deflate(bytes(65536), 6))
    e = _refusal(ctx, zeros * 32768, cap=0)
    assert e.rc == -4 and str(e).endswith("bgzf_inflate: 2^31 inflated bytes or more")
    assert _refusal(ctx, chunk, 4).rc == -1


# ---- the FASTQ entries ----------------------------------------------------------------------------------------------------------------------
def virtual(chunk, u):
    """the virtual offset of inflated offset u of a chunk of whole blocks, by bgzf_members"""
    at = out = 0
    for payload, total, _ in bp.bgzf_members(chunk):
        if out + len(payload) > u:
            return at << 16 | (u - out)
        at, out = at + total, out + len(payload)
    return at << 16


def _same(got, want, what):
    assert got.n_reads == want.n_reads and got.needed == want.needed, what
    for k in ARRAYS:
        assert np.array_equal(getattr(got, k), getattr(want, k)), (what, k)


@pytest.mark.parametrize("payload", PAYLOADS)
def test_fastq_cases_bgzipped(ctx, payload):
    for name, (t1, t2, flags) in fc.CASES.items():
        want = ctx.fastq_parse(t1, t2, flags)
        z1, z2 = ic.bgzip(t1, payload, eof=True), None if t2 is None else ic.bgzip(t2, payload)
        for path in PATHS:
            got = ctx.fastq_bgzf_parse(z1, z2, flags | path)
            _same(got, want, (name, path))
            assert got.consumed[0] == virtual(z1, want.consumed[0]), (name, path)
            assert got.consumed[1] == (0 if t2 is None else virtual(z2, want.consumed[1])), (name, path)


@pytest.mark.parametrize("skip", [0, 1, 15, 16, 17, "block"])
def test_skip(ctx, skip):
    """the text begins `skip` bytes into the first block: a first record of that many bytes is what an earlier call consumed"""
    body = fc.records(np.random.default_rng(3), 40, 5, 30)
    first_block = 333
    k = first_block if skip == "block" else skip
    head = b"#" * k   # (what earlier calls consumed is not looked at again)
    z = ic.bgzip(head + body, first_block)
    want = ctx.fastq_parse(body, None, fp.FINAL)
    for path in PATHS:
        got = ctx.fastq_bgzf_parse(z, None, fp.FINAL | path, skip=(k, 0))
        _same(got, want, (skip, path))
        assert got.consumed[0] == virtual(z, k + want.consumed[0])
    with pytest.raises(bpsw_hip.FastqError, match="fastq_bgzf_parse: text 1: skip is not within the first block's bytes"):
        ctx.fastq_bgzf_parse(z, None, fp.FINAL, skip=(first_block + 1, 0))
    with pytest.raises(bpsw_hip.FastqError, match="fastq_bgzf_parse: text 1: skip is not within the first block's bytes"):
        ctx.fastq_bgzf_parse(b"", None, fp.FINAL, skip=(1, 0))


@pytest.mark.parametrize("path", PATHS)
def test_chunk_loop_by_virtual_offsets(ctx, path):
    """a file walked in chunks of three blocks: every call begins at the block the last one stopped in, skip is where it stopped"""
    text = fc.records(np.random.default_rng(21), 400, 20, 90)
    file = ic.bgzip(text, 1021, eof=True)
    sizes = [m[1] for m in bp.bgzf_members(file)]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    want = ctx.fastq_parse(text, None, fp.FINAL)
    pools, names, n, at, skip, calls = [], [], 0, 0, 0, 0
    while at < len(file):
        block = int(np.searchsorted(starts, at))
        assert starts[block] == at
        end = int(starts[min(block + 3, len(sizes))])
        final = fp.FINAL if end == len(file) else 0
        got = ctx.fastq_bgzf_parse(file[at:end], None, final | path, skip=(skip, 0))
        coff, skip = bpsw_hip.voffset(got.consumed[0])
        assert got.n_reads > 0 or final
        pools.append((got.read_len, got.read_pool, got.qual_pool, got.name_pool))
        n, at, calls = n + got.n_reads, at + coff, calls + 1
        assert calls < 1000
    assert n == want.n_reads and skip == 0 and calls > 20
    assert np.array_equal(np.concatenate([p[0] for p in pools]), want.read_len)
    for k, f in ((1, "read_pool"), (2, "qual_pool"), (3, "name_pool")):
        assert np.array_equal(np.concatenate([p[k] for p in pools]), getattr(want, f)), f


def test_two_texts_of_65_and_70_records(ctx):
    t1, t2, flags = fc.CASES["pairs_65_70"]
    want = ctx.fastq_parse(t1, t2, flags)
    assert want.n_reads == 130
    z1, z2 = ic.bgzip(t1, 500), ic.bgzip(t2, 700)
    for path in PATHS:
        got = ctx.fastq_bgzf_parse(z1, z2, flags | path)
        _same(got, want, path)
        assert got.consumed == (virtual(z1, want.consumed[0]), virtual(z2, want.consumed[1]))
        assert bpsw_hip.voffset(got.consumed[0]) == (len(z1), 0) and bpsw_hip.voffset(got.consumed[1])[0] < len(z2)


def test_an_inflate_refusal_wins_over_a_malformed_record(ctx):
    text = b"no at sign\nACGT\n+\nIIII\n" + fc.CASES["count_65"][0]
    z = ic.bgzip(text, 300)
    members = bp.bgzf_members(z)
    at = members[0][1] + members[1][1]
    broken = z[: at + members[2][1] - 8] + bytes(4) + z[at + members[2][1] - 4:]
    for path in PATHS:
        with pytest.raises(bpsw_hip.FastqError) as e:
            ctx.fastq_bgzf_parse(z, None, fp.FINAL | path)
        assert str(e.value).endswith("fastq_bgzf_parse: record 0 of text 1: the header line does not begin with '@' (not four-line FASTQ)")
        with pytest.raises(bpsw_hip.FastqError) as e:
            ctx.fastq_bgzf_parse(broken, None, fp.FINAL | path)
        assert e.value.rc == -1 and str(e.value).endswith("fastq_bgzf_parse: text 1: block 2: " + ic.REASON_TEXT["CRC"])
        with pytest.raises(bpsw_hip.FastqError) as e:
            ctx.fastq_bgzf_parse(z[:-5], None, fp.FINAL | path)
        assert str(e.value).endswith("fastq_bgzf_parse: text 1: the text ends inside a BGZF block")
        plain = next(c for c in ic.cases() if c.name == "header_plain_gzip").chunk
        with pytest.raises(bpsw_hip.FastqError) as e:
            ctx.fastq_bgzf_parse(z, plain, fp.FINAL | path)
        assert str(e.value).endswith("fastq_bgzf_parse: text 2: block 0: " + ic.REASON_TEXT["NO_BC"])


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------
def test_fastq_bgzf_to_sam_and_bam_single_end(ctx, gold, fixture_reads):
    g, idx, reads, quals, _ = fixture_reads
    opt, so, topt = bpsw_hip.default_opt(), _opt(gold, "c1"), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    _load(ctx, gold["g1_pac"], g.size, _contig_tables(g.size)[1], idx)
    text = _fastq_of(reads, quals, [b"frag%d" % i for i in range(len(reads))])
    z = ic.bgzip(text, 1021, eof=True)
    kw = dict(id0=1000, id_step=2, zdrop_mode=bpsw_hip.ZDROP_BWA)
    want, consumed = ctx.align_fastq_se(opt, so, topt, text, fp.FINAL, **kw)
    assert len(want) == 105 and consumed == len(text)
    for path in PATHS:
        got, v = ctx.align_fastq_bgzf_se(opt, so, topt, z, 0, fp.FINAL | path, **kw)
        assert got == want and bpsw_hip.voffset(v) == (len(z), 0), path
    for flags in (0, bpsw_hip.BAM_DEFLATE):
        want_bam, n, consumed = ctx.align_fastq_bam_se(opt, so, topt, text, fp.FINAL, flags=flags, **kw)
        for path in PATHS:
            got, n2, v = ctx.align_fastq_bgzf_bam_se(opt, so, topt, z, 0, fp.FINAL | path, flags=flags, **kw)
            assert got == want_bam and n2 == n == 105 and bpsw_hip.voffset(v) == (len(z), 0), (flags, path)
    # round trip: what BPSW_BAM_DEFLATE wrote, read back on the device
    data, n_blocks, used = ctx.bgzf_inflate(want_bam, bpsw_hip.BGZF_FINAL)
    assert data == bp.bgzf_inflate(want_bam) and used == len(want_bam) and n_blocks == len(bp.bgzf_members(want_bam))
    assert want_bam[18] & 7 == 5


def test_fastq_bgzf_to_sam_and_bam_pairs(ctx, gold, fixture_reads):
    g, idx, reads, quals, _ = fixture_reads
    opt, so, topt = bpsw_hip.default_opt(), _opt(gold, "c1"), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    _load(ctx, gold["g1_pac"], g.size, _contig_tables(g.size)[1], idx)
    first, second = PAIR_ORDER[0::2], PAIR_ORDER[1::2]
    assert len(first) == 52
    t1 = _fastq_of([reads[i] for i in first], [quals[i] for i in first], [b"pair%d/1" % k for k in range(52)])
    t2 = _fastq_of([reads[i] for i in second], [quals[i] for i in second], [b"pair%d/2" % k for k in range(52)])
    z1, z2 = ic.bgzip(t1, 1021), ic.bgzip(t2, 64)
    kw = dict(id0=500, zdrop_mode=bpsw_hip.ZDROP_BWA)
    want, want_pes, consumed = ctx.align_fastq_pe(opt, so, topt, t1, t2, fp.FINAL, **kw)
    assert len(want) == 104 and consumed == (len(t1), len(t2))
    for path in PATHS:
        got, pes, v = ctx.align_fastq_bgzf_pe(opt, so, topt, z1, z2, (0, 0), fp.FINAL | path, **kw)
        assert got == want and pes == want_pes and v == (len(z1) << 16, len(z2) << 16), path
    for flags in (0, bpsw_hip.BAM_DEFLATE):
        want_bam, _, n, _ = ctx.align_fastq_bam_pe(opt, so, topt, t1, t2, fp.FINAL, flags=flags, **kw)
        for path in PATHS:
            got, pes, n2, v = ctx.align_fastq_bgzf_bam_pe(opt, so, topt, z1, z2, (0, 0), fp.FINAL | path, flags=flags, **kw)
            assert got == want_bam and n2 == n == 104 and v == (len(z1) << 16, len(z2) << 16), (flags, path)
    assert ctx.bgzf_inflate(want_bam)[0] == bp.bgzf_inflate(want_bam)
