"""Alignments out as BAM: bpsw_bam_se_batch / bpsw_bam_pe_batch, bpsw_align_bam_*_batch and bpsw_align_fastq_bam_* (csrc/bpsw_bam.hip:
bam_len_kernel, bam_write_kernel, bgzf_frame_kernel over csrc/bpsw_bam_core.h).

Every case decodes the output with the BGZF reader of tests/bam_plain.py -- which walks the members by BSIZE, inflates each with zlib
and checks CRC32 and ISIZE with zlib.crc32, so a wrong frame, CRC or size fails there -- checks that every member is one stored block
of the payload size in force and that the call's size is the closed form S + 31 ceil(S / P), and then compares the inflated stream
byte for byte with bam_plain.sam_to_bam applied to the text the SAM twin entry returns for the same input (BPSW_SAM_TEXT_DEVICE).
The fixtures and helpers are those of test_sam_se_gpu.py / test_sam_pe_gpu.py."""
import copy
import ctypes as C

import numpy as np
import pytest

import bam_plain as bp
import bpsw_hip
from bpsw_hip import fmi
from tail_util import load_sam_pe_golden
from test_sam_pe_gpu import ALL, FLAGS3, NO_MULTI, PAIR_ORDER, PES_FR, _group_of, _paired_fixture, _ready, own_regions  # noqa: F401
from test_sam_se_gpu import NO_PES, _lines, _se, fixture_reads, gold  # noqa: F401
from test_worker1_gpu import _opt

pytestmark = pytest.mark.gpu

DEV = bpsw_hip.SAM_TEXT_DEVICE
P0 = 65280
FLAVOURS = [bpsw_hip.TAIL_SCALA, bpsw_hip.TAIL_C]


class payload:
    """the BGZF payload size for the calls inside, the default again behind them"""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        assert bpsw_hip.bam_set_block_payload(self.n) == 0
        return self.n or P0

    def __exit__(self, *a):
        assert bpsw_hip.bam_set_block_payload(0) == 0


def _ref_id(names, n=None):
    return {(s.encode() if s else b"ctg%d" % (k + 1)): k for k, s in enumerate(names if names is not None else [""] * n)}


def _records_of(texts, ref_id):
    return [bp.sam_to_bam(line, ref_id) for t in texts for line in t.split(b"\n")[:-1]]


def _check(bam, texts, ref_id, p=P0):
    """the framing of `bam` and its stream against the text -> (the stream, the members)"""
    want = b"".join(_records_of(texts, ref_id))
    members = bp.bgzf_members(bam)
    blocks = -(-len(want) // p)
    assert len(bam) == len(want) + 31 * blocks                                   # the closed form
    assert [len(m[0]) for m in members] == [p] * (len(want) // p) + ([len(want) % p] if len(want) % p else [])
    assert all(m[1] == len(m[0]) + 31 and m[2][0] == 1 for m in members)         # one stored block each, 31 bytes around the payload
    got = b"".join(m[0] for m in members)
    if got != want:
        a, b = bp.split_records(got), bp.split_records(want)
        bad = [i for i in range(min(len(a), len(b))) if a[i] != b[i]]
        raise AssertionError((len(a), len(b), bad[:3], a[bad[0]].hex() if bad else None, b[bad[0]].hex() if bad else None))
    return got, members


def _pe_both(ctx, opt, topt, g, ref_id, p=P0):
    text, regs_t = ctx.sam_pe_batch(opt, topt, g, flags=DEV)
    bam, regs_b = ctx.bam_pe_batch(opt, topt, g)
    assert regs_t.tobytes() == regs_b.tobytes()
    return _check(bam, text, ref_id, p)[0], text


def _se_both(ctx, opt, topt, g, ref_id, p=P0):
    text, regs_t = ctx.sam_se_batch(opt, topt, g, flags=DEV)
    bam, regs_b = ctx.bam_se_batch(opt, topt, g)
    assert regs_t.tobytes() == regs_b.tobytes()
    return _check(bam, text, ref_id, p)[0], text


# ---- 1. the goldens and the fixture pairs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("stem", ["mem_sam_pe", "mem_sam_pe_all", "mem_sam_pe_rg"])
def test_bam_pe_goldens(ctx, stem, flavour):
    pac, g, flag, _ = load_sam_pe_golden(stem)
    ctx.ref_load(pac, g.l_pac)
    names = [bytes(g.ann_name_pool[int(g.ann_name_off[i]):int(g.ann_name_off[i + 1])]).decode() for i in range(g.ann_off.shape[0])]
    ctx.bns_load(g.ann_off, g.ann_len, names)
    opt = bpsw_hip.default_opt()
    opt.flag = flag
    topt = bpsw_hip.default_tail_opt(flavour)
    topt.rg_id = g.rg_id
    stream, text = _pe_both(ctx, opt, topt, g, _ref_id(names))
    assert len(bp.split_records(stream)) == sum(t.count(b"\n") for t in text) >= 2 * g.group_size
    t = bpsw_hip.last_bam_times()
    assert t[0] > 0 and t[1] > 0 and t[2] > 0 and all(x >= 0 for x in t)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_bam_fixture_pairs_and_single_ends(ctx, gold, fixture_reads, own_regions, flavour):
    """the 52 fixture pairs (supplementary lines, unmapped mates, both-unmapped pairs, reverse strands; secondaries with l_seq == 0 under
    MEM_F_ALL; MEM_F_NO_MULTI, where the flavours differ) as pairs and as single ends, RG on and off"""
    table = _ready(ctx, gold, fixture_reads)
    ids = _ref_id(table[2])
    for flag, rg, pes in ((0, b"", NO_PES), (ALL, b"run12.lane3", PES_FR), (ALL | NO_MULTI, b"", NO_PES), (NO_MULTI, b"g", NO_PES)):
        opt, topt = bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(flavour)
        opt.flag = flag
        topt.rg_id = rg
        stream, text = _pe_both(ctx, opt, topt, _paired_fixture(fixture_reads, *own_regions, table, pes), ids)
        f = _lines(text)
        if flag == 0:
            assert sum(any(x.startswith(b"SA:Z:") for x in l) for l in f) >= 4 and sum(int(l[1]) & 0xc == 0xc for l in f) >= 2, "the input degenerated"
            assert sum(bool(int(l[1]) & 0x10) for l in f) >= 20 and sum(bool(int(l[1]) & 0x800) for l in f) >= 2
        if flag & ALL:
            assert sum(l[9] == b"*" for l in f) >= 100                           # l_seq == 0
        assert all((b"RGZ" + rg + b"\0" in r) == bool(rg) for r in bp.split_records(stream))
        _se_both(ctx, opt, topt, _se(fixture_reads, *own_regions), ids)


# ---- 2. record counts around a wavefront, and the hundred-line read ---------------------------------------------------------------------------
def test_bam_record_counts_around_a_wavefront(ctx, gold, fixture_reads, own_regions):
    table = _ready(ctx, gold, fixture_reads)
    ids = _ref_id(table[2])
    opt, topt = bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    text, _ = ctx.sam_se_batch(opt, topt, _se(fixture_reads, *own_regions), flags=DEV)
    one = [i for i, t in enumerate(text) if t.count(b"\n") == 1]
    assert len(one) >= 60
    for n in (0, 1, 63, 64, 65, 129):
        stream, _ = _se_both(ctx, opt, topt, _se(fixture_reads, *own_regions, which=[one[k % len(one)] for k in range(n)]), ids)
        assert len(bp.split_records(stream)) == n
    st, keep, _ = bpsw_hip._se_struct(_se(fixture_reads, *own_regions, which=[]), True)   # no read: no block, nothing needed
    need = C.c_size_t(99)
    assert ctx.lib.bpsw_bam_se_batch(ctx.h, C.byref(opt), C.byref(topt), C.byref(st), 0, None, 0, C.byref(need), None) == 0 and need.value == 0


def test_bam_of_the_pair_with_a_hundred_lines(ctx, gold, fixture_reads, own_regions):
    table = _ready(ctx, gold, fixture_reads)
    opt = bpsw_hip.default_opt()
    opt.flag = ALL
    text, _ = ctx.sam_pe_batch(opt, bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C), _paired_fixture(fixture_reads, *own_regions, table, NO_PES), flags=DEV)
    big = int(np.argmax([t.count(b"\n") for t in text]))
    pair = [PAIR_ORDER[big & ~1], PAIR_ORDER[big | 1]]
    for flavour in FLAVOURS:
        for o, flag in ((pair, ALL), ([0, 1, 3, 5] + pair[::-1], ALL | NO_MULTI), (pair, 0)):
            opt.flag = flag
            stream, t = _pe_both(ctx, opt, bpsw_hip.default_tail_opt(flavour), _paired_fixture(fixture_reads, *own_regions, table, NO_PES, order=o),
                                 _ref_id(table[2]))
            assert flag == 0 or max(x.count(b"\n") for x in t) >= 101
            # (its lines are secondaries, which no SA list names: the SA list of a hundred lines is tests/bam_host's)


# ---- 3. block edges -------------------------------------------------------------------------------------------------------------------------------
def _parts(rec):
    """the parts of a record as (name, begin, end) offsets"""
    import struct
    l_name, n_cig, l_seq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<I", rec, 20)[0]
    at = [0, 36, 36 + l_name, 36 + l_name + 4 * n_cig, 36 + l_name + 4 * n_cig + (l_seq + 1) // 2]
    at += [at[-1] + l_seq, len(rec)]
    return list(zip(("fixed", "name", "cigar", "seq", "qual", "tag"), at[:-1], at[1:]))


def test_bam_block_edges_inside_every_part_of_a_record(ctx, gold, fixture_reads, own_regions):
    table = _ready(ctx, gold, fixture_reads)
    opt, topt = bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    opt.flag = ALL
    g = _paired_fixture(fixture_reads, *own_regions, table, PES_FR)
    hit = set()
    for p in (64, 256, 1021):
        with payload(p):
            stream, _ = _pe_both(ctx, opt, topt, g, _ref_id(table[2]), p)
        recs, at = bp.split_records(stream), 0
        cuts = set(range(p, len(stream), p))
        for r in recs:
            for name, b, e in _parts(r):
                if any(c in cuts for c in range(at + b + 1, at + e)):   # strictly inside the part
                    hit.add(name)
            at += len(r)
    assert hit == {"fixed", "name", "cigar", "seq", "qual", "tag"}, hit


@pytest.mark.parametrize("total,blocks", [(65279, 1), (65280, 1), (65281, 2)])
def test_bam_stream_of_one_block_more_or_less_a_byte(ctx, gold, fixture_reads, own_regions, total, blocks):
    """at the default payload a stream of 65 279, 65 280 and 65 281 bytes: a block a byte short, a full block, a full block and one of
    one byte.  The reads are the fixture's with one-byte names, as many as stay below the target; the names of single-line reads are
    then lengthened (a name's bytes enter the stream once per line of its read) until bam_plain counts the target."""
    table = _ready(ctx, gold, fixture_reads)
    ids = _ref_id(table[2])
    opt, topt = bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    n_reads = len(fixture_reads[2])
    text, _ = ctx.sam_se_batch(opt, topt, _se(fixture_reads, *own_regions, names=[b"n"] * n_reads), flags=DEV)
    size = [sum(len(r) for r in _records_of([t], ids)) for t in text]
    which, s = [], 0
    for k in range(4 * n_reads):   # (a read's lines may change with its place in the batch, which it is hashed by: leave room)
        if s + size[k % n_reads] > total - 1000:
            break
        which.append(k % n_reads)
        s += size[k % n_reads]
    text, _ = ctx.sam_se_batch(opt, topt, _se(fixture_reads, *own_regions, which=which, names=[b"n"] * len(which)), flags=DEV)
    left = total - sum(len(r) for r in _records_of(text, ids))
    assert 0 < left < 2000
    names = []
    for t in text:
        add = min(left, 253) if t.count(b"\n") == 1 else 0
        names.append(b"n" * (1 + add))
        left -= add
    assert left == 0
    with payload(0):
        stream, _ = _se_both(ctx, opt, topt, _se(fixture_reads, *own_regions, which=which, names=names), ids)
    assert len(stream) == total
    bam, _ = ctx.bam_se_batch(opt, topt, _se(fixture_reads, *own_regions, which=which, names=names))
    assert [len(m[0]) for m in bp.bgzf_members(bam)] == ([total] if blocks == 1 else [65280, 1]) and len(bam) == total + 31 * blocks


# ---- 4. fields ---------------------------------------------------------------------------------------------------------------------------------------
def test_bam_read_lengths_qualities_and_contig_names(ctx, gold, fixture_reads):
    """reads of 1, 2, 133 (odd) and 251 bases on both strands, with and without qualities, with and without contig names"""
    g = fixture_reads[0]
    for with_names in (True, False):
        table = _ready(ctx, gold, fixture_reads, names=with_names)
        ids = _ref_id(table[2] if with_names else None, len(table[2]))
        opt, so = bpsw_hip.default_opt(), _opt(gold, "c1")
        reads = [g[77:78], g[5000:5251], g[90:92], (3 - g[6000:6133][::-1]).astype(np.uint8), g[300:433], (3 - g[7000:7251][::-1]).astype(np.uint8)]
        cnt, regs = ctx.worker1_batch(opt, so, fmi.ReadBatch.from_list(reads), zdrop_mode=bpsw_hip.ZDROP_BWA, flags=bpsw_hip.C2A_SORT_DEDUP)
        assert cnt[0] == 0 and all(cnt[i] >= 1 for i in (1, 3, 4, 5))
        at = np.concatenate([[0], np.cumsum(cnt)])
        rng = np.random.default_rng(9)
        quals = [rng.integers(33, 127, len(r)).astype(np.uint8) for r in reads]
        for flavour in FLAVOURS:
            for with_quals in (True, False):
                topt = bpsw_hip.default_tail_opt(flavour)
                grp = _group_of(g.size, reads, quals, [b"q", b"n" * 254, b"mid"], cnt, [regs[at[i]:at[i + 1]] for i in range(6)], table, PES_FR, id0=5,
                                with_quals=with_quals)
                stream, text = _pe_both(ctx, opt, topt, grp, ids)
                f = _lines(text)
                assert sorted({len(l[9]) for l in f}) == [1, 2, 133, 251] and any(int(l[1]) & 0x10 for l in f)
                assert all((l[10] == b"*") == (not with_quals) for l in f) and (with_names or any(l[2] in (b"ctg1", b"ctg2") for l in f))
                se = bpsw_hip.SeReadsSoA.from_lists(reads, [b"a", b"b" * 254, b"c", b"d", b"e", b"f"], quals if with_quals else None, reg_cnt=cnt, regs=regs)
                _se_both(ctx, opt, topt, se, ids)


# ---- 5. capacity and refusals ---------------------------------------------------------------------------------------------------------------------------
def test_bam_capacity_and_refusals(ctx, gold, fixture_reads, own_regions):
    table = _ready(ctx, gold, fixture_reads)
    opt, topt = bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    g = _paired_fixture(fixture_reads, *own_regions, table, NO_PES)
    with payload(1021) as p:
        stream, text = _pe_both(ctx, opt, topt, g, _ref_id(table[2]), p)
        whole, _ = ctx.bam_pe_batch(opt, topt, g)
        st, keep, regs = bpsw_hip._pairs_struct(g)
        need = C.c_size_t(0)
        call = lambda flags, buf, cap: ctx.lib.bpsw_bam_pe_batch(ctx.h, C.byref(opt), C.byref(topt), C.byref(st), flags, bpsw_hip._ptr(buf), cap,
                                                                 C.byref(need), None)
        for cap in (0, 1, len(whole) - 1):
            buf = np.full(len(whole) + 64, 0xAB, np.uint8)
            need.value = 0
            assert call(0, buf, cap) == -3 and need.value == len(whole) == len(stream) + 31 * -(-len(stream) // p)
            assert (buf == 0xAB).all()                                           # nothing is written, not even below the capacity
        buf = np.full(len(whole) + 64, 0xAB, np.uint8)
        assert call(0, buf, need.value) == 0 and buf[: len(whole)].tobytes() == whole and (buf[len(whole):] == 0xAB).all()
        for unknown in (DEV, 2, -2):                                             # BAM is no flag, and no flag is known here
            assert call(unknown, buf, len(buf)) == -1
    # a name of 255 bytes cannot be a record; 254 can
    se = lambda n: _se(fixture_reads, *own_regions, which=[0, 1, 2], names=[b"a", b"b" * n, b"c"])
    _se_both(ctx, opt, topt, se(254), _ref_id(table[2]))
    buf = np.full(4096, 0xAB, np.uint8)
    st, keep, _ = bpsw_hip._se_struct(se(255), True)
    need = C.c_size_t(0)
    assert ctx.lib.bpsw_bam_se_batch(ctx.h, C.byref(opt), C.byref(topt), C.byref(st), 0, bpsw_hip._ptr(buf), len(buf), C.byref(need), None) == -4
    assert (buf == 0xAB).all() and b"254" in ctx.lib.bpsw_last_error()
    grp = _paired_fixture(fixture_reads, *own_regions, table, NO_PES, order=[0, 1, 2, 3], names=[b"x" * 255, b"y"])
    with pytest.raises(bpsw_hip.BpswError, match=r"\(-4\)"):
        ctx.bam_pe_batch(opt, topt, grp)
    # the setter: 0 is the default, 65 280 the most, 65 281 refused and without effect
    assert bpsw_hip.bam_set_block_payload(65280) == 0 and bpsw_hip.bam_set_block_payload(0) == 0
    assert bpsw_hip.bam_set_block_payload(300) == 0 and bpsw_hip.bam_set_block_payload(65281) == -1 and bpsw_hip.bam_set_block_payload(-5) == -1
    try:
        bam, _ = ctx.bam_se_batch(opt, topt, se(3))
        assert max(len(m[0]) for m in bp.bgzf_members(bam)) == 300
    finally:
        assert bpsw_hip.bam_set_block_payload(0) == 0


# ---- 6. reads and FASTQ text to BAM ------------------------------------------------------------------------------------------------------------------------
def _fastq(names, reads, quals):
    return b"".join(b"@" + n + b"\n" + bytes(b"ACGTN"[c] for c in r) + b"\n+\n" + bytes(q) + b"\n" for n, r, q in zip(names, reads, quals))


def test_align_bam_entries_against_their_sam_twins(ctx, gold, fixture_reads):
    g, idx, reads, quals, names = fixture_reads
    table = _ready(ctx, gold, fixture_reads)
    ids = _ref_id(table[2])
    opt, so, topt = bpsw_hip.default_opt(), _opt(gold, "c1"), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    none = np.zeros(0, bpsw_hip.ALNREG_DTYPE)
    order = PAIR_ORDER[:40]
    bare = _group_of(g.size, [reads[i] for i in order], [quals[i] for i in order], [b"pair%d" % k for k in range(20)], [0] * 40, [none] * 40, table, NO_PES)
    bare.reg_cnt, bare.regs = None, None
    for w1 in (0, bpsw_hip.W1_CHAIN_DEVICE):
        text, pes = ctx.align_pe_batch(opt, so, topt, bare, zdrop_mode=bpsw_hip.ZDROP_BWA, w1_flags=w1, flags=DEV)
        bam, pes_b = ctx.align_bam_pe_batch(opt, so, topt, bare, zdrop_mode=bpsw_hip.ZDROP_BWA, w1_flags=w1)
        assert pes == pes_b
        _check(bam, text, ids)
    se = bpsw_hip.SeReadsSoA.from_lists([reads[i] for i in order], [names[i] for i in order], [quals[i] for i in order])
    text = ctx.align_se_batch(opt, so, topt, se, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=DEV)
    _check(ctx.align_bam_se_batch(opt, so, topt, se, zdrop_mode=bpsw_hip.ZDROP_BWA), text, ids)
    with pytest.raises(bpsw_hip.BpswError, match=r"\(-1\)"):
        ctx.align_bam_se_batch(opt, so, topt, se, flags=DEV)
    with pytest.raises(bpsw_hip.BpswError, match=r"\(-1\)"):
        ctx.align_bam_pe_batch(opt, so, topt, bare, flags=2)
    # FASTQ text: single ends, and pairs from two texts
    fq = _fastq([b"r%d" % i for i in order], [reads[i] for i in order], [quals[i] for i in order])
    text, consumed = ctx.align_fastq_se(opt, so, topt, fq, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=DEV)
    bam, n, consumed_b = ctx.align_fastq_bam_se(opt, so, topt, fq, zdrop_mode=bpsw_hip.ZDROP_BWA)
    assert n == len(order) == len(text) and consumed == consumed_b == len(fq)
    _check(bam, text, ids)
    pn = [b"p%d" % k for k in range(20)]
    fq1 = _fastq(pn, [reads[i] for i in order[0::2]], [quals[i] for i in order[0::2]])
    fq2 = _fastq(pn, [reads[i] for i in order[1::2]], [quals[i] for i in order[1::2]])
    text, pes, consumed = ctx.align_fastq_pe(opt, so, topt, fq1, fq2, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=DEV)
    bam, pes_b, n, consumed_b = ctx.align_fastq_bam_pe(opt, so, topt, fq1, fq2, zdrop_mode=bpsw_hip.ZDROP_BWA)
    assert n == 40 == len(text) and pes == pes_b and consumed == consumed_b == (len(fq1), len(fq2))
    _check(bam, text, ids)
    with pytest.raises(bpsw_hip.BpswError, match=r"\(-1\)"):
        ctx.align_fastq_bam_se(opt, so, topt, fq, flags=DEV)


# ---- 7. a whole file ---------------------------------------------------------------------------------------------------------------------------------------------
def test_bam_file_of_a_header_two_calls_and_the_end(ctx, gold, fixture_reads, own_regions):
    table = _ready(ctx, gold, fixture_reads)
    ids = _ref_id(table[2])
    opt, topt = bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    topt.rg_id = b"g1"
    extra = b"@RG\tID:g1\tSM:s\n"
    first = _paired_fixture(fixture_reads, *own_regions, table, NO_PES, order=PAIR_ORDER[:60])
    second = _paired_fixture(fixture_reads, *own_regions, table, NO_PES, order=PAIR_ORDER[60:])
    with payload(4096) as p:
        parts = [ctx.bam_header(extra), ctx.bam_pe_batch(opt, topt, first)[0], ctx.bam_pe_batch(opt, topt, second)[0], ctx.bam_eof()]
    data = b"".join(parts)
    members = bp.bgzf_members(data)
    assert members[-1][0] == b"" and data.endswith(bp.EOF_BLOCK)
    stream = b"".join(m[0] for m in members)
    text, refs, at = bp.parse_bam_header(stream)
    assert text == ctx.sam_header(extra) == bp.sam_header_text(table[2], table[1], extra)
    assert refs == [(n.encode(), l) for n, l in zip(table[2], table[1])]
    want = [ctx.sam_pe_batch(opt, topt, g, flags=DEV)[0] for g in (first, second)]
    assert stream[at:] == b"".join(_records_of(want[0] + want[1], ids))
    on, checked, faults = ctx.ring_integrity()
    assert faults == 0
