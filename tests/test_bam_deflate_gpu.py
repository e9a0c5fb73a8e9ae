"""BPSW_BAM_DEFLATE on the device: every BGZF block of the six BAM entries as one dynamic-Huffman deflate block with LZ77 matches
(bgzf_deflate_kernel, bgzf_pack_kernel; csrc/bpsw_deflate_core.h).

The yardsticks: the same call without the flag (its inflated stream must be the flagged call's), tests/bam_plain.bgzf_members (BSIZE,
CRC-32, ISIZE and the end of every member's deflate stream, inflated by zlib), and the host twin of the kernel -- the program of
tests/test_deflate_core_host.py built without the sanitizer and fed the inflated stream and P -- whose bytes the device's must EQUAL:
that identity, on the golden pairs and the fixture's single ends at five payload sizes, is the kernel's parity test."""
import ctypes as C

import numpy as np
import pytest

import bam_plain as bp
import bpsw_hip
from tail_util import load_sam_pe_golden
from test_bam_gpu import DEV, P0, _fastq, _records_of, _ref_id, payload
from test_deflate_core_host import build_host, run_host
from test_sam_pe_gpu import NO_MULTI, PAIR_ORDER, PES_FR, _group_of, _paired_fixture, _ready, own_regions  # noqa: F401
from test_sam_se_gpu import NO_PES, _se, fixture_reads, gold  # noqa: F401
from test_worker1_gpu import _opt

pytestmark = pytest.mark.gpu

Z = bpsw_hip.BAM_DEFLATE
SIZES = [64, 256, 1021, 4096, 0]


@pytest.fixture(scope="module")
def twin():
    return build_host(False)


def _both(call, p):
    """call(flags) -> bytes, with and without the flag -> (flagged, stream); the members of both are checked and hold the same payloads"""
    plain, packed = call(0), call(Z)
    a, b = bp.bgzf_members(plain), bp.bgzf_members(packed)
    assert [m[0] for m in a] == [m[0] for m in b]
    assert all(len(m[0]) == p for m in b[:-1]) and all(0 < len(m[0]) <= p for m in b[-1:])
    for pay, total, cdata in b:
        assert cdata[0] & 7 in (1, 5) and total <= len(pay) + 31 and (total == len(pay) + 31) == (cdata[0] & 7 == 1)
    assert len(packed) <= len(plain)
    return packed, b"".join(m[0] for m in a)


def test_golden_pairs_equal_the_host_twin_at_five_payload_sizes(ctx, twin):
    got, cases = [], []
    for stem in ("mem_sam_pe", "mem_sam_pe_all", "mem_sam_pe_rg"):
        pac, g, flag, _ = load_sam_pe_golden(stem)
        ctx.ref_load(pac, g.l_pac)
        names = [bytes(g.ann_name_pool[int(g.ann_name_off[i]):int(g.ann_name_off[i + 1])]).decode() for i in range(g.ann_off.shape[0])]
        ctx.bns_load(g.ann_off, g.ann_len, names)
        opt, topt = bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
        opt.flag, topt.rg_id = flag, g.rg_id
        for size in SIZES:
            with payload(size) as p:
                packed, stream = _both(lambda f: ctx.bam_pe_batch(opt, topt, g, flags=f)[0], p)
            got.append(packed)
            cases.append((p, stream))
            if p == P0:
                assert packed[18] & 7 == 5 and len(packed) < 0.75 * len(stream)   # (0.69 on the host; a Huffman table alone gives 0.76)
    assert run_host(twin, cases, "gpu_golden") == got


def test_single_ends_and_record_counts_around_a_wavefront(ctx, twin, gold, fixture_reads, own_regions):
    table = _ready(ctx, gold, fixture_reads)
    ids = _ref_id(table[2])
    opt, topt = bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    got, cases = [], []
    g = _se(fixture_reads, *own_regions)
    text, _ = ctx.sam_se_batch(opt, topt, g, flags=DEV)
    for size in SIZES:
        with payload(size) as p:
            packed, stream = _both(lambda f: ctx.bam_se_batch(opt, topt, g, flags=f)[0], p)
        assert stream == b"".join(_records_of(text, ids))
        got.append(packed)
        cases.append((p, stream))
    one = [i for i, t in enumerate(text) if t.count(b"\n") == 1]
    for n in (0, 1, 63, 64, 65, 129):
        few = _se(fixture_reads, *own_regions, which=[one[k % len(one)] for k in range(n)])
        for size in (256, 0):
            with payload(size) as p:
                packed, stream = _both(lambda f: ctx.bam_se_batch(opt, topt, few, flags=f)[0], p)
            assert len(bp.split_records(stream)) == n and (n > 0 or packed == b"")
            got.append(packed)
            cases.append((p, stream))
    assert run_host(twin, cases, "gpu_se") == got


def test_capacity_is_the_compressed_size(ctx, gold, fixture_reads, own_regions):
    table = _ready(ctx, gold, fixture_reads)
    opt, topt = bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    g = _paired_fixture(fixture_reads, *own_regions, table, NO_PES)
    with payload(4096):
        whole, _ = ctx.bam_pe_batch(opt, topt, g, flags=Z)
        stored, _ = ctx.bam_pe_batch(opt, topt, g)
        st, keep, regs = bpsw_hip._pairs_struct(g)
        need = C.c_size_t(0)
        call = lambda flags, buf, cap: ctx.lib.bpsw_bam_pe_batch(ctx.h, C.byref(opt), C.byref(topt), C.byref(st), flags, bpsw_hip._ptr(buf), cap,
                                                                 C.byref(need), None)
        assert len(whole) < len(stored)
        for cap in (0, 1, len(whole) - 1):
            buf = np.full(len(stored) + 64, 0xAB, np.uint8)
            need.value = 0
            assert call(Z, buf, cap) == -3 and need.value == len(whole)
            assert (buf == 0xAB).all()                                           # nothing is written, not even below the capacity
        assert ctx.lib.bpsw_bam_pe_batch(ctx.h, C.byref(opt), C.byref(topt), C.byref(st), Z, None, 1 << 30, C.byref(need), None) == -3
        assert need.value == len(whole)
        buf = np.full(len(stored) + 64, 0xAB, np.uint8)
        assert call(Z, buf, need.value) == 0 and buf[: len(whole)].tobytes() == whole and (buf[len(whole):] == 0xAB).all()
        need.value = 0
        assert call(0, buf, 0) == -3 and need.value == len(stored) >= len(whole)   # the bound a caller sizes by without a first call
        assert call(Z, buf, len(stored)) == 0 and buf[: len(whole)].tobytes() == whole


def test_flags_other_than_the_one_are_refused_by_all_six_entries(ctx, gold, fixture_reads, own_regions):
    g0, idx, reads, quals, names = fixture_reads
    table = _ready(ctx, gold, fixture_reads)
    opt, so, topt = bpsw_hip.default_opt(), _opt(gold, "c1"), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    order = PAIR_ORDER[:4]
    none = np.zeros(0, bpsw_hip.ALNREG_DTYPE)
    bare = _group_of(g0.size, [reads[i] for i in order], [quals[i] for i in order], [b"pair%d" % k for k in range(2)], [0] * 4, [none] * 4, table, NO_PES)
    bare.reg_cnt, bare.regs = None, None
    se_bare = bpsw_hip.SeReadsSoA.from_lists([reads[i] for i in order], [names[i] for i in order], [quals[i] for i in order])
    fq = _fastq([b"r%d" % i for i in order], [reads[i] for i in order], [quals[i] for i in order])
    pn = [b"p0", b"p1"]
    fq1 = _fastq(pn, [reads[i] for i in order[0::2]], [quals[i] for i in order[0::2]])
    fq2 = _fastq(pn, [reads[i] for i in order[1::2]], [quals[i] for i in order[1::2]])
    pairs = _paired_fixture(fixture_reads, *own_regions, table, NO_PES, order=order)
    ends = _se(fixture_reads, *own_regions, which=[0, 1, 2])
    bwa = bpsw_hip.ZDROP_BWA
    entries = [lambda f: ctx.bam_pe_batch(opt, topt, pairs, flags=f)[0],
               lambda f: ctx.bam_se_batch(opt, topt, ends, flags=f)[0],
               lambda f: ctx.align_bam_pe_batch(opt, so, topt, bare, zdrop_mode=bwa, flags=f)[0],
               lambda f: ctx.align_bam_se_batch(opt, so, topt, se_bare, zdrop_mode=bwa, flags=f),
               lambda f: ctx.align_fastq_bam_pe(opt, so, topt, fq1, fq2, zdrop_mode=bwa, flags=f)[0],
               lambda f: ctx.align_fastq_bam_se(opt, so, topt, fq, zdrop_mode=bwa, flags=f)[0]]
    for entry in entries:
        for unknown in (1, 2, -2, 16 | 1):
            with pytest.raises(bpsw_hip.BpswError, match=r"\(-1\)"):
                entry(unknown)
        assert bp.bgzf_inflate(entry(16)) == bp.bgzf_inflate(entry(0)) != b""


def test_align_and_fastq_entries_against_their_flagless_twins(ctx, gold, fixture_reads):
    g, idx, reads, quals, names = fixture_reads
    table = _ready(ctx, gold, fixture_reads)
    opt, so, topt = bpsw_hip.default_opt(), _opt(gold, "c1"), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    none = np.zeros(0, bpsw_hip.ALNREG_DTYPE)
    order = PAIR_ORDER[:40]
    bare = _group_of(g.size, [reads[i] for i in order], [quals[i] for i in order], [b"pair%d" % k for k in range(20)], [0] * 40, [none] * 40, table, NO_PES)
    bare.reg_cnt, bare.regs = None, None
    se = bpsw_hip.SeReadsSoA.from_lists([reads[i] for i in order], [names[i] for i in order], [quals[i] for i in order])
    fq = _fastq([b"r%d" % i for i in order], [reads[i] for i in order], [quals[i] for i in order])
    pn = [b"p%d" % k for k in range(20)]
    fq1 = _fastq(pn, [reads[i] for i in order[0::2]], [quals[i] for i in order[0::2]])
    fq2 = _fastq(pn, [reads[i] for i in order[1::2]], [quals[i] for i in order[1::2]])
    bwa = bpsw_hip.ZDROP_BWA
    with payload(4096) as p:
        for call in (lambda f: ctx.align_bam_pe_batch(opt, so, topt, bare, zdrop_mode=bwa, flags=f)[0],
                     lambda f: ctx.align_bam_se_batch(opt, so, topt, se, zdrop_mode=bwa, flags=f),
                     lambda f: ctx.align_fastq_bam_pe(opt, so, topt, fq1, fq2, zdrop_mode=bwa, flags=f)[0],
                     lambda f: ctx.align_fastq_bam_se(opt, so, topt, fq, zdrop_mode=bwa, flags=f)[0]):
            packed, stream = _both(call, p)
            assert len(bp.split_records(stream)) >= 40 and len(packed) < len(stream)


def test_a_file_of_a_header_a_stored_call_a_compressed_call_and_the_end(ctx, gold, fixture_reads, own_regions):
    table = _ready(ctx, gold, fixture_reads)
    ids = _ref_id(table[2])
    opt, topt = bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    topt.rg_id = b"g1"
    extra = b"@RG\tID:g1\tSM:s\n"
    first = _paired_fixture(fixture_reads, *own_regions, table, NO_PES, order=PAIR_ORDER[:60])
    second = _paired_fixture(fixture_reads, *own_regions, table, NO_PES, order=PAIR_ORDER[60:])
    with payload(4096):
        parts = [ctx.bam_header(extra), ctx.bam_pe_batch(opt, topt, first)[0], ctx.bam_pe_batch(opt, topt, second, flags=Z)[0], ctx.bam_eof()]
    data = b"".join(parts)
    members = bp.bgzf_members(data)
    assert members[-1][0] == b"" and data.endswith(bp.EOF_BLOCK)
    kinds = [m[2][0] & 7 for m in members]
    assert 5 in kinds and kinds.index(5) > len(bp.bgzf_members(parts[0])) and kinds[-1] == 3
    stream = b"".join(m[0] for m in members)
    text, refs, at = bp.parse_bam_header(stream)
    assert text == bp.sam_header_text(table[2], table[1], extra) and refs == [(n.encode(), l) for n, l in zip(table[2], table[1])]
    want = [ctx.sam_pe_batch(opt, topt, g, flags=DEV)[0] for g in (first, second)]
    assert bp.split_records(stream[at:]) == _records_of(want[0] + want[1], ids)


def test_deflate_times(ctx, gold, fixture_reads, own_regions):
    table = _ready(ctx, gold, fixture_reads)
    opt, topt = bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    g = _paired_fixture(fixture_reads, *own_regions, table, NO_PES)
    ctx.bam_pe_batch(opt, topt, g, flags=Z)
    t, b = bpsw_hip.last_bam_deflate_times(), bpsw_hip.last_bam_times()
    assert t[0] > 0 and t[1] > 0 and all(x >= 0 for x in t) and b[0] > 0 and b[1] > 0 and b[2] == 0
    ctx.bam_pe_batch(opt, topt, g)
    assert bpsw_hip.last_bam_deflate_times() == (0.0, 0.0, 0.0, 0.0) and bpsw_hip.last_bam_times()[2] > 0
