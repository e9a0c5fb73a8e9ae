"""bpsw_bam_sort on the device: the BAM entries' outputs to a coordinate-sorted BAM body and its .bai (csrc/bpsw_bam_sort.hip:
bam_walk_kernel, bam_key_kernel, bam_len_kernel, bam_gather_kernel, the index build's radix sort, the BAM entries' framing kernels).

Every case decodes `out` with the BGZF reader of tests/bam_plain.py, compares the records byte for byte with the yardstick's stable sort
of the input's records (tests/bam_sort_plain.py), compares `bai` byte for byte with the yardstick's BAI over the blocks' offsets read
from `out`, and for a few regions per contig reads the file by the BAI's chunks and requires exactly the records a linear scan finds
overlapping.  The inputs are tests/bam_sort_cases.py's records, framed by the yardstick's BGZF writer, and the library's own BAM output."""
import ctypes as C
import random

import numpy as np
import pytest

import bam_plain as bp
import bam_sort_cases as bc
import bam_sort_plain as sp
import bpsw_hip
from tail_util import load_sam_pe_golden
from test_bam_gpu import P0, _ref_id, payload
from test_deflate_core_host import build_host, run_host
from test_sam_pe_gpu import PAIR_ORDER, _paired_fixture, _ready, own_regions  # noqa: F401
from test_sam_se_gpu import NO_PES, fixture_reads, gold  # noqa: F401

pytestmark = pytest.mark.gpu

Z = bpsw_hip.BAM_DEFLATE


class window:
    """bam_walk_kernel's window for the calls inside, the default again behind them"""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        assert bpsw_hip.bam_sort_set_window(self.n) == 0

    def __exit__(self, *a):
        assert bpsw_hip.bam_sort_set_window(0) == 0


@pytest.fixture(scope="module")
def twin():
    return build_host(False)


def frame(records, p=P0, level=0):
    return sp.bgzf_write(b"".join(records), p, level)


def verify(out, bai, n, records, lens, p, file_off=0, stored=True, n_regions=4):
    """`out` and `bai` against the yardstick -> the sorted stream"""
    srt = sp.sort_records(records, len(lens))
    members = bp.bgzf_members(out)
    stream = b"".join(m[0] for m in members)
    assert n == len(records)
    assert bp.split_records(stream) == srt
    assert [len(m[0]) for m in members] == [p] * (len(stream) // p) + ([len(stream) % p] if len(stream) % p else [])
    coff = sp.member_offsets(out)
    if stored:
        assert coff == sp.stored_offsets(len(stream), p) and all(m[2][0] == 1 for m in members)
    off, _ = sp.offsets_of(srt)
    assert bai == sp.build_bai(srt, off, coff, p, file_off, len(lens))
    data = bytes(file_off) + out
    contigs = sorted(set(list(range(min(len(lens), 3))) + [len(lens) - 1])) if lens else []
    for rid, beg, end in [r for r in bc.regions(lens, 11, 2 + n_regions) if r[0] in contigs]:
        want = sp.overlapping(srt, rid, beg, end)
        got = sp.read_chunks(data, sp.bai_query(bai, rid, beg, end))
        assert [r for r in got if sp.fields(r)[0] == rid and sp.fields(r)[1] < end and sp.fields(r)[2] > beg] == want, (rid, beg, end)
    return stream


def sort_and_verify(ctx, records, lens, p_in=P0, level=0, p_out=0, seg_off=None, flags=0, file_off=0, body=None, twin=None):
    body = frame(records, p_in, level) if body is None else body
    with payload(p_out) as p:
        out, bai, n = ctx.bam_sort(body, seg_off=seg_off, flags=flags, file_off=file_off, lens=lens)
    stream = verify(out, bai, n, records, lens, p, file_off, stored=not flags)
    if flags:
        assert twin is not None
        assert run_host(twin, [(p, stream)], "bam_sort_gpu") == [out]     # the deflate core's host twin over the same payloads
    return out, bai


# ---- counts, ties, key widths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 4095, 4096, 4097])
def test_counts_around_a_wavefront_and_a_sort_tile(ctx, n):
    lens = [100000, 3000]
    sort_and_verify(ctx, bc.random_records(n, lens, 100 + n), lens)


def test_ties_and_orders(ctx):
    lens = [5000, 70000]
    base = bc.random_records(300, lens, 7)
    same = [bc.with_pos(bc.with_ref_id(r, 1), 1234) for r in base if sp.fields(r)[0] >= 0 and not sp.fields(r)[3] & 16]
    unplaced = bc.random_records(50, lens, 8, unplaced_every=1)
    srt = sp.sort_records(base, 2)
    strands = bc.records_of([bc.placed(b"s%d" % k, 0, 77, 100, random.Random(k), flag=(16, 0)[k % 2]) for k in range(10)], 2)
    for recs in (same, unplaced, srt, srt[::-1], strands):
        out, _ = sort_and_verify(ctx, recs, lens, p_out=1021)
        if recs in (same, unplaced, srt):
            assert bp.bgzf_inflate(out) == b"".join(recs)             # the stream comes back as it went in
    assert [sp.fields(r)[3] & 16 for r in bp.split_records(bp.bgzf_inflate(out))] == [0] * 5 + [16] * 5


@pytest.mark.parametrize("n_ref", [1, 255, 256, 257])
def test_key_widths_by_the_number_of_contigs(ctx, n_ref):
    lens = [1, 255, 65536, 1 << 29][: min(n_ref, 4)] + [1000] * max(0, n_ref - 4)
    recs = bc.random_records(400, lens, n_ref) + bc.edge_records(lens, n_ref + 1)
    _, bai = sort_and_verify(ctx, recs, lens, p_out=1021, file_off=12345)
    if n_ref >= 4:
        refs, _ = sp.parse_bai(bai)
        assert 4681 + (((1 << 29) - 1) >> 14) in refs[3][0] and len(refs[3][2]) == 1 << 15     # the top bin, the last linear window


@pytest.mark.parametrize("longest", [1, 255, 65536, 1 << 29])
def test_key_widths_by_the_longest_contig(ctx, longest):
    lens = [longest, 1]
    sort_and_verify(ctx, bc.random_records(200, lens, longest % 1000) + bc.edge_records(lens, 3), lens, p_out=256)


# ---- the walk -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", [64, 256, 0])
def test_windows_whose_edge_falls_in_every_part_of_a_record(ctx, win):
    lens = [40000, 900]
    recs = bc.random_records(300, lens, 40 + win)       # about 200 bytes each, 300 of them: the edge of a 64-byte window lands everywhere
    rng = random.Random(5)
    long_one = bc.records_of([bc.line(b"n" * 254, 0, b"c0", 101, b"10000M", 10000, rng)], 2)    # longer than any window
    assert 150 < sum(map(len, recs)) / len(recs) < 300 and len(long_one[0]) > 15000
    with window(win):
        sort_and_verify(ctx, recs[:150] + long_one + recs[150:], lens, p_in=4096)


@pytest.mark.parametrize("n_seg", [1, 2, 65])
def test_segments(ctx, n_seg):
    lens = [40000, 900]
    recs = bc.random_records(260, lens, 21)
    cut = [len(recs) * k // n_seg for k in range(n_seg + 1)]
    parts = [frame(recs[cut[k]: cut[k + 1]], 256) for k in range(n_seg)]
    body = b"".join(parts)
    starts = [sum(map(len, parts[:k])) for k in range(n_seg)]
    with window(256):
        a = sort_and_verify(ctx, recs, lens, body=body, seg_off=starts)               # the calls' starts, 0 first
        b = sort_and_verify(ctx, recs, lens, body=body, seg_off=starts[1:])           # ... without it: the first segment begins at 0 anyway
        c = sort_and_verify(ctx, recs, lens, body=body, seg_off=starts[1:] + [len(body)])
        d = sort_and_verify(ctx, recs, lens, body=body)
    assert a == b == c == d


def test_an_empty_segment_and_end_of_file_blocks_in_the_middle(ctx):
    lens = [40000, 900]
    recs = bc.random_records(90, lens, 22)
    parts = [frame(recs[:30], 1021), frame(recs[30:], 1021)]
    at = len(parts[0])
    sort_and_verify(ctx, recs, lens, body=parts[0] + parts[1], seg_off=[0, at, at, at])
    body = bp.EOF_BLOCK + parts[0] + bp.EOF_BLOCK + bp.EOF_BLOCK + parts[1] + bp.EOF_BLOCK
    sort_and_verify(ctx, recs, lens, body=body)
    sort_and_verify(ctx, recs, lens, body=body, seg_off=[28, 28 + at, 28 + at + 28, 28 + at + 56])
    sort_and_verify(ctx, [], lens, body=bp.EOF_BLOCK)
    sort_and_verify(ctx, [], lens, body=b"")


# ---- block edges ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [64, 256, 1021, 0])
def test_input_and_output_payloads(ctx, twin, p):
    lens = [300000, 77]
    recs = bc.random_records(500, lens, 60 + p)
    stream = b"".join(recs)
    mixed = b"".join(sp.bgzf_member(stream[at: at + (p or P0)], (0, 6, 1)[k % 3]) for k, at in enumerate(range(0, len(stream), p or P0)))
    for body in (frame(recs, p or P0, 0), frame(recs, p or P0, 6), mixed):
        sort_and_verify(ctx, recs, lens, body=body, p_out=p)
    if p != 64:        # (at 64 bytes the twin's every block is stored: nothing the stored case does not show)
        sort_and_verify(ctx, recs, lens, body=mixed, p_out=p, flags=Z, twin=twin, file_off=999)
    sort_and_verify(ctx, recs, lens, body=frame(recs, 4096, 1), p_out=p, flags=Z if p else 0, twin=twin)


def test_a_sorted_stream_of_exactly_one_block_and_a_byte_around(ctx, twin):
    lens = [300000]
    recs = bc.random_records(40, lens, 5, unplaced_every=0)
    size = sum(map(len, recs))
    for p in (size - 1, size, size + 1):
        for flags in (0, Z):
            out, _ = sort_and_verify(ctx, recs, lens, p_out=p, flags=flags, twin=twin)
            assert len(bp.bgzf_members(out)) == (2 if p < size else 1)


# ---- virtual offsets: a whole file ----------------------------------------------------------------------------------------------------------
def test_a_whole_file_parsed_from_byte_0_and_sought_by_the_index(ctx, twin):
    lens, names = [40000, 900, 5], ["one", "two", "three"]
    recs = bc.random_records(700, lens, 70)
    header = bpsw_hip.bam_header(lens, names, b"@PG\tID:t\n", flags=bpsw_hip.HDR_COORDINATE)
    assert header != bpsw_hip.bam_header(lens, names, b"@PG\tID:t\n") == bpsw_hip.bam_header(lens, names, b"@PG\tID:t\n", flags=0)
    assert bpsw_hip.sam_header(lens, names, flags=1).startswith(b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:one\tLN:40000\n")
    assert bpsw_hip.sam_header(lens, names) == bp.sam_header_text(names, lens)
    with pytest.raises(bpsw_hip.BpswError, match=r"\(-1\)"):
        bpsw_hip.bam_header(lens, names, flags=2)
    for flags in (0, Z):
        with payload(4096):
            out, bai, n = ctx.bam_sort(frame(recs, 1021), flags=flags, file_off=len(header), lens=lens)
        data = header + out + bpsw_hip.bam_eof()
        text, refs, at = bp.parse_bam_header(bp.bgzf_inflate(data))
        assert text.startswith(b"@HD\tVN:1.6\tSO:coordinate\n") and refs == [(b"one", 40000), (b"two", 900), (b"three", 5)]
        srt = sp.sort_records(recs, 3)
        assert bp.split_records(bp.bgzf_inflate(data)[at:]) == srt and n == 700
        assert bai == sp.build_bai(srt, sp.offsets_of(srt)[0], sp.member_offsets(out), 4096, len(header), 3)
        for rid, beg, end in bc.regions(lens, 3, 6):
            got = sp.read_chunks(data, sp.bai_query(bai, rid, beg, end))
            assert [r for r in got if r in sp.overlapping(srt, rid, beg, end)] == sp.overlapping(srt, rid, beg, end)
        refs, none = sp.parse_bai(bai)
        first, last = refs[0][1][0]
        assert first >> 16 == len(header) and none == sum(sp.fields(r)[0] < 0 for r in recs) > 0


# ---- the library's own output ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stem", ["mem_sam_pe", "mem_sam_pe_all", "mem_sam_pe_rg"])
def test_goldens_in_two_calls(ctx, twin, stem):
    pac, g, flag, _ = load_sam_pe_golden(stem)
    ctx.ref_load(pac, g.l_pac)
    names = [bytes(g.ann_name_pool[int(g.ann_name_off[i]):int(g.ann_name_off[i + 1])]).decode() for i in range(g.ann_off.shape[0])]
    ctx.bns_load(g.ann_off, g.ann_len, names)
    opt, topt = bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    opt.flag, topt.rg_id = flag, g.rg_id
    with payload(4096):
        a, b = ctx.bam_pe_batch(opt, topt, g)[0], ctx.bam_pe_batch(opt, topt, g, flags=Z)[0]      # the same records twice: ties, mixed blocks
    recs = bp.split_records(bp.bgzf_inflate(a)) * 2
    lens = [int(x) for x in g.ann_len]
    for seg in ([len(a)], [0, len(a)], [len(a), len(a) + len(b)]):
        with payload(1021) as p:
            out, bai, n = ctx.bam_sort(a + b, seg_off=seg)                                      # the contigs: the table just loaded
        verify(out, bai, n, recs, lens, p)
    sort_and_verify(ctx, recs, lens, body=a + b, seg_off=[len(a)], p_out=4096, flags=Z, twin=twin)


def test_the_fixture_pairs_in_two_calls(ctx, gold, fixture_reads, own_regions):
    table = _ready(ctx, gold, fixture_reads)
    opt, topt = bpsw_hip.default_opt(), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    opt.flag = bpsw_hip.MEM_F_ALL
    first = _paired_fixture(fixture_reads, *own_regions, table, NO_PES, order=PAIR_ORDER[:60])
    second = _paired_fixture(fixture_reads, *own_regions, table, NO_PES, order=PAIR_ORDER[60:])
    a, b = ctx.bam_pe_batch(opt, topt, first)[0], ctx.bam_pe_batch(opt, topt, second)[0]
    recs = bp.split_records(bp.bgzf_inflate(a + b))
    assert len(recs) >= 104 and _ref_id(table[2])
    with payload(256) as p:
        out, bai, n = ctx.bam_sort(a + b, seg_off=[len(a)], file_off=321)
    verify(out, bai, n, recs, [int(x) for x in table[1]], p, 321)
    t = bpsw_hip.last_bam_sort_times()
    assert len(t) == 8 and all(x >= 0 for x in t) and all(t[k] > 0 for k in (0, 1, 2, 3, 4, 5, 7)) and t[7] >= t[6]


# ---- refusals and capacity ------------------------------------------------------------------------------------------------------------------
def _raw(ctx, body, lens, cap, bai_cap, seg=None, flags=0):
    ln = np.ascontiguousarray(lens, np.int32)
    sg = None if seg is None else np.ascontiguousarray(seg, np.int64)
    out, bai = np.full(cap + 64, 0xAB, np.uint8), np.full(bai_cap + 64, 0xAB, np.uint8)
    need, bneed, n = C.c_size_t(0), C.c_size_t(0), C.c_int64(0)
    rc = ctx.lib.bpsw_bam_sort(ctx.h, body, len(body), bpsw_hip._ptr(sg), 0 if sg is None else len(sg), len(ln), bpsw_hip._ptr(ln), 0, flags,
                               bpsw_hip._ptr(out), cap, C.byref(need), bpsw_hip._ptr(bai), bai_cap, C.byref(bneed), C.byref(n))
    return rc, out, bai, need.value, bneed.value, n.value


@pytest.mark.parametrize("flags", [0, Z])
def test_capacity_one_byte_short(ctx, flags):
    lens = [40000, 900]
    recs = bc.random_records(200, lens, 80)
    body = frame(recs, 4096)
    with payload(1021):
        whole, index, n = ctx.bam_sort(body, flags=flags, lens=lens)
        for cap, bai_cap in ((len(whole) - 1, len(index)), (len(whole), len(index) - 1), (0, 0)):
            rc, out, bai, need, bneed, cnt = _raw(ctx, body, lens, cap, bai_cap, flags=flags)
            assert (rc, need, bneed, cnt) == (-3, len(whole), len(index), 200)
            assert (out == 0xAB).all() and (bai == 0xAB).all()                     # nothing is written, not even below the capacity
        rc, out, bai, need, bneed, cnt = _raw(ctx, body, lens, len(whole), len(index), flags=flags)
        assert rc == 0 and out[: need].tobytes() == whole and bai[: bneed].tobytes() == index and (out[need:] == 0xAB).all()
        with pytest.raises(bpsw_hip.BamSortError) as e:
            ctx.bam_sort(body, flags=flags, lens=lens, cap=len(whole) - 1, bai_cap=len(index))
        assert e.value.rc == -3 and e.value.needed == (len(whole), len(index)) and e.value.n_records == 200


def test_refusals(ctx):
    lens = [40000, 900]
    recs = bc.random_records(20, lens, 33)
    off, size = sp.offsets_of(recs)
    body = frame(recs, 256)

    def refused(rc, text, body=body, lens=lens, **kw):
        with pytest.raises(bpsw_hip.BamSortError, match=text) as e:
            ctx.bam_sort(body, lens=lens, **kw)
        assert e.value.rc == rc
    coff = sp.member_offsets(body)
    refused(-1, "segment 1 begins at offset %d, which is not a block boundary" % (coff[1] + 13), seg_off=[coff[1] + 13])
    k = max(i for i in range(20) if off[i] < 8 * 256)                  # the record that block 8's start, stream offset 2048, lies in
    assert off[k] < 8 * 256 < off[k] + len(recs[k])
    refused(-1, r"segment 0: the chain of block_size fields does not end on the segment's end \(stream offset %d\)" % off[k], seg_off=[coff[8]])
    refused(-1, "not ascending", seg_off=[coff[2], coff[1]])
    refused(-1, "record 3: refID is outside", body=frame(recs[:3] + [bc.with_ref_id(recs[3], 2)] + recs[4:], 256))
    refused(-1, "record 4: block_size is below", body=frame(recs[:4] + [bc.with_block_size(recs[4], 31)] + recs[5:], 256))
    placed = next(k for k, r in enumerate(recs) if sp.fields(r)[0] == 1)
    refused(-1, "record %d: pos is below -1, or at or above" % placed,
            body=frame(recs[:placed] + [bc.with_pos(recs[placed], 900)] + recs[placed + 1:], 256))
    refused(-4, "contig 1 is longer than 2\\^29", lens=[40000, (1 << 29) + 1])
    header = bp.bam_header_stream(bp.sam_header_text([b"c0", b"c1"], lens), [b"c0", b"c1"], lens)
    refused(-1, r"segment 0: the chain of block_size fields .*\(stream offset 0\)", body=sp.bgzf_write(header + b"".join(recs), 4096))
    refused(-1, "unknown flag", flags=1)
    refused(-1, "bytes behind the last whole block", body=body + b"\x1f\x8b")
    refused(-1, "block 0: ", body=b"BAM\1" + body)
    bad_crc = bytearray(body)
    bad_crc[coff[1] + 40] ^= 1                                         # a byte of block 1's payload
    refused(-1, "block 1: the CRC-32 differs", body=bytes(bad_crc))
    assert bpsw_hip.bam_sort_set_window(63) == -1 and bpsw_hip.bam_sort_set_window(16385) == -1 and bpsw_hip.bam_sort_set_window(0) == 0
    sort_and_verify(ctx, recs, lens, body=body)                                        # and the context still sorts
