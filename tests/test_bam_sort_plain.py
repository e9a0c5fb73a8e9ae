"""tests/bam_sort_plain.py, the yardstick of bpsw_bam_sort, pinned on literals worked out by hand from the specification (5.2, 5.3)."""
import struct

import bam_plain as bp
import bam_sort_plain as sp

REF = {b"A": 0, b"B": 1}


def rec(name, flag, rname, pos1, cigar, n=4):
    seq = b"ACGT" * ((n + 3) // 4)
    return bp.sam_to_bam(b"\t".join([name, b"%d" % flag, rname, b"%d" % pos1, b"30", cigar, b"*", b"0", b"0", seq[:n], b"I" * n]), REF)


def test_three_records_on_two_contigs():
    r0, r1, r2 = rec(b"r0", 0, b"A", 101, b"50M", 50), rec(b"r1", 0, b"B", 11, b"20M", 20), rec(b"r2", 16, b"A", 6, b"30M", 30)
    assert [sp.fields(r) for r in (r0, r1, r2)] == [(0, 100, 150, 0), (1, 10, 30, 0), (0, 5, 35, 16)]
    srt = sp.sort_records([r0, r1, r2], 2)
    assert srt == [r2, r0, r1]
    off, size = sp.offsets_of(srt)
    assert off == [0, len(r2), len(r2) + len(r0)] and size == len(r0) + len(r1) + len(r2) < 65280
    base = 1000 << 16          # one block at file offset 1000: a virtual offset is that << 16 | the stream offset
    a0, a1, b1 = base, base + off[2], base + size
    want = b"BAI\1" + struct.pack("<i", 2)
    # contig A: both records lie in the first 16 Kib window, bin 4681; one chunk; the pseudo-bin; one linear entry
    want += struct.pack("<i", 2) + struct.pack("<IiQQ", 4681, 1, a0, a1) + struct.pack("<IiQQQQ", 37450, 2, a0, a1, 2, 0)
    want += struct.pack("<iQ", 1, a0)
    want += struct.pack("<i", 2) + struct.pack("<IiQQ", 4681, 1, a1, b1) + struct.pack("<IiQQQQ", 37450, 2, a1, b1, 1, 0)
    want += struct.pack("<iQ", 1, a1)
    want += struct.pack("<Q", 0)
    bai = sp.build_bai(srt, off, sp.stored_offsets(size, 65280), 65280, 1000, 2)
    assert bai == want
    assert sp.bai_query(bai, 0, 0, 10) == [(a0, a1)] and sp.bai_query(bai, 1, 0, 10) == [(a1, b1)] and sp.bai_query(bai, 0, 20000, 20001) == []


def test_one_unplaced_record():
    r = rec(b"u", 4, b"*", 0, b"*")
    assert sp.fields(r) == (-1, -1, 0, 4) and sp.sort_key(r, 1) == (1, 0, 0)
    bai = sp.build_bai([r], [0], sp.stored_offsets(len(r), 65280), 65280, 0, 1)
    assert bai == bytes.fromhex("42414901" "01000000" "00000000" "00000000" "0100000000000000")
    assert sp.parse_bai(bai) == ([({}, None, [])], 1)


def test_a_record_that_straddles_a_window():
    r = rec(b"s", 0, b"A", 16381, b"10M", 10)       # [16380, 16390): windows 0 and 1, so not a bin of the last level but 585 + 0
    assert sp.fields(r)[:3] == (0, 16380, 16390) and bp.reg2bin(16380, 16390) == 585
    end = len(r)
    bai = sp.build_bai([r], [0], sp.stored_offsets(end, 65280), 65280, 0, 2)
    want = b"BAI\1" + struct.pack("<i", 2) + struct.pack("<i", 2) + struct.pack("<IiQQ", 585, 1, 0, end)
    want += struct.pack("<IiQQQQ", 37450, 2, 0, end, 1, 0) + struct.pack("<iQQ", 2, 0, 0) + struct.pack("<ii", 0, 0) + struct.pack("<Q", 0)
    assert bai == want
    assert sp.reg2bins(16380, 16390) == [0, 1, 9, 73, 585, 4681, 4682]


def test_block_edges_in_virtual_offsets_and_holes_in_the_linear_index():
    recs = [rec(b"a", 0, b"A", 1, b"4M"), rec(b"b", 0, b"A", 3 * 16384 + 1, b"4M"), rec(b"c", 4, b"A", 3 * 16384 + 1, b"*")]
    off, size = sp.offsets_of(recs)
    P = len(recs[0])                                  # the second record begins a block: its start is (coff[1], 0), as is the first's end
    coff = sp.stored_offsets(size, P)
    assert coff[:2] == [0, P + 31] and coff[-1] == size + 31 * ((size + P - 1) // P)
    refs, none = sp.parse_bai(sp.build_bai(recs, off, coff, P, 7, 2))
    bins, pseudo, linear = refs[0]
    v1 = (7 + P + 31) << 16
    assert bins[4681] == [(7 << 16, v1)] and bins[4684][0][0] == v1 and len(bins[4684]) == 1     # the two at one place: one chunk
    assert pseudo[1] == (2, 1) and pseudo[0][0] == 7 << 16 and none == 0
    assert linear == [7 << 16, v1, v1, v1]            # windows 1 and 2 take window 3's entry
    assert refs[1] == ({}, None, [])


def test_ties_keep_their_order_and_the_strand_bit_counts():
    a, b, c, d = rec(b"a", 16, b"A", 10, b"4M"), rec(b"b", 0, b"A", 10, b"4M"), rec(b"c", 16, b"A", 10, b"4M"), rec(b"d", 0, b"A", 10, b"4M")
    u = rec(b"u", 4, b"*", 0, b"*")
    assert sp.sort_records([u, a, b, c, d], 2) == [b, d, a, c, u]


def test_the_writer_and_the_reader_agree():
    recs = [rec(b"n%d" % k, 0, b"A", 1 + 100 * k, b"4M") for k in range(40)]
    stream = b"".join(recs)
    for level in (0, 6):
        for P in (64, len(stream) - 1, len(stream), len(stream) + 1):
            data = sp.bgzf_write(stream, P, level)
            members = bp.bgzf_members(data)
            assert b"".join(m[0] for m in members) == stream and all(len(m[0]) == P for m in members[:-1])
            coff = sp.member_offsets(data)
            assert level or coff == sp.stored_offsets(len(stream), P)
            off, size = sp.offsets_of(recs)
            bai = sp.build_bai(recs, off, coff, P, 0, 2)
            for beg, end in ((0, 1), (150, 1250), (3900, 3905), (3904, 4000)):
                got = sp.read_chunks(data, sp.bai_query(bai, 0, beg, end))
                assert [r for r in got if r in sp.overlapping(recs, 0, beg, end)] == sp.overlapping(recs, 0, beg, end)
                assert set(got) <= set(recs)
