"""tests/bam_plain.py, the yardstick the BAM tests compare with, pinned on literals worked out by hand from the SAM specification."""
import struct
import zlib

import pytest

import bam_plain as bp


def test_reg2bin_literals():
    assert bp.reg2bin(0, 1) == 4681
    assert bp.reg2bin(-1, 0) == 4680                       # an unplaced record
    assert bp.reg2bin(16383, 16384) == 4681 and bp.reg2bin(16384, 16385) == 4682
    assert bp.reg2bin(16383, 16385) == 585                 # across a 16 kb edge: the 128 kb level
    assert bp.reg2bin(131071, 131073) == 73                # across a 128 kb edge: the 1 Mb level
    assert bp.reg2bin(0, 1 << 29) == 0


@pytest.mark.parametrize("beg,end,want", [
    # two bases either side of the 9th edge of a level lie in bin 1 of the level above: offsets 4681 585 73 9 1 0 (specification 5.3)
    ((9 << 14) - 1, (9 << 14) + 1, 585 + 1),       # 16 kb edge 9 is inside 128 kb bin 1
    ((9 << 17) - 1, (9 << 17) + 1, 73 + 1),        # 128 kb edge 9 is inside 1 Mb bin 1
    ((9 << 20) - 1, (9 << 20) + 1, 9 + 1),         # 1 Mb edge 9 is inside 8 Mb bin 1
    ((9 << 23) - 1, (9 << 23) + 1, 1 + 1),         # 8 Mb edge 9 is inside 64 Mb bin 1
    ((1 << 26) - 1, (1 << 26) + 1, 0),             # across a 64 Mb edge: bin 0
    (1 << 29, (1 << 29) + 1, 4681 + 32768),        # 37 449: beyond the 512 Mb the scheme was made for, the formula goes on
    (1 << 30, (1 << 30) + 1, 4681 + 65536),        # 70 217: more than the record's 16-bit field holds
])
def test_reg2bin_one_literal_per_level_and_beyond_512_mb(beg, end, want):
    assert want in (586, 74, 10, 2, 0, 37449, 70217)
    assert bp.reg2bin(beg, end) == want
    assert want != 70217 or want & 0xffff == 4681    # what the field keeps of it


@pytest.mark.parametrize("v,want", [(0, b"NMC\x00"), (255, b"NMC\xff"), (256, b"NMS\x00\x01"), (65535, b"NMS\xff\xff"),
                                    (65536, b"NMI\x00\x00\x01\x00"), (-1, b"NMc\xff"), (-128, b"NMc\x80"), (-129, b"NMs\x7f\xff"),
                                    (-32769, b"NMi\xff\x7f\xff\xff")])
def test_integer_tag_widths(v, want):
    assert bp.int_tag(b"NM", v) == want


def test_one_record_by_hand():
    line = b"r1\t99\tchr1\t101\t60\t4M\t=\t201\t104\tACGT\tIIII\tNM:i:0\n"
    want = bytes.fromhex(
        "31000000"      # block_size: 32 + 3 + 4 + 2 + 4 + 4
        "00000000"      # refID
        "64000000"      # pos 100
        "03" "3c"       # l_read_name, mapq 60
        "4912"          # bin 4681
        "0100" "6300"   # n_cigar_op, flag 99
        "04000000"      # l_seq
        "00000000"      # next_refID: '=' is the line's own
        "c8000000"      # next_pos 200
        "68000000"      # tlen 104
        "723100"        # r1 NUL
        "40000000"      # 4M
        "1248"          # A C | G T
        "28282828"      # 'I' - 33
        "4e4d4300")     # NM C 0
    assert bp.sam_to_bam(line, {b"chr1": 0}) == want


def test_unplaced_record_without_qualities_and_odd_length():
    rec = bp.sam_to_bam(b"q\t4\t*\t0\t0\t*\t*\t0\t0\tACN\t*\tAS:i:0\tXS:i:300\tRG:Z:g", {})
    assert struct.unpack_from("<iiBBHHHIiii", rec, 4) == (-1, -1, 2, 0, 4680, 0, 4, 3, -1, -1, 0)
    assert rec[36:] == b"q\0" + b"\x12\xf0" + b"\xff\xff\xff" + b"ASC\x00" + b"XSS\x2c\x01" + b"RGZg\0"


def test_hidden_sequence_and_hard_clip():
    rec = bp.sam_to_bam(b"q\t272\tc\t5\t0\t3H2M\t*\t0\t0\t*\t*", {b"c": 7})
    assert struct.unpack_from("<iiBBHHHIiii", rec, 4) == (7, 4, 2, 0, 4681, 2, 272, 0, -1, -1, 0)
    assert rec[36:] == b"q\0" + struct.pack("<II", 3 << 4 | 5, 2 << 4 | 0)


def test_bgzf_reader_on_members_made_with_zlib():
    def member(payload, level):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        cdata = c.compress(payload) + c.flush()
        return (b"\x1f\x8b\x08\x04" + bytes(4) + b"\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(cdata) + 25) + cdata +
                struct.pack("<II", zlib.crc32(payload), len(payload)))
    a, b = bytes(range(200)) * 3, b"xyz"
    data = member(a, 0) + member(b, 6) + bp.EOF_BLOCK
    assert [p for p, _, _ in bp.bgzf_members(data)] == [a, b, b""]
    assert bp.bgzf_inflate(data) == a + b
    bad = bytearray(data)
    bad[30] ^= 1   # a payload byte of the first, stored, member
    with pytest.raises(AssertionError, match="CRC32"):
        bp.bgzf_members(bytes(bad))


def test_header_stream_and_its_parser():
    text = bp.sam_header_text(["chr1", ""], [1000, 5], b"@PG\tID:x\n")
    assert text == b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:ctg2\tLN:5\n@PG\tID:x\n"
    s = bp.bam_header_stream(text, ["chr1", ""], [1000, 5])
    assert s[:8] == b"BAM\1" + struct.pack("<I", len(text))
    assert bp.parse_bam_header(s + b"rest") == (text, [(b"chr1", 1000), (b"ctg2", 5)], len(s))
