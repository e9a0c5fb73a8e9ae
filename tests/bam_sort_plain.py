"""A plain-Python yardstick for bpsw_bam_sort, written from the SAM specification (4.2 the record, 5.2 the BAI, 5.3 the bins) and the
rules the entry documents: the order (refID with -1 last, pos, the strand bit, ties in input order), a chunk per maximal run of one bin,
the pseudo-bin 37450, the linear index with its holes filled from the right.  It sits beside tests/bam_plain.py and uses that file's
split_records, reg2bin and bgzf_members; it knows nothing of the library.  tests/test_bam_sort_plain.py pins it on literals."""
import struct
import zlib

import bam_plain as bp

PSEUDO_BIN = 37450
REF_OPS = (0, 2, 3, 7, 8)     # M D N = X consume reference


def fields(rec: bytes):
    """-> (refID, pos, end, flag) of a record (block_size included): end = pos + the reference bases of the CIGAR, pos + 1 without any
    or at pos -1"""
    ref, pos, l_name, _mapq, _bin, n_cig, flag, _l_seq = struct.unpack_from("<iiBBHHHI", rec, 4)
    ops = struct.unpack_from("<%dI" % n_cig, rec, 36 + l_name)
    ref_len = sum(w >> 4 for w in ops if (w & 15) in REF_OPS)
    return ref, pos, pos + (ref_len if pos >= 0 and ref_len > 0 else 1), flag


def sort_key(rec: bytes, n_ref: int):
    ref, pos, _end, flag = fields(rec)
    return (n_ref if ref < 0 else ref, pos + 1, (flag >> 4) & 1)


def sort_records(records, n_ref: int):
    """Python's stable sorted on (refID with -1 as n_ref, pos + 1, the reverse-strand bit)"""
    return sorted(records, key=lambda r: sort_key(r, n_ref))


def offsets_of(records):
    """-> (the offset of every record in the stream they form, the stream's size)"""
    off, at = [], 0
    for r in records:
        off.append(at)
        at += len(r)
    return off, at


def build_bai(records, rec_off, coff, P: int, file_off: int, n_ref: int) -> bytes:
    """records in file order with their offsets in the stream; coff[b]: where block b of the stream (P bytes each) begins in the output,
    coff[blocks] the output's size -> the BAI's bytes"""
    size = rec_off[-1] + len(records[-1]) if records else 0

    def voff(o):
        return (file_off + coff[o // P]) << 16 | o % P
    ends = rec_off[1:] + [size]
    out = b"BAI\1" + struct.pack("<i", n_ref)
    k = 0
    for ref in range(n_ref):
        bins, linear, first, counts, last_bin = {}, {}, k, [0, 0], None
        while k < len(records) and fields(records[k])[0] == ref:
            _, pos, end, flag = fields(records[k])
            b = bp.reg2bin(pos, end)
            v0, v1 = voff(rec_off[k]), voff(ends[k])
            if b == last_bin:
                bins[b][-1][1] = v1
            else:
                bins.setdefault(b, []).append([v0, v1])
            last_bin = b
            counts[(flag >> 2) & 1] += 1
            for w in range(max(pos, 0) >> 14, (max(end - 1, 0) >> 14) + 1):
                linear[w] = min(linear.get(w, v0), v0)
            k += 1
        if k == first:
            out += struct.pack("<ii", 0, 0)
            continue
        out += struct.pack("<i", len(bins) + 1)
        for b in sorted(bins):
            out += struct.pack("<Ii", b, len(bins[b])) + b"".join(struct.pack("<QQ", *c) for c in bins[b])
        out += struct.pack("<IiQQQQ", PSEUDO_BIN, 2, voff(rec_off[first]), voff(ends[k - 1]), counts[0], counts[1])
        n_intv = max(linear) + 1
        row = [None] * n_intv
        for w in range(n_intv - 1, -1, -1):
            row[w] = linear[w] if w in linear else row[w + 1]
        out += struct.pack("<i", n_intv) + struct.pack("<%dQ" % n_intv, *row)
    return out + struct.pack("<Q", len(records) - k)


def parse_bai(bai: bytes):
    """-> ([(bins {bin: [(beg, end)]}, pseudo [(beg, end), (mapped, unmapped)] or None, linear [ioffset])] per contig, n_no_coor)"""
    assert bai[:4] == b"BAI\1"
    n_ref, at, refs = struct.unpack_from("<i", bai, 4)[0], 8, []
    for _ in range(n_ref):
        n_bin, bins, pseudo = struct.unpack_from("<i", bai, at)[0], {}, None
        at += 4
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, at)
            chunks = [struct.unpack_from("<QQ", bai, at + 8 + 16 * c) for c in range(n_chunk)]
            at += 8 + 16 * n_chunk
            if b == PSEUDO_BIN:
                pseudo = chunks
            else:
                assert b not in bins
                bins[b] = chunks
        n_intv = struct.unpack_from("<i", bai, at)[0]
        linear = list(struct.unpack_from("<%dQ" % n_intv, bai, at + 4))
        at += 4 + 8 * n_intv
        refs.append((bins, pseudo, linear))
    n_no_coor = struct.unpack_from("<Q", bai, at)[0] if at < len(bai) else None
    assert at + 8 == len(bai)
    return refs, n_no_coor


def reg2bins(beg: int, end: int):
    """the bins that may hold records overlapping the 0-based half-open [beg, end) (specification 5.3)"""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


def bai_query(bai: bytes, ref: int, beg: int, end: int):
    """the chunks a reader visits for [beg, end) of contig ref: those of reg2bins' bins that end above the linear index's lower bound
    for beg's window, sorted by their start"""
    bins, _pseudo, linear = parse_bai(bai)[0][ref]
    w = beg >> 14
    if w >= len(linear):       # behind the last overlapped window nothing overlaps
        return []
    return sorted(c for b in reg2bins(beg, end) for c in bins.get(b, []) if c[1] > linear[w])


def read_chunks(data: bytes, chunks):
    """the records (block_size included) a reader gets from the file `data` by seeking to every chunk's start and reading records until
    the virtual offset reaches its end; a record is returned once however many chunks hold it"""
    cache, got, seen = {}, [], set()

    def block(coff):
        if coff not in cache:
            bsize = struct.unpack_from("<H", data, coff + 16)[0] + 1
            (m,) = bp.bgzf_members(data[coff: coff + bsize])
            cache[coff] = (m[0], bsize)
        return cache[coff]

    def take(coff, uoff, n):
        """n bytes from (coff, uoff) -> (bytes, the position behind them: never a block's end, but the next block's start)"""
        out = b""
        while True:
            if coff < len(data):
                pay, bsize = block(coff)
                if uoff == len(pay):
                    coff, uoff = coff + bsize, 0
                    continue
            if n == 0:
                return out, coff, uoff
            assert coff < len(data), "a read past the end of the file"
            part = pay[uoff: uoff + n]
            out, uoff, n = out + part, uoff + len(part), n - len(part)

    for beg, end in chunks:
        _, coff, uoff = take(beg >> 16, beg & 0xffff, 0)
        while (coff << 16 | uoff) < end and coff < len(data):
            start = (coff, uoff)
            head, coff, uoff = take(coff, uoff, 4)
            body, coff, uoff = take(coff, uoff, struct.unpack("<I", head)[0])
            if start not in seen:
                seen.add(start)
                got.append((start, head + body))
    return [r for _, r in sorted(got)]


def overlapping(records, ref: int, beg: int, end: int):
    """a linear scan: the records of contig ref whose [pos, end) overlaps [beg, end)"""
    out = []
    for r in records:
        rid, pos, rend, _ = fields(r)
        if rid == ref and pos < end and rend > beg:
            out.append(r)
    return out


def bgzf_write(stream: bytes, P: int, level: int = 0) -> bytes:
    """the stream cut every P bytes, each part one BGZF member: stored (level 0) or deflated by zlib at that level"""
    out = b""
    for at in range(0, len(stream), P):
        out += bgzf_member(stream[at: at + P], level)
    return out


def bgzf_member(payload: bytes, level: int = 0) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    cdata = c.compress(payload) + c.flush()
    assert len(cdata) + 26 <= 65536
    return (bytes.fromhex("1f8b08040000000000ff060042430200") + struct.pack("<H", len(cdata) + 25) + cdata +
            struct.pack("<II", zlib.crc32(payload), len(payload)))


def stored_offsets(size: int, P: int):
    """coff of a stream framed in stored blocks: block b at b (P + 31); the output's size behind the last"""
    blocks = (size + P - 1) // P
    return [b * (P + 31) for b in range(blocks)] + [size + 31 * blocks]


def member_offsets(framed: bytes):
    """coff of any framed output, read from its members"""
    coff, at = [], 0
    for _, total, _ in bp.bgzf_members(framed):
        coff.append(at)
        at += total
    return coff + [at]
