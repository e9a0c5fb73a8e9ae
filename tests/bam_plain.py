"""A plain-Python yardstick for the BAM output, written from the SAM specification alone (it knows nothing of the library's line
table): (1) the text of a SAM line -> the bytes of its BAM record (specification 4.2, bin by 5.3, tags typed as htslib's text parser
types them), and the header; (2) a BGZF reader that walks the gzip members by BSIZE, inflates each with zlib and checks CRC32 and
ISIZE with zlib.crc32.  tests/test_bam_plain.py pins it on literals."""
import struct
import zlib

CIGAR_OPS = b"MIDNSHP=X"
SEQ_NIBBLE = {c: i for i, c in enumerate(b"=ACMGRSVTWYHKDBN")}
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def reg2bin(beg: int, end: int) -> int:
    """the bin of the 0-based half-open [beg, end) (specification 5.3)"""
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def int_tag(tag: bytes, v: int) -> bytes:
    """an integer tag in the narrowest type: C S I from 0 up, c s i below"""
    if v >= 0:
        t, f = (b"C", "<B") if v <= 0xff else (b"S", "<H") if v <= 0xffff else (b"I", "<I")
    else:
        t, f = (b"c", "<b") if v >= -128 else (b"s", "<h") if v >= -32768 else (b"i", "<i")
    return tag + t + struct.pack(f, v)


def parse_cigar(text: bytes):
    """'*' -> []; else [(length, op index in MIDNSHP=X)]"""
    if text == b"*":
        return []
    out, n = [], 0
    for c in text:
        if 48 <= c <= 57:
            n = n * 10 + c - 48
        else:
            out.append((n, CIGAR_OPS.index(bytes([c]))))
            n = 0
    return out


def tag_bytes(field: bytes) -> bytes:
    tag, typ, val = field.split(b":", 2)
    assert len(tag) == 2, field
    if typ == b"i":
        return int_tag(tag, int(val))
    if typ == b"Z":
        return tag + b"Z" + val + b"\0"
    if typ == b"A":
        assert len(val) == 1
        return tag + b"A" + val
    raise ValueError(f"tag type {typ!r} is not one the library writes")


def sam_to_bam(line: bytes, ref_id: dict) -> bytes:
    """one SAM line (with or without its newline) -> its BAM record, block_size included.  ref_id: contig name -> index in the header"""
    f = line.rstrip(b"\n").split(b"\t")
    assert len(f) >= 11, line
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    rid = -1 if rname == b"*" else ref_id[rname]
    pos0 = int(pos) - 1
    ops = parse_cigar(cigar)
    ref_len = sum(n for n, op in ops if op in (0, 2, 3, 7, 8))
    bin_ = reg2bin(pos0, pos0 + (ref_len if ref_len > 0 else 1)) & 0xffff   # (the field has 16 bits)
    next_rid = -1 if rnext == b"*" else rid if rnext == b"=" else ref_id[rnext]
    bases = b"" if seq == b"*" else seq
    packed = bytearray((len(bases) + 1) // 2)
    for i, c in enumerate(bases):
        packed[i >> 1] |= SEQ_NIBBLE[c] << (0 if i & 1 else 4)
    if qual == b"*":
        quals = b"\xff" * len(bases)
    else:
        assert len(qual) == len(bases), line
        quals = bytes(q - 33 for q in qual)
    assert len(qname) + 1 <= 255 and len(ops) <= 0xffff
    body = struct.pack("<iiBBHHHIiii", rid, pos0, len(qname) + 1, int(mapq), bin_, len(ops), int(flag), len(bases), next_rid, int(pnext) - 1,
                       int(tlen))
    body += qname + b"\0" + b"".join(struct.pack("<I", n << 4 | op) for n, op in ops) + bytes(packed) + quals
    body += b"".join(tag_bytes(t) for t in f[11:])
    return struct.pack("<I", len(body)) + body


def sam_header_text(names, lens, extra: bytes = b"") -> bytes:
    """the header the library writes: @HD, one @SQ per contig (an empty name is ctg<index + 1>), the caller's lines"""
    out = b"@HD\tVN:1.6\tSO:unsorted\n"
    for k, (n, l) in enumerate(zip(names, lens)):
        n = n if isinstance(n, bytes) else n.encode()
        out += b"@SQ\tSN:" + (n or b"ctg%d" % (k + 1)) + b"\tLN:%d\n" % int(l)
    return out + extra


def bam_header_stream(text: bytes, names, lens) -> bytes:
    """the uncompressed bytes in front of the first record (specification 4.2)"""
    out = b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(names))
    for k, (n, l) in enumerate(zip(names, lens)):
        n = n if isinstance(n, bytes) else n.encode()
        n = n or b"ctg%d" % (k + 1)
        out += struct.pack("<I", len(n) + 1) + n + b"\0" + struct.pack("<I", int(l))
    return out


def bgzf_members(data: bytes):
    """walks the members by BSIZE -> [(payload, member size, the member's deflate bytes)]; every field of every member is checked"""
    out, at = [], 0
    while at < len(data):
        assert len(data) - at >= 28, "a trailing part shorter than the smallest member"
        id1, id2, cm, flg, _mtime, _xfl, _os, xlen = struct.unpack_from("<BBBBIBBH", data, at)
        assert (id1, id2, cm, flg) == (0x1f, 0x8b, 8, 4), f"not a BGZF member at {at}"
        bsize, x = None, at + 12
        while x < at + 12 + xlen:
            si1, si2, slen = struct.unpack_from("<BBH", data, x)
            if (si1, si2) == (66, 67):
                assert slen == 2
                bsize = struct.unpack_from("<H", data, x + 4)[0]
            x += 4 + slen
        assert x == at + 12 + xlen and bsize is not None, "no BC subfield"
        total = bsize + 1
        assert at + total <= len(data), "BSIZE runs past the data"
        cdata = data[at + 12 + xlen: at + total - 8]
        d = zlib.decompressobj(-15)
        payload = d.decompress(cdata)
        assert d.eof and not d.unused_data, "the deflate stream does not end where the member's trailer begins"
        crc, isize = struct.unpack_from("<II", data, at + total - 8)
        assert crc == zlib.crc32(payload), f"CRC32 of the member at {at}"
        assert isize == len(payload), f"ISIZE of the member at {at}"
        out.append((payload, total, cdata))
        at += total
    assert at == len(data)
    return out


def bgzf_inflate(data: bytes) -> bytes:
    return b"".join(p for p, _, _ in bgzf_members(data))


def split_records(stream: bytes):
    """a stream of BAM records -> the records (block_size included)"""
    out, at = [], 0
    while at < len(stream):
        n = struct.unpack_from("<I", stream, at)[0]
        assert at + 4 + n <= len(stream), "a record runs past the stream"
        out.append(stream[at: at + 4 + n])
        at += 4 + n
    return out


def parse_bam_header(stream: bytes):
    """-> (the header text, [(name, length)], the offset of the first record)"""
    assert stream[:4] == b"BAM\1"
    l_text = struct.unpack_from("<I", stream, 4)[0]
    text = stream[8: 8 + l_text]
    at = 8 + l_text
    n_ref = struct.unpack_from("<I", stream, at)[0]
    at += 4
    refs = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<I", stream, at)[0]
        name = stream[at + 4: at + 4 + l_name]
        assert name.endswith(b"\0")
        at += 4 + l_name
        refs.append((name[:-1], struct.unpack_from("<I", stream, at)[0]))
        at += 4
    return text, refs, at
