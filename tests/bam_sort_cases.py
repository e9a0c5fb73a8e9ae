"""Inputs for the tests of bpsw_bam_sort: BAM records made by tests/bam_plain.sam_to_bam from generated SAM lines, at the shapes the sort's
parts can go wrong at, and what the yardstick (tests/bam_sort_plain.py) says of them.  Shared by tests/test_bam_sort_core_host.py (the
rules on the host) and tests/test_bam_sort_gpu.py (the kernels)."""
import random
import struct

import bam_plain as bp
import bam_sort_plain as sp

BASES = b"ACGT"


def names_of(n_ref):
    return [b"c%d" % k for k in range(n_ref)]


def line(name: bytes, flag: int, rname: bytes, pos1: int, cigar: bytes, qlen: int, rng, tags=True) -> bytes:
    seq = bytes(rng.choice(BASES) for _ in range(qlen)) if qlen else b"*"
    qual = bytes(rng.randrange(35, 74) for _ in range(qlen)) if qlen else b"*"
    f = [name, b"%d" % flag, rname, b"%d" % pos1, b"%d" % rng.randrange(61), cigar, b"*", b"0", b"0", seq, qual]
    if tags:
        f += [b"NM:i:%d" % rng.randrange(5), b"MD:Z:%d" % max(qlen, 1), b"AS:i:%d" % qlen, b"XS:i:%d" % rng.randrange(max(qlen, 1))]
    return b"\t".join(f)


def placed(name, rid, pos0, room, rng, read_len=100, flag=None):
    """a line on contig rid at pos0 whose reference span stays inside `room` bases from pos0 (room >= 1); one of five CIGAR shapes"""
    span = min(room, read_len)
    shape = rng.randrange(5) if span >= 12 else 0
    if shape == 0:
        cigar, qlen = b"%dM" % span, span
    elif shape == 1:
        a = rng.randrange(3, span - 6)
        cigar, qlen = b"%dM2I%dM" % (a, span - a), span + 2
    elif shape == 2:
        a = rng.randrange(3, span - 6)
        cigar, qlen = b"%dM3D%dM" % (a, span - a - 3), span - 3
    elif shape == 3:
        cigar, qlen = b"5S%dM" % span, span + 5
    else:
        a = rng.randrange(3, span - 6)
        cigar, qlen = b"%d=1X%dM" % (a, span - a - 1), span
    fl = flag if flag is not None else rng.choice((0, 16, 0, 16, 4))     # (4 with a coordinate: an unmapped mate placed with its mate)
    if fl & 4:
        cigar, qlen = b"*", read_len
    return line(name, fl, b"c%d" % rid, pos0 + 1, cigar, qlen, rng)


def unplaced(name, rng, read_len=100):
    return line(name, 4, b"*", 0, b"*", read_len, rng)


def records_of(lines, n_ref):
    ref_id = {b"c%d" % k: k for k in range(n_ref)}
    return [bp.sam_to_bam(l, ref_id) for l in lines]


def random_records(n, lens, seed, read_len=100, unplaced_every=7):
    """n records spread over the contigs, every unplaced_every-th without a coordinate, in random order"""
    rng = random.Random(seed)
    lines = []
    for k in range(n):
        if unplaced_every and k % unplaced_every == unplaced_every - 1:
            lines.append(unplaced(b"u%d" % k, rng, read_len))
            continue
        rid = rng.randrange(len(lens))
        pos0 = rng.randrange(lens[rid])
        lines.append(placed(b"r%d" % k, rid, pos0, lens[rid] - pos0, rng, read_len))
    return records_of(lines, len(lens))


def edge_records(lens, seed):
    """per contig a record at position 0 and one at its last base, on both strands, and an unmapped mate at each"""
    rng = random.Random(seed)
    lines = []
    for rid, l in enumerate(lens):
        for pos0 in (l - 1, 0):
            for fl in (16, 0, 4):
                lines.append(placed(b"e%d_%d_%d" % (rid, pos0, fl), rid, pos0, l - pos0, rng, flag=fl))
    return records_of(lines, len(lens))


def key_of(rec, lens):
    """the packed key as the entry documents it"""
    pos_bits, n_ref = max(lens, default=0).bit_length(), len(lens)
    r, p, s = sp.sort_key(rec, n_ref)
    return r << (pos_bits + 1) | p << 1 | s


def key_bits(lens):
    return len(lens).bit_length() + max(lens, default=0).bit_length() + 1


def expect(records, lens, P, file_off, coff=None):
    """-> (the sorted records, the BAI of their stream framed in stored blocks of P -- or in blocks at coff)"""
    srt = sp.sort_records(records, len(lens))
    off, size = sp.offsets_of(srt)
    return srt, sp.build_bai(srt, off, coff if coff is not None else sp.stored_offsets(size, P), P, file_off, len(lens))


def regions(lens, seed, per_contig=3):
    """a few regions per contig: its start, its end, and random ones"""
    rng = random.Random(seed)
    out = []
    for rid, l in enumerate(lens):
        out += [(rid, 0, min(l, 200)), (rid, max(l - 200, 0), l)]
        for _ in range(per_contig - 2):
            a = rng.randrange(l)
            out.append((rid, a, min(l, a + rng.randrange(1, 40000))))
    return out


def with_block_size(rec: bytes, block_size: int) -> bytes:
    """the record with another block_size in front of the same bytes (cut or padded to it)"""
    body = rec[4: 4 + block_size] + bytes(max(0, block_size - (len(rec) - 4)))
    return struct.pack("<I", block_size) + body


def with_ref_id(rec: bytes, rid: int) -> bytes:
    return rec[:4] + struct.pack("<i", rid) + rec[8:]


def with_pos(rec: bytes, pos0: int) -> bytes:
    return rec[:8] + struct.pack("<i", pos0) + rec[12:]
