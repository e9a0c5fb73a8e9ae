"""The case table of the BGZF inflate (csrc/bpsw_inflate_core.h), shared by tests/test_inflate_core_host.py (the host twin under the
sanitizers) and tests/test_bgzf_in_gpu.py (the device against the twin and zlib).

A case is a chunk of BGZF blocks and what it must give: the inflated bytes (zlib's, checked through bam_plain.bgzf_members when the
case is built), or the (block, reason) of the refusal.  The streams come from zlib at settings chosen for what they make zlib emit,
from the library's own deflate twin, and from a small bit writer for what no encoder emits.  Every case asserts through walk_deflate --
a plain-Python reader of deflate data that reports the block types, the longest literal/length code, the repeat symbols, the largest
distance, overlapping matches and matches of 258 -- that its stream has the property it is named for: with another zlib build a case
fails here instead of quietly testing something else."""
import functools
import gzip
import os
import random
import struct
import zlib

import bam_plain as bp

Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED = 2, 3, 4
P0 = 65280

# the reasons, in the order of inflcore::Reason (index == code)
REASONS = ["OK", "MAGIC", "NO_BC", "BSIZE", "ISIZE", "BTYPE", "STORED_LEN", "HLIT", "HDIST", "CL_OVER", "CL_INCOMPLETE", "REPEAT_FIRST", "RUN_PAST",
           "NO_EOB", "LL_OVER", "LL_INCOMPLETE", "D_OVER", "D_INCOMPLETE", "BAD_CODE", "LL_SYMBOL", "D_SYMBOL", "DIST_BEFORE", "DATA_ENDS", "TOO_LONG",
           "TOO_SHORT", "CRC"]
R = {name: code for code, name in enumerate(REASONS)}
REASON_TEXT = {
    "MAGIC": "the block does not begin with 1f 8b 08 04 (not a BGZF block)",
    "NO_BC": "no BC subfield in the gzip header (plain gzip, not BGZF)",
    "BSIZE": "BSIZE and the extra field are inconsistent",
    "ISIZE": "ISIZE is above 65536",
    "BTYPE": "a deflate block of type 11",
    "STORED_LEN": "a stored block whose LEN is not the complement of NLEN",
    "HLIT": "HLIT above 286",
    "HDIST": "HDIST above 30",
    "CL_OVER": "the code-length code is over-subscribed",
    "CL_INCOMPLETE": "the code-length code is incomplete",
    "REPEAT_FIRST": "a repeat of the previous length with no length in front",
    "RUN_PAST": "a run of lengths past HLIT + HDIST",
    "NO_EOB": "the literal/length code has no end-of-block symbol",
    "LL_OVER": "the literal/length code is over-subscribed",
    "LL_INCOMPLETE": "the literal/length code is incomplete",
    "D_OVER": "the distance code is over-subscribed",
    "D_INCOMPLETE": "the distance code is incomplete",
    "BAD_CODE": "bits that are no code of the block's",
    "LL_SYMBOL": "literal/length symbol 286 or 287",
    "D_SYMBOL": "distance symbol 30 or 31",
    "DIST_BEFORE": "a distance that reaches in front of the block's output",
    "DATA_ENDS": "the deflate data ends early",
    "TOO_LONG": "the output is longer than ISIZE",
    "TOO_SHORT": "the output is shorter than ISIZE",
    "CRC": "the CRC-32 differs from the trailer's",
}

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


# ---- framing ----------------------------------------------------------------------------------------------------------------------------
def frame(payload: bytes, raw: bytes, extra: bytes = b"", crc=None, isize=None) -> bytes:
    """payload and its raw deflate bytes -> a BGZF block; extra: whole subfields in front of BC"""
    xlen = len(extra) + 6
    total = 12 + xlen + len(raw) + 8
    assert total <= 65536
    head = struct.pack("<BBBBIBBH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, xlen) + extra + struct.pack("<BBHH", 66, 67, 2, total - 1)
    return head + raw + struct.pack("<II", zlib.crc32(payload) if crc is None else crc, len(payload) if isize is None else isize)


def deflate(data: bytes, level=6, strategy=0, mem_level=8, flush_at=None, flush_mode=None) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    if flush_at is None:
        return c.compress(data) + c.flush()
    return c.compress(data[:flush_at]) + c.flush(flush_mode) + c.compress(data[flush_at:]) + c.flush()


def bgzip(data: bytes, payload: int = P0, level: int = 6, eof: bool = False) -> bytes:
    """data cut every `payload` bytes, each piece a block"""
    out = b"".join(frame(data[at: at + payload], deflate(data[at: at + payload], level)) for at in range(0, len(data), payload))
    return out + (bp.EOF_BLOCK if eof else b"")


# ---- a bit writer ----------------------------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value: int, nb: int):
        """a value, its lowest bit first"""
        assert 0 <= value < (1 << nb) or nb == 0
        self.v |= value << self.n
        self.n += nb
        return self

    def code(self, code: int, nb: int):
        """a Huffman code, its first bit first"""
        for k in range(nb - 1, -1, -1):
            self.put((code >> k) & 1, 1)
        return self

    def align(self):
        self.n = (self.n + 7) & ~7
        return self

    def raw(self, data: bytes):
        assert self.n % 8 == 0
        self.v |= int.from_bytes(data, "little") << self.n
        self.n += 8 * len(data)
        return self

    def bytes(self) -> bytes:
        return self.v.to_bytes((self.n + 7) // 8, "little")


def canonical(lens):
    """code lengths -> {symbol: (code, length)} (RFC 1951 3.2.2)"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def put_tokens(b: Bits, tokens, ll_lens, d_lens):
    """tokens: ints (literals, or 256) and (length, distance) pairs, or ("ll", symbol) / ("d", symbol, extra) for a symbol as it is"""
    ll, d = canonical(ll_lens), canonical(d_lens)
    for t in tokens:
        if isinstance(t, int):
            b.code(*ll[t])
        elif t[0] == "ll":
            b.code(*ll[t[1]])
        elif t[0] == "d":
            b.code(*d[t[1]])
            b.put(t[2], DIST_EXTRA[t[1]] if t[1] < 30 else 0)
        else:
            length, dist = t
            k = max(i for i in range(29) if LEN_BASE[i] <= length) if length < 258 else 28
            b.code(*ll[257 + k]).put(length - LEN_BASE[k], LEN_EXTRA[k])
            j = max(i for i in range(30) if DIST_BASE[i] <= dist)
            b.code(*d[j]).put(dist - DIST_BASE[j], DIST_EXTRA[j])
    return b


def fixed_block(tokens, final=True, b=None) -> Bits:
    b = b or Bits()
    b.put(1 if final else 0, 1).put(1, 2)
    return put_tokens(b, tokens, FIXED_LL, FIXED_D)


def stored_block(data: bytes, final=True, b=None, nlen=None) -> Bits:
    b = b or Bits()
    b.put(1 if final else 0, 1).put(0, 2).align()
    b.put(len(data), 16).put((~len(data) & 0xffff) if nlen is None else nlen, 16)
    return b.raw(data)


def complete_cl(used):
    """lengths of a complete code over the symbols `used` (two at least): the shortest of its kind"""
    used = sorted(used)
    k = len(used)
    assert k >= 2
    m = k.bit_length() - 1
    short = (2 << m) - k
    return {s: (m if i < short else m + 1) for i, s in enumerate(used)}


def dynamic_block(ops, tokens=(), ll_lens=None, d_lens=None, cl_lens=None, hlit=None, hdist=None, final=True, b=None) -> Bits:
    """a dynamic block whose header is spelled out: ops are the code-length code's symbols, (symbol, extra value) each; the code-length
    code is complete over the symbols used unless cl_lens ({symbol: length}) says otherwise.  hlit / hdist: the declared counts (taken
    from the lists unless given).  Tokens are written when both lists are given."""
    b = b or Bits()
    cl = cl_lens if cl_lens is not None else complete_cl({s for s, _ in ops} | ({0, 1} if len({s for s, _ in ops}) < 2 else set()))
    lens19 = [cl.get(s, 0) for s in range(19)]
    hclen = max([4] + [k + 1 for k in range(19) if lens19[CL_ORDER[k]]])
    b.put(1 if final else 0, 1).put(2, 2)
    b.put((len(ll_lens) if hlit is None else hlit) - 257, 5).put((len(d_lens) if hdist is None else hdist) - 1, 5).put(hclen - 4, 4)
    for k in range(hclen):
        b.put(lens19[CL_ORDER[k]], 3)
    codes = canonical(lens19)
    for s, extra in ops:
        if s in codes:
            b.code(*codes[s])
            b.put(extra, {16: 2, 17: 3, 18: 7}.get(s, 0))
    if tokens:
        put_tokens(b, tokens, ll_lens, d_lens)
    return b


def plain_ops(lens):
    """a list of lengths as ops without repeat symbols"""
    return [(l, 0) for l in lens]


# ---- a reader of deflate data -------------------------------------------------------------------------------------------------------------
class _In:
    def __init__(self, data):
        self.d, self.at, self.acc, self.n = data, 0, 0, 0

    def bits(self, nb):
        while self.n < nb:
            self.acc |= (self.d[self.at] if self.at < len(self.d) else 0) << self.n
            assert self.at < len(self.d) + 8, "the data ends"
            self.at += 1
            self.n += 8
        v = self.acc & ((1 << nb) - 1)
        self.acc >>= nb
        self.n -= nb
        return v

    def sym(self, dec):
        code, l = 0, 0
        while True:
            code, l = code << 1 | self.bits(1), l + 1
            if (l, code) in dec:
                return dec[(l, code)]
            assert l < 16, "no such code"

    def used_bits(self):
        return 8 * self.at - self.n


def _decoder(lens):
    return {(l, c): s for s, (c, l) in canonical(lens).items()}


def walk_deflate(raw: bytes):
    """-> (the bytes, what was met): btypes (per deflate block), max_ll_len, max_cl_len, repeats (set of 16 / 17 / 18), crossing (a
    repeat that runs from the literal/length lengths into the distance lengths), max_dist, max_dist_sym, overlap (a match with distance <
    length), n258, syms285 (matches through symbol 285), lone_dist (a block with one distance code), off_byte (the data ends inside a
    byte), dists (set)"""
    f, out = _In(raw), bytearray()
    info = dict(btypes=[], max_ll_len=0, max_cl_len=0, repeats=set(), crossing=False, max_dist=0, max_dist_sym=-1, overlap=False, n258=0, syms285=0,
                lone_dist=False, off_byte=False, dists=set())
    while True:
        final, btype = f.bits(1), f.bits(2)
        info["btypes"].append(btype)
        assert btype != 3
        if btype == 0:
            f.bits(f.n & 7)
            n, nn = f.bits(16), f.bits(16)
            assert n ^ nn == 0xffff
            for _ in range(n):
                out.append(f.bits(8))
        else:
            if btype == 1:
                ll, d = FIXED_LL, FIXED_D
            else:
                hlit, hdist, hclen = f.bits(5) + 257, f.bits(5) + 1, f.bits(4) + 4
                cl = [0] * 19
                for k in range(hclen):
                    cl[CL_ORDER[k]] = f.bits(3)
                info["max_cl_len"] = max(info["max_cl_len"], max(cl))
                dec, lens = _decoder(cl), []
                while len(lens) < hlit + hdist:
                    s = f.sym(dec)
                    before = len(lens)
                    if s < 16:
                        lens.append(s)
                        continue
                    info["repeats"].add(s)
                    if s == 16:
                        lens += [lens[-1]] * (3 + f.bits(2))
                    else:
                        lens += [0] * ((3 + f.bits(3)) if s == 17 else (11 + f.bits(7)))
                    info["crossing"] |= before < hlit < len(lens)
                assert len(lens) == hlit + hdist
                ll, d = lens[:hlit], lens[hlit:]
                info["lone_dist"] |= sum(1 for l in d if l) == 1
            info["max_ll_len"] = max(info["max_ll_len"], max(ll))
            dl, dd = _decoder(ll), _decoder(d)
            while True:
                s = f.sym(dl)
                if s < 256:
                    out.append(s)
                    continue
                if s == 256:
                    break
                length = LEN_BASE[s - 257] + f.bits(LEN_EXTRA[s - 257])
                t = f.sym(dd)
                dist = DIST_BASE[t] + f.bits(DIST_EXTRA[t])
                assert dist <= len(out)
                info["max_dist"], info["max_dist_sym"] = max(info["max_dist"], dist), max(info["max_dist_sym"], t)
                info["dists"].add(dist)
                info["overlap"] |= dist < length
                info["n258"] += length == 258
                info["syms285"] += s == 285
                for _ in range(length):
                    out.append(out[-dist])
        if final:
            break
    assert (f.used_bits() + 7) // 8 == len(raw), "bytes behind the last deflate block"
    info["off_byte"] = f.used_bits() % 8 != 0
    return bytes(out), info


# ---- payloads -----------------------------------------------------------------------------------------------------------------------------
def fastq_like(n: int, seed: int = 11) -> bytes:
    rng, out, k = random.Random(seed), bytearray(), 0
    while len(out) < n:
        l = rng.randrange(90, 152)
        out += b"@read%d/1\n" % k + bytes(rng.choice(b"ACGT") for _ in range(l)) + b"\n+\n" + bytes(rng.choice(b"FFFFF:,#") for _ in range(l)) + b"\n"
        k += 1
    return bytes(out[:n])


def fibonacci_bytes() -> bytes:
    """46 367 bytes: 22 values with the counts 1, 1, 2, 3, ..., 17711, shuffled: a Huffman tree more than 15 bits deep"""
    f, vals = [1, 1], []
    while len(f) < 22:
        f.append(f[-1] + f[-2])
    for k, c in enumerate(f):
        vals += [k + 40] * c
    assert len(vals) == 46367
    random.Random(5).shuffle(vals)
    return bytes(vals)


class Case:
    def __init__(self, name, chunk, want=None, bad=None, n_blocks=None, consumed=None, header=False):
        self.name, self.chunk, self.want, self.bad = name, chunk, want, bad
        self.n_blocks, self.consumed, self.header = n_blocks, consumed, header   # header: the refusal is the walk's

    def __repr__(self):
        return self.name


def _ok(name, payload, raw, check=None, extra=b""):
    """an accepted one-block case; check(info) asserts what the stream is named for"""
    got, info = walk_deflate(raw)
    assert got == payload, name
    if check:
        assert check(info), (name, {k: v for k, v in info.items() if k != "dists"}, sorted(info["dists"])[-3:])
    chunk = frame(payload, raw, extra)
    if not extra:
        assert bp.bgzf_inflate(chunk) == payload
    else:
        assert zlib.decompress(raw, -15) == payload
    c = Case(name, chunk, want=payload, n_blocks=1, consumed=len(chunk))
    c.info = info
    return c


def _bad(name, raw, reason, payload=b"", crc=None, isize=None, zlib_refuses=True):
    if zlib_refuses:
        try:
            d = zlib.decompressobj(-15)
            d.decompress(raw)
            assert not d.eof, name + ": zlib takes this stream"
        except zlib.error:
            pass
    return Case(name, frame(payload, raw, crc=crc, isize=isize), bad=(0, R[reason]), n_blocks=1)


def _library_frames():
    """the library's own deflate twin (block_serial) over a golden record stream at the payload sizes of test_deflate_core_host.py"""
    import test_deflate_core_host as tdh
    exe = tdh.build_host(False)
    data = tdh.golden_stream("mem_sam_pe")
    return [(p, data[: min(len(data), 40 * p)]) for p in tdh.PAYLOADS], tdh, exe


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    text = fastq_like(P0)
    # ---- zlib at the settings that make it emit what the names say ------------------------------------------------------------------------
    for level in (1, 6, 9):
        out.append(_ok("zlib_level%d" % level, text, deflate(text, level),
                       lambda i: set(i["btypes"]) == {2} and i["max_ll_len"] > 10 and i["repeats"] >= {17, 18}
                       and i["max_dist"] > 30000 and i["overlap"]))
    assert set().union(*(c.info["repeats"] for c in out)) == {16, 17, 18}
    out.append(_ok("zlib_fixed", text[:20000], deflate(text[:20000], 6, Z_FIXED), lambda i: set(i["btypes"]) == {1}))
    out.append(_ok("zlib_level0", text, deflate(text, 0), lambda i: set(i["btypes"]) == {0} and len(i["btypes"]) >= 2))
    out.append(_ok("zlib_memlevel1", text, deflate(text, 6, 0, 1), lambda i: len(i["btypes"]) > 64))
    for name, mode in (("full", zlib.Z_FULL_FLUSH), ("sync", zlib.Z_SYNC_FLUSH)):
        out.append(_ok("zlib_%s_flush" % name, text, deflate(text, 6, flush_at=30000, flush_mode=mode),
                       lambda i: 0 in i["btypes"][1:-1] and i["btypes"][0] == 2 and i["btypes"][-1] == 2))
    out.append(_ok("zlib_rle", text, deflate(text, 6, Z_RLE), lambda i: i["dists"] <= {1}))
    out.append(_ok("zeros_65280", bytes(65280), deflate(bytes(65280), 6), lambda i: i["n258"] >= 250 and i["dists"] == {1} and i["overlap"]))
    out.append(_ok("zeros_65536", bytes(65536), deflate(bytes(65536), 6), lambda i: i["n258"] >= 250 and i["dists"] == {1}))
    fib = fibonacci_bytes()
    out.append(_ok("fibonacci_huffman_only", fib, deflate(fib, 6, Z_HUFFMAN_ONLY), lambda i: i["max_ll_len"] == 15 and i["max_dist"] == 0))
    out.append(_ok("empty", b"", deflate(b"", 6), lambda i: i["btypes"] == [1]))
    assert len(deflate(b"", 6)) == 2 and len(deflate(b"x", 6)) == 3
    out.append(_ok("one_byte", b"x", deflate(b"x", 6), lambda i: i["btypes"] == [1]))
    rnd = random.Random(3).randbytes(65000)
    out.append(_ok("random_65000_stored", rnd, deflate(rnd, 6), lambda i: set(i["btypes"]) == {0}))
    for n in (15, 16, 17, 65535):
        out.append(_ok("isize_%d" % n, text[:n], deflate(text[:n], 6)))
    # ---- what no encoder emits, by the bit writer -----------------------------------------------------------------------------------------
    head = random.Random(4).randbytes(32768)
    b = stored_block(head, final=False)
    fixed_block([(258, 32768), 256], b=b)
    out.append(_ok("distance_32768_length_258", head + head[:258], b.bytes(),
                   lambda i: i["max_dist"] == 32768 and i["max_dist_sym"] == 29 and i["syms285"] == 1 and i["btypes"] == [0, 1]))
    ll = [0] * 258
    ll[97] = ll[98] = ll[256] = ll[257] = 2
    ops = [(18, 86), (2, 0), (2, 0), (18, 127), (18, 8), (2, 0), (16, 2)]   # 97 zeros, a, b, 157 zeros, 256, then 257 and four distances
    b = dynamic_block(ops, [97, 98, (3, 2), (3, 1), 256], ll, [2, 2, 2, 2])
    out.append(_ok("run_crosses_into_the_distances", b"ababaaaa", b.bytes(), lambda i: i["crossing"] and i["repeats"] == {16, 18}))
    ll = [0] * 258
    ll[97], ll[256], ll[257] = 1, 2, 2
    b = dynamic_block(plain_ops(ll + [1]), [97, (3, 1), 256], ll, [1])
    out.append(_ok("one_distance_code_of_one_bit", b"aaaa", b.bytes(), lambda i: i["lone_dist"]))
    b = dynamic_block(plain_ops(ll + [0]), [97, 97, 256], ll, [0])
    out.append(_ok("no_distance_code", b"aa", b.bytes()))
    b = fixed_block([97, 98, 99, 256], final=False)
    stored_block(b"", final=False, b=b)
    fixed_block([(3, 3), 256], b=b)
    out.append(_ok("match_reaches_over_block_borders", b"abcabc", b.bytes(), lambda i: i["btypes"] == [1, 0, 1]))
    # ---- a second subfield in front of BC -----------------------------------------------------------------------------------------------
    out.append(_ok("extra_subfield_first", text[:3000], deflate(text[:3000], 6), extra=struct.pack("<BBH", 88, 89, 5) + b"hello"))
    out.append(_ok("extra_subfield_empty", text[:100], deflate(text[:100], 6), extra=struct.pack("<BBH", 1, 2, 0)))
    # ---- the library's own blocks ----------------------------------------------------------------------------------------------------------
    frames, tdh, exe = _library_frames()
    for (p, data), framed in zip(frames, tdh.run_host(exe, frames, "inflate_cases")):
        members = bp.bgzf_members(framed)
        assert b"".join(m[0] for m in members) == data and (p < 1021 or any(m[2][0] & 7 == 5 for m in members))
        out.append(Case("library_deflate_%d" % p, framed, want=data, n_blocks=len(members), consumed=len(framed)))
    # ---- a reason each ------------------------------------------------------------------------------------------------------------------------
    out.append(_bad("btype_11", Bits().put(1, 1).put(3, 2).bytes(), "BTYPE"))
    out.append(_bad("stored_len", stored_block(b"abc", nlen=0x1234).bytes(), "STORED_LEN", b"abc"))
    ll = [0] * 258
    ll[97], ll[256], ll[257] = 1, 2, 2
    out.append(_bad("hlit_287", dynamic_block(plain_ops(ll + [1]), hlit=287, hdist=1).bytes(), "HLIT"))
    out.append(_bad("hdist_31", dynamic_block(plain_ops(ll + [1]), hlit=258, hdist=31).bytes(), "HDIST"))
    out.append(_bad("cl_over", dynamic_block([], cl_lens={0: 1, 1: 1, 2: 1}, hlit=258, hdist=1).bytes(), "CL_OVER"))
    out.append(_bad("cl_incomplete", dynamic_block([], cl_lens={0: 1, 1: 2}, hlit=258, hdist=1).bytes(), "CL_INCOMPLETE"))
    out.append(_bad("cl_lone_code", dynamic_block([], cl_lens={0: 1}, hlit=258, hdist=1).bytes(), "CL_INCOMPLETE"))
    out.append(_bad("repeat_first", dynamic_block([(16, 0), (1, 0)], hlit=258, hdist=1).bytes(), "REPEAT_FIRST"))
    out.append(_bad("run_past", dynamic_block([(18, 127), (18, 127)], hlit=258, hdist=1).bytes(), "RUN_PAST"))
    no_eob = [0] * 258
    no_eob[97] = no_eob[98] = 1
    out.append(_bad("no_eob", dynamic_block(plain_ops(no_eob + [1]), hlit=258, hdist=1).bytes(), "NO_EOB"))
    over = list(ll)
    over[98] = 1
    out.append(_bad("ll_over", dynamic_block(plain_ops(over + [1]), hlit=258, hdist=1).bytes(), "LL_OVER"))
    inc = list(ll)
    inc[257] = 0
    out.append(_bad("ll_incomplete", dynamic_block(plain_ops(inc + [1]), hlit=258, hdist=1).bytes(), "LL_INCOMPLETE"))
    lone = [0] * 258
    lone[256] = 1
    out.append(_bad("ll_lone_code", dynamic_block(plain_ops(lone + [1]), hlit=258, hdist=1).bytes(), "LL_INCOMPLETE", zlib_refuses=False))
    out.append(_bad("d_over", dynamic_block(plain_ops(ll + [1, 1, 1]), hlit=258, hdist=3).bytes(), "D_OVER"))
    out.append(_bad("d_incomplete", dynamic_block(plain_ops(ll + [1, 2]), hlit=258, hdist=2).bytes(), "D_INCOMPLETE"))
    out.append(_bad("d_lone_code_of_two_bits", dynamic_block(plain_ops(ll + [2]), hlit=258, hdist=1).bytes(), "D_INCOMPLETE"))
    b = dynamic_block(plain_ops(ll + [1]), [97, ("ll", 257)], ll, [1]).put(1, 1)   # the one distance code is 0: a 1 is none
    put_tokens(b, [256], ll, [1])
    out.append(_bad("bad_code", b.bytes(), "BAD_CODE", b"aaaa"))
    out.append(_bad("ll_symbol_286", fixed_block([97, ("ll", 286), 256]).bytes(), "LL_SYMBOL", b"a"))
    out.append(_bad("d_symbol_30", fixed_block([97, ("ll", 257), ("d", 30, 0), 256]).bytes(), "D_SYMBOL", b"aaaa"))
    out.append(_bad("distance_before", fixed_block([97, (3, 2), 256]).bytes(), "DIST_BEFORE", b"aaaa"))
    out.append(_bad("distance_before_in_second_block", fixed_block([(3, 2), 256], b=fixed_block([97, 256], final=False)).bytes(),
                    "DIST_BEFORE", b"aaaa"))
    out.append(_bad("data_ends_no_eob", fixed_block([97, 98, 99]).bytes(), "DATA_ENDS", b"abc"))
    out.append(_bad("data_ends_not_final", fixed_block([97, 256], final=False).bytes(), "DATA_ENDS", b"a"))
    out.append(_bad("data_ends_stored", stored_block(b"abcdef").bytes()[:-2], "DATA_ENDS", b"abcdef"))
    out.append(_bad("data_ends_nothing", b"", "DATA_ENDS"))
    z = deflate(text[:5000], 6)
    out.append(_bad("too_long_literal", z, "TOO_LONG", text[:5000], isize=4999, zlib_refuses=False))
    out.append(_bad("too_long_match", deflate(bytes(1000), 6), "TOO_LONG", bytes(1000), isize=999, zlib_refuses=False))
    out.append(_bad("too_long_stored", stored_block(b"abcdef").bytes(), "TOO_LONG", b"abcdef", isize=5, zlib_refuses=False))
    out.append(_bad("too_short", z, "TOO_SHORT", text[:5000], isize=5001, zlib_refuses=False))
    out.append(_bad("crc", z, "CRC", text[:5000], crc=zlib.crc32(text[:5000]) ^ 0x100, zlib_refuses=False))
    # ---- headers ----------------------------------------------------------------------------------------------------------------------------
    good = frame(text[:500], deflate(text[:500], 6))
    plain = gzip.compress(text[:500], mtime=0)
    out.append(Case("header_magic", b"BAM\1" + good[4:], bad=(0, R["MAGIC"]), n_blocks=0, header=True))
    out.append(Case("header_plain_gzip", plain, bad=(0, R["NO_BC"]), n_blocks=0, header=True))
    out.append(Case("header_plain_gzip_behind_a_block", good + plain, bad=(1, R["NO_BC"]), n_blocks=1, header=True))
    other = struct.pack("<BBBBIBBH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6) + struct.pack("<BBHH", 88, 89, 2, 7) + deflate(b"", 6) + bytes(8)
    out.append(Case("header_extra_without_bc", other, bad=(0, R["NO_BC"]), n_blocks=0, header=True))
    out.append(Case("header_bsize_too_small", good[:16] + struct.pack("<H", 20) + good[18:], bad=(0, R["BSIZE"]), n_blocks=0, header=True))
    out.append(Case("header_bc_slen_4", good[:14] + struct.pack("<H", 4) + good[16:], bad=(0, R["BSIZE"]), n_blocks=0, header=True))
    out.append(Case("header_isize_65537", frame(b"", deflate(b"", 6), isize=65537), bad=(0, R["ISIZE"]), n_blocks=0, header=True))
    out.append(Case("header_name_flag", good[:3] + b"\x0c" + good[4:], bad=(0, R["MAGIC"]), n_blocks=0, header=True))
    # ---- chunks that end inside a block -------------------------------------------------------------------------------------------------------
    two = bgzip(text[:3000], 1500)
    third = frame(text[3000:3100], deflate(text[3000:3100], 6))
    for name, cut in (("one_byte_into_the_header", 1), ("eleven_bytes_into_the_header", 11), ("inside_the_extra_field", 14),
                      ("one_byte_short_of_the_trailer_end", len(third) - 1)):
        out.append(Case("chunk_cut_" + name, two + third[:cut], want=text[:3000], n_blocks=2, consumed=len(two)))
    out.append(Case("chunk_cut_at_the_end", two + third, want=text[:3100], n_blocks=3, consumed=len(two) + len(third)))
    out.append(Case("chunk_empty", b"", want=b"", n_blocks=0, consumed=0))
    out.append(Case("chunk_lone_eof", bp.EOF_BLOCK, want=b"", n_blocks=1, consumed=28))
    out.append(Case("chunk_with_eof", two + bp.EOF_BLOCK, want=text[:3000], n_blocks=3, consumed=len(two) + 28))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def accepted():
    return [c for c in cases() if c.bad is None]


def refused():
    return [c for c in cases() if c.bad is not None]


# ---- the twin as a program (tests/inflate_host/inflate_host.cpp) ----------------------------------------------------------------------------
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "inflate_host", "inflate_host.cpp")
CSRC = os.path.join(ROOT, "cloud-scale-bwamem_amd", "csrc")
HDRS = [os.path.join(CSRC, h) for h in ("bpsw_inflate_core.h", "bpsw_deflate_core.h", "bpsw_bam_core.h", "bpsw_sam_core.h")]
OUT = os.path.join(HERE, "inflate_host", "_build")


def build_host(sanitize=True):
    """-> the program's path (built when it is older than its sources)"""
    import subprocess
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "inflate_host_san" if sanitize else "inflate_host")
    if not (os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(p) for p in [SRC] + HDRS)):
        san = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
               "-static-libubsan"] if sanitize else ["-O2"]
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function"] + san + ["-I" + CSRC, "-o", exe, SRC], check=True)
    return exe


def run_host(exe, chunks, tag):
    """chunks -> per chunk dict(n_blocks, consumed, total, bad_block, reason, header, blocks: [(coff, data_off, data_len, isize, crc,
    out_off)], data: the bytes or None)"""
    import subprocess
    src, dst = os.path.join(OUT, tag + ".in"), os.path.join(OUT, tag + ".out")
    with open(src, "wb") as f:
        for c in chunks:
            f.write(struct.pack("<I", len(c)) + c)
    r = subprocess.run([exe, "run", src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    blob, at, out = open(dst, "rb").read(), 0, []
    for _ in chunks:
        nb, consumed, total, bad, reason, header = struct.unpack_from("<IqqqiI", blob, at)
        at += 36
        blocks = [struct.unpack_from("<6I", blob, at + 24 * k) for k in range(nb)]
        at += 24 * nb
        data = None
        if not reason:
            data = blob[at: at + total]
            at += total
        out.append(dict(n_blocks=nb, consumed=consumed, total=total, bad_block=bad, reason=reason, header=bool(header), blocks=blocks, data=data))
    assert at == len(blob)
    return out


def run_trunc(exe, items, tag):
    """items: [(one block, [lengths its deflate data is cut to])] -> per item the reasons"""
    import subprocess
    src, dst = os.path.join(OUT, tag + ".in"), os.path.join(OUT, tag + ".out")
    with open(src, "wb") as f:
        for chunk, cuts in items:
            f.write(struct.pack("<II", len(chunk), len(cuts)) + chunk + struct.pack("<%dI" % len(cuts), *cuts))
    r = subprocess.run([exe, "trunc", src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    blob, at, out = open(dst, "rb").read(), 0, []
    for _, cuts in items:
        out.append(list(blob[at: at + len(cuts)]))
        at += len(cuts)
    assert at == len(blob)
    return out
