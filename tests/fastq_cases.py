"""The FASTQ texts the fastq tests share, the recording of what the reference's own parser made of them
(tests/golden/fastq_cases.npz), and the call of that parser where oracle/_ref/libbwaref.so exists.

CASES: name -> (text1, text2 or None, flags): well-formed texts (the flags always include FINAL).  CUT_CASES: name -> text whose last
record is malformed in a way at which kseq_read stops too (it returns -2): the record index a parse reports equals the number of
records bseq_read returns.  `python tests/fastq_cases.py` writes the recording (needs the reference build)."""
import ctypes as C
import os
import tempfile

import numpy as np

import fastq_plain as fp

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "fastq_cases.npz")
LETTERS = b"ACGT"


def rec(name, seq, qual=None, eol=b"\n", plus=b"+", comment=b""):
    qual = bytes(33 + (7 * k + len(seq)) % 40 for k in range(len(seq))) if qual is None else qual
    return b"@" + name + comment + eol + seq + eol + plus + eol + qual + eol


def seq_of(rng, n, alphabet=LETTERS):
    return bytes(alphabet[k] for k in rng.integers(0, len(alphabet), n))


def records(rng, n, lo=1, hi=40, tag=b"r", suffix=b""):
    return b"".join(rec(tag + str(k).encode() + suffix, seq_of(rng, int(rng.integers(lo, hi + 1)))) for k in range(n))


def newline_at(rng, p):
    """a text whose first header line ends with its '\\n' at byte p, followed by three ordinary records"""
    name = b"n" * min(p - 1, 20)
    comment = b" " + b"c" * (p - 2 - len(name)) if p - 1 > len(name) else b""
    head = b"@" + name + comment
    assert len(head) == p
    return head + b"\n" + b"ACGTAC\n+\nIIIIII\n" + records(rng, 3)


def of_length(rng, total):
    """a text of exactly `total` bytes: records, the last one stretched to fit"""
    body = records(rng, 8, 20, 60)
    room = total - len(body)
    k = (room - len(b"@z\n\n+\n\n")) // 2
    last = rec(b"z" + b"y" * ((room - len(b"@z\n\n+\n\n")) % 2), seq_of(rng, k))
    assert k > 0 and len(body + last) == total
    return body + last


def build_cases():
    rng = np.random.default_rng(20240611)
    F = fp.FINAL
    c = {}
    for p in (15, 16, 1023, 1024, 4095, 4096):
        c[f"newline_at_{p}"] = (newline_at(rng, p), None, F)
    for n in (1023, 1024, 1025):
        c[f"length_{n}"] = (of_length(rng, n), None, F)
    c["long_header"] = (rec(b"long", b"ACGTN", comment=b"\t" + b"x" * 1094) + records(rng, 2), None, F)
    c["one_and_256"] = (rec(b"one", b"G") + rec(b"many", seq_of(rng, 256)) + rec(b"one_more", b"t"), None, F)
    for n in (0, 1, 63, 64, 65, 257):
        c[f"count_{n}"] = (records(rng, n, 1, 12), None, F)
    c["crlf"] = (b"".join(rec(b"w" + str(k).encode(), seq_of(rng, 5 + k), eol=b"\r\n") for k in range(5)), None, F)
    c["lone_cr"] = (rec(b"a", b"ACGT") + b"@cr\n\r\n+\n\r\n" + rec(b"b", b"TTGA"), None, F)
    c["comments"] = (rec(b"s1", b"ACGT", comment=b" a comment/1") + rec(b"t1", b"ACG", comment=b"\tBC:Z:ACGT") + rec(b"v", b"AC", comment=b"\x0bv") +
                     rec(b"f/2", b"GG", comment=b"\x0cf"), None, F)
    c["names"] = (b"".join(rec(n, seq_of(rng, 7)) for n in (b"a/1", b"/1", b"x/", b"ab/9", b"ab/x", b"q", b"a/b/2", b"//3", b"@@/0")), None, F)
    c["quality_at_plus"] = (rec(b"q1", b"ACGTA", qual=b"@IIII") + rec(b"q2", b"CCGTA", qual=b"+IIII") + rec(b"q3", b"A", qual=b"@") +
                            rec(b"q4", b"C", qual=b"+"), None, F)
    c["plus_repeats_name"] = (rec(b"p1", b"ACGTT", plus=b"+p1") + rec(b"p2", b"ACGTG", plus=b"+p2 with a comment"), None, F)
    c["bases"] = (rec(b"lower", b"acgtn") + rec(b"iupac", b"RYKMSWBDHVNrykmswbdhvn") + rec(b"dots", b"A.C.G.T.") + rec(b"odd", b"UuXx*=\x7f\xc3"), None, F)
    c["no_final_newline"] = ((records(rng, 3) + rec(b"last", b"ACGTACGT"))[:-1], None, F)
    c["no_final_newline_crlf"] = ((records(rng, 2) + rec(b"last", b"ACGTACGT", eol=b"\r\n"))[:-2], None, F)
    r1, r2 = np.random.default_rng(7), np.random.default_rng(8)
    c["pairs_65_70"] = (records(r1, 65, 1, 30, b"pair", b"/1"), records(r2, 70, 1, 30, b"pair", b"/2"), F)
    c["pairs_plain_names"] = (records(r1, 9, 1, 30, b"same"), records(r2, 9, 1, 30, b"same"), F)
    c["interleaved_odd"] = (b"".join(rec(b"il" + str(k // 2).encode() + (b"/1", b"/2")[k & 1], seq_of(rng, 4 + k)) for k in range(7)),
                            None, F | fp.INTERLEAVED | fp.PAIR_NAMES)
    return c


def build_cut_cases():
    rng = np.random.default_rng(99)
    head = records(rng, 5)
    return {
        "quality_longer": head + b"@bad\nACGT\n+\nIIIII\n" + records(rng, 2),
        "quality_missing": head + records(rng, 2) + b"@bad\nACGT\n+\n",
        "plus_line_open": head + b"@bad\nACGT\n+",
    }


CASES = build_cases()
CUT_CASES = build_cut_cases()


# ---- the reference's parser ---------------------------------------------------------------------------------------------------
class _Bseq1(C.Structure):  # bseq1_t
    _fields_ = [("l_seq", C.c_int), ("name", C.c_char_p), ("comment", C.c_char_p), ("seq", C.c_char_p), ("qual", C.c_char_p), ("sam", C.c_char_p)]


def ref_bseq_read(ref_so, text1, text2=None):
    """bseq_read over the whole of one or two texts -> [(l_seq, name, seq, qual)]"""
    lib = C.CDLL(ref_so)
    lib.gzopen.restype = C.c_void_p
    lib.gzopen.argtypes = [C.c_char_p, C.c_char_p]
    lib.gzclose.argtypes = [C.c_void_p]
    lib.kseq_init.restype = C.c_void_p
    lib.kseq_init.argtypes = [C.c_void_p]
    lib.kseq_destroy.argtypes = [C.c_void_p]
    lib.bseq_read.restype = C.POINTER(_Bseq1)
    lib.bseq_read.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
    with tempfile.TemporaryDirectory() as d:
        files, seqs = [], []
        for k, t in enumerate((text1, text2)):
            if t is None:
                continue
            path = os.path.join(d, f"t{k}.fq")
            with open(path, "wb") as f:
                f.write(t)
            fpz = lib.gzopen(path.encode(), b"r")
            assert fpz
            files.append(fpz)
            seqs.append(lib.kseq_init(fpz))
        n = C.c_int(0)
        got = lib.bseq_read(2**31 - 1, C.byref(n), seqs[0], seqs[1] if len(seqs) == 2 else None)
        out = [(int(got[i].l_seq), got[i].name, got[i].seq, got[i].qual or b"") for i in range(n.value)]
        for s, f in zip(seqs, files):
            lib.kseq_destroy(s)
            lib.gzclose(f)
    return out


# ---- the recording ---------------------------------------------------------------------------------------------------------------
def _pack(items):
    off = np.zeros(len(items) + 1, np.int64)
    off[1:] = np.cumsum([len(b) for b in items])
    return np.frombuffer(b"".join(items), np.uint8), off


def _unpack(data, off):
    raw = data.tobytes()
    return [raw[int(off[k]): int(off[k + 1])] for k in range(len(off) - 1)]


def record(ref_so, path=GOLDEN):
    out = {}
    names = list(CASES) + list(CUT_CASES)
    out["case_names"], out["case_names_off"] = _pack([n.encode() for n in names])
    for k, name in enumerate(names):
        t1, t2, _ = CASES[name] if name in CASES else (CUT_CASES[name], None, 0)
        got = ref_bseq_read(ref_so, t1, t2)
        out[f"c{k}_text1"] = np.frombuffer(t1, np.uint8)
        out[f"c{k}_text2"] = np.frombuffer(t2 or b"", np.uint8)
        out[f"c{k}_two"] = np.array([t2 is not None], np.int32)
        out[f"c{k}_l_seq"] = np.array([g[0] for g in got], np.int32)
        for j, field in enumerate(("name", "seq", "qual")):
            out[f"c{k}_{field}"], out[f"c{k}_{field}_off"] = _pack([g[1 + j] for g in got])
    np.savez_compressed(path, **out)
    return path


def load(path=GOLDEN):
    """name -> dict(text1, text2 (None or bytes), l_seq, names, seqs, quals) as recorded"""
    z = np.load(path)
    cases = {}
    for k, name in enumerate(_unpack(z["case_names"], z["case_names_off"])):
        cases[name.decode()] = dict(
            text1=z[f"c{k}_text1"].tobytes(), text2=z[f"c{k}_text2"].tobytes() if int(z[f"c{k}_two"][0]) else None,
            l_seq=z[f"c{k}_l_seq"], names=_unpack(z[f"c{k}_name"], z[f"c{k}_name_off"]),
            seqs=_unpack(z[f"c{k}_seq"], z[f"c{k}_seq_off"]), quals=_unpack(z[f"c{k}_qual"], z[f"c{k}_qual_off"]))
    return cases


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
    import pyoracle
    print(record(pyoracle.REF_SO), os.path.getsize(GOLDEN), "bytes")
