"""A plain Python parser of four-line FASTQ, the yardstick of the fastq tests: bytes.split(b"\\n"), groups of four, split() for the
name, a dict for the base codes.  It shares nothing with csrc/bpsw_fastq_core.h; tests/test_fastq_core_host.py pins it on what the
reference's own bseq_read returned for the recorded cases (tests/golden/fastq_cases.npz).

parse() returns the six arrays of bpsw_fastq_parse with n_reads and consumed, or raises Refused with the read index, the record, the
text (1 or 2) and a key for the reason."""
import numpy as np

FINAL, INTERLEAVED, PAIR_NAMES, HOST = 1, 2, 4, 8
CODES = {ord(c): k for k, pair in enumerate(("Aa", "Cc", "Gg", "Tt")) for c in pair}

# reason key -> the fixed words of bpsw_last_error
REASON_TEXT = {
    "no_at": "the header line does not begin with '@' (not four-line FASTQ)",
    "no_plus": "the third line does not begin with '+' (not four-line FASTQ)",
    "empty_read": "the read is empty",
    "len_diff": "the quality line is not as long as the read",
    "empty_name": "the name is empty",
    "dash": "'-' in the read",
    "low_byte": "a byte below 4 in the read",
    "pair_name": "the name differs from the first end's",
    "truncated": "the text ends inside the record (not four-line FASTQ)",
}


class Refused(Exception):
    def __init__(self, read, record, text, key, pairs):
        self.read, self.record, self.text, self.key, self.pairs = read, record, text, key, pairs
        super().__init__(self.message("fastq_parse"))

    def message(self, who):
        pair = f" (pair {self.read // 2})" if self.pairs else ""
        return f"{who}: record {self.record} of text {self.text}{pair}: {REASON_TEXT[self.key]}"


def _lines(text, final):
    """the text's lines without their '\\n' (a last line without one only when final), and the number of whole lines"""
    parts = text.split(b"\n")
    lines, rest = parts[:-1], parts[-1]
    if final and rest:
        lines.append(rest)
    return lines


def _strip_cr(line):
    return line[:-1] if len(line) > 1 and line.endswith(b"\r") else line


def _name(header):
    body = header[1:]
    if not body or body[:1].isspace():
        return b""
    name = body.split()[0]
    if len(name) > 2 and name[-2:-1] == b"/" and name[-1:].isdigit():
        name = name[:-2]
    return name


def _record(four):
    """(name, read, quality) of four lines, or the key of the first rule they break"""
    header, seq, plus, qual = four
    if not header.startswith(b"@"):
        return "no_at"
    if not plus.startswith(b"+"):
        return "no_plus"
    seq, qual = _strip_cr(seq), _strip_cr(qual)
    if not seq:
        return "empty_read"
    if len(qual) != len(seq):
        return "len_diff"
    name = _name(header)
    if not name:
        return "empty_name"
    if b"-" in seq:
        return "dash"
    if any(b < 4 for b in seq):
        return "low_byte"
    return name, seq, qual


def parse(text1, text2=None, flags=0):
    final = bool(flags & FINAL)
    texts = [text1 or b""] + ([text2] if text2 is not None else [])
    two = len(texts) == 2
    pairs = two or bool(flags & PAIR_NAMES)
    lines = [_lines(t, final) for t in texts]
    recs = [len(ls) // 4 for ls in lines]
    if two:
        used = [min(recs)] * 2
        order = [(k & 1, k >> 1) for k in range(2 * used[0])]
    else:
        used = [recs[0] - (recs[0] & 1 if flags & INTERLEAVED else 0)]
        order = [(0, k) for k in range(used[0])]
    out = []
    for i, (t, r) in enumerate(order):
        got = _record(lines[t][4 * r: 4 * r + 4])
        if isinstance(got, str):
            raise Refused(i, r, t + 1, got, pairs)
        if pairs and i & 1 and got[0] != out[i - 1][0]:
            raise Refused(i, r, t + 1, "pair_name", pairs)
        out.append(got)
    if final:
        cut = [(2 * (len(ls) // 4) + t if two else len(ls) // 4, t) for t, ls in enumerate(lines) if len(ls) % 4]
        if cut:
            i, t = min(cut)
            raise Refused(i, len(lines[t]) // 4, t + 1, "truncated", pairs)
    consumed = [min(sum(len(l) + 1 for l in ls[: 4 * u]), len(t)) for ls, u, t in zip(lines, used, texts)] + [0] * (2 - len(texts))
    read_len = np.array([len(s) for _, s, _ in out], np.int32)
    read_off = np.zeros(len(out), np.int64)
    read_off[1:] = np.cumsum(read_len)[:-1]
    names = [n for i, (n, _, _) in enumerate(out) if not (pairs and i & 1)]
    name_off = np.zeros(len(names) + 1, np.int64)
    name_off[1:] = np.cumsum([len(n) for n in names])
    return dict(n_reads=len(out), consumed=tuple(consumed), read_len=read_len, read_off=read_off,
                read_pool=np.array([CODES.get(b, 4) for _, s, _ in out for b in s], np.uint8),
                qual_pool=np.frombuffer(b"".join(q for _, _, q in out), np.uint8),
                name_off=name_off, name_pool=np.frombuffer(b"".join(names), np.uint8),
                names=names, reads=[s for _, s, _ in out], quals=[q for _, _, q in out])
