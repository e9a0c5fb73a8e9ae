"""FASTQ text to reads on the device (bpsw_fastq_parse) and FASTQ text to SAM text (bpsw_align_fastq_se / _pe).

Every case runs through the kernels of csrc/bpsw_fastq.hip and through BPSW_FASTQ_HOST; the six output arrays, n_reads and consumed
are compared with two yardsticks that are not the code under test: the plain Python parser (tests/fastq_plain.py) and what the
reference's own bseq_read returned for the same text (tests/golden/fastq_cases.npz, recorded by tests/fastq_cases.py; live in
tests/test_fastq_core_host.py where the reference build exists).  The refusals are a table of (input, code, exact error text)."""
import ctypes as C

import numpy as np
import pytest

import bpsw_hip
import fastq_cases as fc
import fastq_plain as fp
from test_sam_pe_gpu import PAIR_ORDER, _group_of
from test_sam_se_gpu import NO_PES, TEXT_MODES, _contig_tables, _load, fixture_reads, gold  # noqa: F401
from test_worker1_gpu import _opt

pytestmark = pytest.mark.gpu

ARRAYS = ("read_len", "read_off", "read_pool", "qual_pool", "name_off", "name_pool")
PATHS = (0, bpsw_hip.FASTQ_HOST)


@pytest.fixture(scope="module")
def recorded():
    return fc.load()


def _parse(ctx, path, t1, t2=None, flags=0, **kw):
    return ctx.fastq_parse(t1, t2, flags | path, **kw)


def _assert_same(got, want, what):
    assert got.n_reads == want["n_reads"] and got.consumed == want["consumed"], (what, got.n_reads, got.consumed, want["n_reads"], want["consumed"])
    for k in ARRAYS:
        assert np.array_equal(getattr(got, k), want[k]), (what, k)
    assert got.needed == (want["n_reads"], want["read_pool"].size, want["name_pool"].size), (what, got.needed)


def _check(ctx, t1, t2, flags, what):
    want = fp.parse(t1, t2, flags)
    for path in PATHS:
        _assert_same(_parse(ctx, path, t1, t2, flags), want, (what, path))
    return want


def _refused(ctx, t1, t2, flags, what):
    """both paths refuse with the plain parser's record, text and reason, in the fixed words"""
    with pytest.raises(fp.Refused) as plain:
        fp.parse(t1, t2, flags)
    for path in PATHS:
        with pytest.raises(bpsw_hip.FastqError) as e:
            _parse(ctx, path, t1, t2, flags)
        assert e.value.rc == -1 and str(e.value) == "bpsw_fastq_parse failed (-1): " + plain.value.message("fastq_parse"), (what, path, str(e.value))
    return plain.value


# ---- tile edges, counts, field rules: the shared cases ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.CASES))
def test_case_on_both_paths_against_both_yardsticks(ctx, recorded, name):
    t1, t2, flags = fc.CASES[name]
    want = _check(ctx, t1, t2, flags, name)
    r = recorded[name]
    assert r["text1"] == t1 and r["text2"] == t2
    n = want["n_reads"]
    got = _parse(ctx, 0, t1, t2, flags)
    assert list(got.read_len) == list(r["l_seq"][:n])
    table = np.full(256, 4, np.uint8)
    for k, pair in enumerate(("Aa", "Cc", "Gg", "Tt")):
        table[[ord(c) for c in pair]] = k
    assert bytes(got.read_pool) == bytes(table[np.frombuffer(b"".join(r["seqs"][:n]), np.uint8)]) and bytes(got.qual_pool) == b"".join(r["quals"][:n])
    step = 2 if (t2 is not None or flags & fp.PAIR_NAMES) else 1
    assert bytes(got.name_pool) == b"".join(r["names"][:n:step])
    assert [int(x) for x in np.diff(got.name_off)] == [len(x) for x in r["names"][:n:step]]
    t = bpsw_hip.last_fastq_times()
    assert t[4] > 0 and (n == 0 or min(t[:4]) > 0), t


def test_more_reads_than_one_scan_tile_and_a_second_level(ctx):
    """4 097 records with the scan's tile lowered to 64 items: 65 tiles of reads, so the tile sums themselves take a second step of
    scan_tiles_kernel's loop, and the newline counts of the text's 1 KiB tiles do as well"""
    rng = np.random.default_rng(4097)
    text = fc.records(rng, 4097, 1, 8)
    assert len(text) > 64 * 1024
    lib = bpsw_hip.load_library()
    lib.bpsw_scan_set_tile(64)
    try:
        want = _check(ctx, text, None, fp.FINAL, "4097")
    finally:
        lib.bpsw_scan_set_tile(0)
    assert want["n_reads"] == 4097
    _check(ctx, text, None, fp.FINAL, "4097 at the default tile")


# ---- streaming ----------------------------------------------------------------------------------------------------------------------
def test_a_text_cut_inside_each_line_of_its_last_record(ctx):
    rng = np.random.default_rng(11)
    head = fc.records(rng, 4)
    last = [b"@last one\n", b"ACGTACGTAC\n", b"+last\n", b"IIIIIHHHHH\n"]
    for k in range(4):
        cut = head + b"".join(last[:k]) + last[k][: len(last[k]) // 2]
        want = _check(ctx, cut, None, 0, ("cut", k))
        assert want["n_reads"] == 4 and want["consumed"] == (len(head), 0)
        refusal = _refused(ctx, cut, None, fp.FINAL, ("cut, final", k))
        assert (refusal.record, refusal.key) == (4, "truncated" if k < 3 else "len_diff")
    whole = head + b"".join(last)
    for text, n_open in ((whole, 5), (whole[:-1], 4)):   # a last line without '\n': a line only when the text ends there
        assert _check(ctx, text, None, 0, "open")["n_reads"] == n_open
        assert _check(ctx, text, None, fp.FINAL, "final")["consumed"] == (len(text), 0)


@pytest.mark.parametrize("path", PATHS)
def test_the_remainder_with_the_next_chunk_gives_the_same_records(ctx, path):
    rng = np.random.default_rng(12)
    whole = fc.records(rng, 60, 1, 50)
    want = fp.parse(whole, None, fp.FINAL)
    cuts = [0, 1, 700, 1024, 1025, 2900, len(whole)]
    carry, got = b"", {k: [] for k in ARRAYS if k.endswith("pool") or k == "read_len"}
    for a, b in zip(cuts, cuts[1:]):
        chunk = carry + whole[a:b]
        r = _parse(ctx, path, chunk, None, fp.FINAL if b == len(whole) else 0)
        for k in got:
            got[k].append(getattr(r, k).copy())
        carry = chunk[r.consumed[0]:]
    assert carry == b""
    for k in got:
        assert np.array_equal(np.concatenate(got[k]), want[k]), k


# ---- pairs ---------------------------------------------------------------------------------------------------------------------------
def test_two_texts_of_65_and_70_records(ctx):
    t1, t2, flags = fc.CASES["pairs_65_70"]
    for path in PATHS:
        r = _parse(ctx, path, t1, t2, flags)
        assert r.n_reads == 130 and r.name_off.size == 66
        behind_65 = len(b"\n".join(t2.split(b"\n")[: 4 * 65])) + 1
        assert r.consumed == (len(t1), behind_65) and behind_65 < len(t2)
        assert bytes(r.name_pool[: r.name_off[1]]) == b"pair0"   # "pair0/1" and "pair0/2": one name


def test_a_second_end_with_another_name_is_refused_by_pair(ctx):
    t1, t2, flags = fc.CASES["pairs_plain_names"]
    bad = t2.replace(b"@same3\n", b"@same4\n", 1)
    r = _refused(ctx, t1, bad, flags, "pair name")
    assert (r.read, r.record, r.text, r.key) == (7, 3, 2, "pair_name") and "(pair 3)" in r.message("fastq_parse")
    il = b"".join(fc.rec(n, b"ACGT") for n in (b"a/1", b"a/2", b"b/1", b"c/2"))
    r = _refused(ctx, il, None, fp.FINAL | fp.INTERLEAVED | fp.PAIR_NAMES, "interleaved pair name")
    assert (r.read, r.record, r.text) == (3, 3, 1)
    assert _check(ctx, il, None, fp.FINAL | fp.INTERLEAVED, "interleaved, a name per read")["name_off"].size == 5


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
GOOD = fc.rec(b"g0", b"ACGT") + fc.rec(b"g1", b"TTGACA")
MALFORMED = [   # (what, text, key, record)
    ("missing @", GOOD + b"r2\nACGT\n+\nIIII\n", "no_at", 2),
    ("blank line between records", GOOD + b"\n" + GOOD, "no_at", 2),
    ("missing +", GOOD + b"@r2\nACGT\nx\nIIII\n", "no_plus", 2),
    ("a read on two lines", b"@r0\nACGT\nACGT\n+\nIIIIIIII\n", "no_plus", 0),
    ("lengths differ", GOOD + b"@r2\nACGT\n+\nIII\n", "len_diff", 2),
    ("empty read", GOOD + b"@r2\n\n+\n\n", "empty_read", 2),
    ("empty name", GOOD + b"@\nACGT\n+\nIIII\n", "empty_name", 2),
    ("empty name before a comment", b"@ name\nACGT\n+\nIIII\n", "empty_name", 0),
    ("- in a read", GOOD + b"@r2\nAC-T\n+\nIIII\n", "dash", 2),
    ("a byte below 4 in a read", GOOD + b"@r2\nAC\x03T\n+\nIIII\n", "low_byte", 2),
    ("two bad records: the lower one", GOOD + b"@r2\nA-\n+\nII\n" + GOOD + b"r5\nA\n+\nI\n", "dash", 2),
    ("5 000 bare newlines", b"\n" * 5000, "no_at", 0),
]


@pytest.mark.parametrize("what,text,key,record", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_malformed_records_are_refused_in_fixed_words(ctx, what, text, key, record):
    r = _refused(ctx, text, None, fp.FINAL, what)
    assert (r.key, r.record, r.text) == (key, record, 1)
    if what.startswith("5 000"):   # ... also with room for four reads only: the capacity does not come first, and nothing is stored past a table
        for path in PATHS:
            with pytest.raises(bpsw_hip.FastqError, match="record 0 of text 1: the header line does not begin with '@'"):
                _parse(ctx, path, text, None, fp.FINAL, max_reads=4)


@pytest.mark.parametrize("name", list(fc.CUT_CASES))
def test_where_the_reference_stops_reading(ctx, recorded, name):
    """kseq_read returns -2 at a quality line of another length or a missing one: the reported record is the number bseq_read returned"""
    r = _refused(ctx, fc.CUT_CASES[name], None, fp.FINAL, name)
    assert recorded[name]["text1"] == fc.CUT_CASES[name] and r.record == len(recorded[name]["l_seq"])


def test_arguments_and_capacities(ctx):
    t1, t2, _ = fc.CASES["pairs_plain_names"]
    text = fc.CASES["count_65"][0]
    fit = _parse(ctx, 0, text, None, fp.FINAL)
    n, pool, names = fit.needed
    for path in PATHS:
        for flags, t2_, msg, rc in ((16, None, "unknown flag", -1), (fp.INTERLEAVED, t2, "BPSW_FASTQ_INTERLEAVED with two texts", -1),
                                    (fp.PAIR_NAMES, None, "BPSW_FASTQ_PAIR_NAMES needs two texts or BPSW_FASTQ_INTERLEAVED", -1)):
            with pytest.raises(bpsw_hip.FastqError) as e:
                _parse(ctx, path, t1, t2_, flags)
            assert e.value.rc == rc and str(e.value) == f"bpsw_fastq_parse failed ({rc}): fastq_parse: {msg}"
        for short in ({"max_reads": n - 1}, {"pool_cap": pool - 1}, {"name_cap": names - 1}):
            kw = {"max_reads": n, "pool_cap": pool, "name_cap": names, **short}
            with pytest.raises(bpsw_hip.FastqError) as e:
                _parse(ctx, path, text, None, fp.FINAL, **kw)
            assert e.value.rc == -3 and e.value.needed == fit.needed
            assert str(e.value) == (f"bpsw_fastq_parse failed (-3): fastq_parse: the outputs are too small (needed: {n} reads, {pool} pool bytes, "
                                    f"{names} name bytes)")
        _assert_same(_parse(ctx, path, text, None, fp.FINAL, max_reads=n, pool_cap=pool, name_cap=names), fp.parse(text, None, fp.FINAL), "exact fit")
        # null arguments, and a text of 2^31 bytes (refused before a byte of it is read)
        lib, a = ctx.lib, np.zeros(8, np.int64)
        p = a.ctypes.data_as(C.c_void_p)
        n_reads = C.c_int64(0)
        assert lib.bpsw_fastq_parse(ctx.h, text, len(text), None, 0, fp.FINAL | path, 1, 1, 1, p, p, p, p, p, None, C.byref(n_reads), p, p) == -1
        assert lib.bpsw_last_error() == b"fastq_parse: null argument"
        assert lib.bpsw_fastq_parse(ctx.h, None, 5, None, 0, fp.FINAL | path, 1, 1, 1, p, p, p, p, p, p, C.byref(n_reads), p, p) == -1
        assert lib.bpsw_last_error() == b"fastq_parse: null argument"
        assert lib.bpsw_fastq_parse(ctx.h, text, 2**31, None, 0, fp.FINAL | path, 1, 1, 1, p, p, p, p, p, p, C.byref(n_reads), p, p) == -4
        assert lib.bpsw_last_error() == b"fastq_parse: a text of 2^31 bytes or more"
    assert ctx.lib.bpsw_fastq_parse(None, text, len(text), None, 0, fp.FINAL, 1, 1, 1, p, p, p, p, p, p, C.byref(n_reads), p, p) == -1


# ---- end to end: FASTQ text to SAM text ----------------------------------------------------------------------------------------------
def _fastq_of(reads, quals, names):
    return b"".join(b"@" + n + b"\n" + bytes(b"ACGTN"[c] for c in r) + b"\n+\n" + bytes(q) + b"\n" for r, q, n in zip(reads, quals, names))


def _split(p):
    cut = lambda pool, off, ln: [np.array(pool[int(o): int(o) + int(k)], np.uint8) for o, k in zip(off, ln)]
    return cut(p["read_pool"], p["read_off"], p["read_len"]), cut(p["qual_pool"], p["read_off"], p["read_len"])


def test_fastq_to_sam_single_end(ctx, gold, fixture_reads):
    g, idx, reads, quals, _ = fixture_reads
    opt, so, topt = bpsw_hip.default_opt(), _opt(gold, "c1"), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    _load(ctx, gold["g1_pac"], g.size, _contig_tables(g.size)[1], idx)
    names = [b"frag%d/%d" % (i, i % 3) if i % 2 else b"frag%d" % i for i in range(len(reads))]
    text = _fastq_of(reads, quals, [n + (b" comment" if i % 5 == 0 else b"") for i, n in enumerate(names)])
    p = fp.parse(text, None, fp.FINAL)
    assert p["n_reads"] == len(reads) == 105
    rd, ql = _split(p)
    se = bpsw_hip.SeReadsSoA.from_lists(rd, p["names"], ql, id0=1000, id_step=2)
    for mode in TEXT_MODES:
        want = ctx.align_se_batch(opt, so, topt, se, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=mode)
        for path in PATHS:
            got, consumed = ctx.align_fastq_se(opt, so, topt, text, fp.FINAL | path, id0=1000, id_step=2, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=mode)
            assert got == want and consumed == len(text), (mode, path)
    # a chunk that ends inside a record: the whole records are aligned, the rest is the caller's to carry
    got, consumed = ctx.align_fastq_se(opt, so, topt, text[:-3], 0, id0=1000, id_step=2, zdrop_mode=bpsw_hip.ZDROP_BWA)
    assert got == want[:-1] and text[consumed:].startswith(b"@frag104")
    # the refusals are the stages': a read of 257 bases is the align entry's BPSW_ERR_LIMIT, a malformed record the parse's
    long_text = b"@long\n" + bytes(b"ACGT"[c] for c in g[:257]) + b"\n+\n" + b"F" * 257 + b"\n"
    with pytest.raises(bpsw_hip.FastqError) as e:
        ctx.align_fastq_se(opt, so, topt, long_text)
    assert e.value.rc == -4 and e.value.n_reads == 1
    with pytest.raises(bpsw_hip.FastqError, match=r"align_fastq_se: record 0 of text 1: '-' in the read"):
        ctx.align_fastq_se(opt, so, topt, b"@d\nAC-T\n+\nIIII\n")
    with pytest.raises(bpsw_hip.FastqError) as e:
        ctx.align_fastq_se(opt, so, topt, text, max_reads=104)
    assert e.value.rc == -3 and e.value.n_reads == 105


def test_fastq_to_sam_pairs(ctx, gold, fixture_reads):
    g, idx, reads, quals, _ = fixture_reads
    opt, so, topt = bpsw_hip.default_opt(), _opt(gold, "c1"), bpsw_hip.default_tail_opt(bpsw_hip.TAIL_C)
    table = _contig_tables(g.size)[1]
    _load(ctx, gold["g1_pac"], g.size, table, idx)
    first, second = PAIR_ORDER[0::2], PAIR_ORDER[1::2]
    assert len(first) == 52
    t1 = _fastq_of([reads[i] for i in first], [quals[i] for i in first], [b"pair%d/1" % k for k in range(52)])
    t2 = _fastq_of([reads[i] for i in second], [quals[i] for i in second], [b"pair%d/2" % k for k in range(52)])
    p = fp.parse(t1, t2, fp.FINAL)
    rd, ql = _split(p)
    empty = np.zeros(0, bpsw_hip.ALNREG_DTYPE)
    grp = _group_of(g.size, rd, ql, p["names"], [0] * 104, [empty] * 104, table, NO_PES, id0=500)
    il = b"".join(b"@pair" + a + b"@pair" + b for a, b in zip(t1.split(b"@pair")[1:], t2.split(b"@pair")[1:]))
    for mode in TEXT_MODES:
        want, want_pes = ctx.align_pe_batch(opt, so, topt, grp, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=mode)
        for path in PATHS:
            got, pes, consumed = ctx.align_fastq_pe(opt, so, topt, t1, t2, fp.FINAL | path, id0=500, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=mode)
            assert got == want and pes == want_pes and consumed == (len(t1), len(t2)), (mode, path)
        got, pes, consumed = ctx.align_fastq_pe(opt, so, topt, il, None, fp.FINAL | fp.INTERLEAVED, id0=500, zdrop_mode=bpsw_hip.ZDROP_BWA, flags=mode)
        assert got == want and pes == want_pes and consumed == (len(il), 0), mode
    with pytest.raises(bpsw_hip.FastqError, match=r"align_fastq_pe: record 3 of text 2 \(pair 3\): the name differs from the first end's"):
        ctx.align_fastq_pe(opt, so, topt, t1, t2.replace(b"@pair3/2", b"@pair30/2", 1))
    with pytest.raises(bpsw_hip.FastqError, match="align_fastq_pe: one text without BPSW_FASTQ_INTERLEAVED"):
        ctx.align_fastq_pe(opt, so, topt, t1, None)
