"""The job tables of tests/sw_cases.py through the oracle alone (no GPU): every table still does what its name says, so that a later
edit there cannot quietly turn the kernel-versus-oracle tests of tests/test_swalign_forms_gpu.py into restatements of the easy case."""
import time

import numpy as np
import pytest

import sw_cases as sc

SCORE, TE, QE, SCORE2, TE2, TB, QB = range(7)


@pytest.fixture(scope="module")
def results(orc):
    t0 = time.perf_counter()
    res = [(b, sc.want(orc, b)) for b in sc.all_batches()]
    return res, time.perf_counter() - t0


def _by_tag(results, name, kind):
    out = {}
    for b, w in results[0]:
        if b.name == name:
            for tag, row in zip(b.tags, w):
                if tag[0] == kind:
                    out[tag[1:]] = row
    assert out, (name, kind)
    return out


def test_the_whole_table_costs_seconds(results):
    assert results[1] < 10.0, f"{results[1]:.1f} s of oracle time"


def test_batches_select_the_form_they_are_named_for():
    """by geometry alone (kernel_for restates launch_sw_kernel): every instantiation has a batch of its own at the matching switches"""
    base = {"BPSW_RING": "0"}
    assert [sc.kernel_for(b, base, False) for b in sc.length_cases("packed")] == [f"swp_kernel<{c},lds>" for c in range(1, 6)]
    assert [sc.kernel_for(b, dict(base, BPSW_SW_KEYS_LDS="0"), False) for b in sc.length_cases("packed")] == [f"swp_kernel<{c},hbm>" for c in range(1, 6)]
    off = {"BPSW_SW_PACK": "0", "BPSW_SW_QUAD": "0"}
    assert [sc.kernel_for(b, off, False) for b in sc.length_cases("sw32")] == [f"sw_kernel<{c}>" for c in (1, 2, 3, 4, 6, 8, 3)]
    assert {sc.kernel_for(b, {"BPSW_SW_PACK": "0", "BPSW_SW_QUAD": "1"}, False) for b in sc.length_cases("quad")} == {"sw4_kernel"}
    assert [len(b.pairs) % 4 for b in sc.length_cases("quad")] == [1, 2, 3]
    # at the defaults the refusing scoring sends every 32-bit batch to its sw_kernel<C>, the packable one only the mates above 256
    assert [sc.kernel_for(sc.with_scoring(b, sc.M5X3), {}, False) for b in sc.length_cases("sw32")[:6]] == [f"sw_kernel<{c}>" for c in (1, 2, 3, 4, 6, 8)]
    assert [sc.kernel_for(b, {}, False) for b in sc.length_cases("sw32")[:6]] == [f"swp_kernel<{c},hbm>" for c in (2, 3, 4, 5)] + ["sw_kernel<6>", "sw_kernel<8>"]
    assert all(sc.pack_bias(s) >= 0 for s in sc.PACKABLE) and all(sc.pack_bias(s) < 0 for s in sc.REFUSING)
    assert sc.pack_bias(sc.HI254) + int(sc.HI254.mat.max()) == 254 and int(sc.M5X4.mat.max()) == sc.M5X4.b + 1
    # the key-placement edges: ring below the resident kernel's rows and sixteen jobs, LDS keys up to 1536 rows
    want = {"keys_c5_rows1536_n9": "swp_resident_kernel<5>", "keys_c5_rows1536_n17": "swp_kernel<5,lds>",
            "keys_c5_rows1537_n9": "swp_kernel<5,hbm>", "keys_c5_rows1537_n17": "swp_kernel<5,hbm>",
            "keys_c3_rows1024_n9": "swp_resident_kernel<3>", "keys_c3_rows1024_n17": "swp_kernel<3,lds>",
            "keys_c3_rows1025_n9": "swp_kernel<3,lds>", "keys_c3_rows1025_n17": "swp_kernel<3,lds>",
            "keys_c3_rows1536_n9": "swp_kernel<3,lds>", "keys_c3_rows1537_n9": "swp_kernel<3,hbm>",
            "keys_c3_rows1536_n17": "swp_kernel<3,lds>", "keys_c3_rows1537_n17": "swp_kernel<3,hbm>"}
    assert {b.name: sc.kernel_for(b, {}, sc.takes_ring(b, {})) for b in sc.key_edge_cases()} == want
    assert sc.kernel_for(sc.longest_window(240), {}, False) == "swp_kernel<5,hbm>" and sc.kernel_for(sc.longest_window(300), {}, False) == "sw_kernel<6>"
    assert all(len(b.pairs) < 96 * 64 for b in sc.all_batches())       # no batch is large enough for the quad form by itself


def test_duos_hold_a_short_job_next_to_a_long_one():
    for form in ("packed", "sw32", "quad"):
        for b in sc.length_cases(form):
            tl = [len(t) for _, t, _ in b.pairs]
            if len(tl) > 8:
                assert tl[0] >= 500 and tl[1] == 0 and min(tl[:8:2]) > 30 * max(tl[1:8:2])
                assert sum(r for _, _, r in b.pairs) >= len(tl) // 6


def test_plateaus(results):
    rows = _by_tag(results, "sb_plateau", "plateau")
    for k in sc.PLATEAU_K:
        for p in sc.PLATEAU_P:
            r = rows[(k, p)]
            assert r[SCORE] == k and r[TE] == sc.plateau_start(p) + k - 1
            if p >= 63:
                assert r[SCORE2] == r[SCORE]
                assert r[TE2] == sc.plateau_start(p) + 2 * k + 1        # the first entry of the parity chain beyond te + tmp
                if p > 63:
                    assert (r[TE2] - rows[(k, p - 1)][TE2]) % 2 == 1    # ... which alternates with the parity of p
            if p <= 8:
                assert r[SCORE2] == -1
    assert tuple(rows[(40, 63)][[SCORE2, TE2]]) == (40, 151)
    # with every row hot (threshold 0, 1) the list is at its longest; above every score there is none
    for b, w in results[0]:
        if b.name in ("sb_plateau_thr256", "sb_plateau_thr65535"):
            assert (w[:, SCORE2] == -1).all() and (w[:, TB] == -1).all()
        if b.name == "sb_plateau_thr0":
            assert (w[:, SCORE2] >= 0).all()


def test_second_copy_around_the_exclusion_window(results):
    rows = _by_tag(results, "sb_copy2", "copy2")
    for length in sc.COPY2_MATES:
        for side in (1, -1):
            assert all(rows[(length, side, g)][SCORE] == 2 * length for g in sc.COPY2_G)        # tmp == length != score
            assert rows[(length, side, side)][SCORE2] == 2 * sc.COPY2_PART                      # one row outside: the whole partial copy
            assert rows[(length, side, side)][SCORE2] > rows[(length, side, 0)][SCORE2]         # on the edge row: excluded
            assert rows[(length, side, side)][TE2] == rows[(length, side, 0)][TE] + side * (length + 1)


def test_thresholds(results):
    for s in sc.THRESHOLDS:
        rows = _by_tag(results, f"sb_threshold{s}", "threshold")
        assert [int(rows[(s, d)][SCORE2]) for d in (-1, 0, 1)] == [-1, s, s + 1]


def test_stop_cases_report_the_earliest_row(results):
    seen = set()
    for b, w in results[0]:
        if b.name.startswith("stop") and b.name != "stop_duo_cap":
            for (_, s, r), row in zip(b.tags, w):
                assert row[TE] == r, (b.name, s, r, row)
                assert row[SCORE] == (255 if s == 254 else s)
                seen.add((s, r % sc.PK_G))
    assert seen >= {(s, x) for s in (1, 30, 254) for x in range(sc.PK_G)}
    duo = [w for b, w in results[0] if b.name == "stop_duo_cap"][0]
    caps = (duo[:, SCORE] == 255)
    assert caps.sum() == 6 and (caps[0::2] != caps[1::2]).all() and caps[0] and not caps[2]      # both orders
    assert (duo[caps, TE] < 260).all() and (duo[~caps, TE] > 600).all()


def test_m5x4_exact_copies(results):
    w = [w for b, w in results[0] if b.name == "scoring" and b.scoring is sc.M5X4][0]
    assert w[:4, SCORE].tolist() == [245, 250, 255, 255]


def test_n_tables_hold_what_their_tags_say():
    b = sc.n_cases()[0]
    assert {s.scoring.name for s in sc.n_cases()} >= {"default", "default_g5241"}
    assert sc.DEFAULT_G5241.o_del + sc.DEFAULT_G5241.e_del != sc.DEFAULT_G5241.o_ins + sc.DEFAULT_G5241.e_ins
    where = {}
    for k, ((q, t, _), tag) in enumerate(zip(b.pairs, b.tags)):
        ns = [i for i, x in enumerate(t) if x == 4]
        assert len(t) == sc.N_WINDOW
        if tag[0] == "n":
            assert ns == ([tag[1]] if tag[2] else [])
            where.setdefault(tag[1], set()).add((k % 2, tag[2]))
        elif tag[0] == "n2":
            assert ns == [tag[1], tag[1] + tag[2]]
        else:
            assert list(q).count(4) == 1
    # the N of every row in job A only, in job B only, and in both
    assert set(where) == set(sc.N_ROWS) and all(v == {(0, 1), (0, 0), (1, 0), (1, 1)} for v in where.values())


def test_ends_in_first_columns(results):
    for c, b in enumerate(sc.ends_in_first_columns(), 1):
        w = sc._WANT[(b.name, b.scoring.name, b.xtra)]
        got = set()
        for tag, row in zip(b.tags, w):
            if tag[0] == "ends":
                assert row[QE] == tag[1] and row[SCORE] == tag[1] + 1 and row[TB] >= 0 and row[QB] == 0
                got.add(tag[1])
        assert got == set(range(c + 1)) and sc.packed_class(sc.geometry(b)[1]) == c


def test_longest_windows_use_both_ends_of_the_row_fields(results):
    for b, w in results[0]:
        if b.name.startswith("longest"):
            assert all(len(t) == sc.MAX_TLEN for _, t, _ in b.pairs)
            assert w[0, TE] == sc.MAX_TLEN - 1 and 250 < w[0, TE2] < 300 and w[0, SCORE2] > 50
            assert w[1, TE] < 330 and w[1, TE2] == sc.MAX_TLEN - 1
            assert w[0, SCORE] < 251 and w[0, TB] > 65000
        if b.name.startswith("keys_"):
            assert w[1, TE] == sc.geometry(b)[2] - 1 and w[1, SCORE2] >= 19      # the copy in the last rows of the longest window


def test_coverage_counts(results):
    w = np.concatenate([w for _, w in results[0]])
    start = np.concatenate([np.full(len(w), bool(b.xtra & sc.KSW_XSTART)) for b, w in results[0]])
    n = len(w)
    assert (w[:, SCORE2] >= 0).sum() * 4 >= n, ((w[:, SCORE2] >= 0).sum(), n)
    assert (w[:, TB] >= 0).sum() * 4 >= n, ((w[:, TB] >= 0).sum(), n)
    assert (w[:, SCORE] == 255).sum() * 4 >= n, ((w[:, SCORE] == 255).sum(), n)
    assert ((w[:, TB] == -1) & start).sum() >= 10
    assert ((w[:, QE] >= 0) & (w[:, QE] <= 4)).sum() >= 10
