"""tests/rescue_cases.py on the CPU: every case is what it claims (by the oracle alone), the table meets its floors, and the oracle's
C flavour equals the reference's own C on every case.

The Scala flavour has no second yardstick: no JVM exists here, so nothing runs MemSamPe.scala itself.  What holds it is the text
(tests/scala_text.py pins the cited lines) and, for the one place where the two flavours build a different region, literals derived by
hand from MemSamPe.scala:1192-1212 (rescue_cases.D_SCALA, test_scala_regions_of_each_orientation_are_the_hand_derived_ones)."""
import dataclasses

import numpy as np
import pytest

import pyoracle as po
import rescue_cases as rc
from conftest import region_fields_equal

MODES = [po.RESCUE_C, po.RESCUE_SCALA]


def opt_of(factory, overrides):
    opt = factory()
    for k, v in overrides.items():
        setattr(opt, k, v)
    return opt


@pytest.fixture(scope="module")
def walked(orc):
    """the oracle's answer for every case in both flavours, computed once: {(name, mode): (cnt, regs, n_sw)}"""
    out = {}
    for name, (g, o, _) in rc.CASES.items():
        for mode in MODES:
            cnt, regs, n_sw, _cells = orc.matesw_group(opt_of(orc.default_opt, o), g, mode)
            out[name, mode] = (cnt, regs, n_sw)
    return out


@pytest.mark.parametrize("mode", MODES, ids=["c", "scala"])
@pytest.mark.parametrize("name", list(rc.CASES))
def test_case_is_what_it_claims(orc, walked, name, mode):
    g, o, claims = rc.CASES[name]
    cnt, regs, n_sw = walked[name, mode]
    changed = rc.changed_pairs(g, cnt, regs)
    out_hashes = set(regs["hash"].tolist())
    if "touched" in claims:                       # B: one pair
        assert (n_sw > 0) == claims["touched"]
        if not claims["touched"]:
            assert changed == []
    if "changed" in claims:
        assert changed == claims["changed"]
    if claims.get("count_unchanged"):
        assert np.array_equal(cnt, g.reg_cnt)
    if "n_sw" in claims:
        assert n_sw == claims["n_sw"]
    for h in claims.get("killed", ()):
        assert h in set(g.regs["hash"].tolist()) and h not in out_hashes
    for h in claims.get("kept", ()):
        assert h in out_hashes
    if "rb_eq_re" in claims:
        assert int((regs["rb"] == regs["re"]).sum()) == (claims["rb_eq_re"] if mode == po.RESCUE_SCALA else 0)
    census = rc.window_census(g)
    for what, at_least in claims.get("windows", {}).items():
        assert census[what] >= at_least, (what, census)
    if claims.get("zero_len"):
        assert int(g.seq_len.min()) == 0
    else:
        assert int(g.seq_len.min()) > 0
        first = rc.first_round_jobs(g, opt_of(orc.default_opt, o))
        assert first <= n_sw
        assert (n_sw > first) == claims["second_round"]


def test_fast_and_walk_twins_are_touched_alike(walked):
    """B: a hit far below the threshold and nowhere near a proper distance changes neither the verdict nor the jobs"""
    for fast, walk, _pes, _r, _label, touched in rc.B_TABLE:
        for mode in MODES:
            assert walked[fast, mode][2] == walked[walk, mode][2]
            assert (walked[fast, mode][2] > 0) == touched
        g = rc.CASES[fast][0]
        assert g.reg_cnt.tolist() == [1, 1] and sorted(rc.CASES[walk][0].reg_cnt.tolist()) == [1, 2]


def test_floors_of_the_table(walked):
    # a successful rescue in every orientation in both flavours: the D pairs, whose rescued end starts empty
    g = rc.CASES["D_each_orientation"][0]
    for mode in MODES:
        cnt = walked["D_each_orientation", mode][0]
        seen = {r for k, (r, _rev, e) in enumerate(rc.D_ORDER) if g.reg_cnt[2 * k + e] == 0 and cnt[2 * k + e] == 1}
        assert seen == {0, 1, 2, 3}
    # pairs whose input region was killed
    killed_pairs = 0
    for name, (g, _o, _c) in rc.CASES.items():
        regs = walked[name, po.RESCUE_C][1]
        gone = set(g.regs["hash"].tolist()) - set(regs["hash"].tolist())
        killed_pairs += len({(h >> 8) & 0xFFFFFFFF for h in gone})
    assert killed_pairs >= 4
    # second rounds by a decoy or by the removed justifier
    assert sum(1 for n in ("E_decoy_first", "E_justifier_removed", "A_max_matesw_2", "A_pen_unpaired_0") if rc.CASES[n][2]["second_round"]) >= 2
    # one-hit-per-end pairs on each side of each limit
    for label in ("low-1", "low", "high", "high+1"):
        assert sum(1 for row in rc.B_TABLE if row[4] == label) >= 8
    inside = [rc.CASES[row[0]][2]["inside"] for row in rc.B_TABLE]
    assert inside.count(True) >= 8 and inside.count(False) >= 8


def test_the_justifier_case_is_one(orc):
    """E_justifier_removed: orientation r of anchor 1 is skipped against the INITIAL mate list, yet the sequential walk runs it -- the
    walk's result differs from a walk in which that window is unusable"""
    g, o, _ = rc.CASES["E_justifier_removed"]
    j = rc.JUSTIFIER
    end, anchor, r = j["end"], j["anchor"], j["r"]
    mine = g.regs[g.reg_cnt[0]:] if end else g.regs[:g.reg_cnt[0]]
    mates = g.regs[:g.reg_cnt[0]] if end else g.regs[g.reg_cnt[0]:]
    assert mine["score"][anchor] >= mine["score"][0] - o["pen_unpaired"]
    hit = [rc.infer_dir(int(mine["rb"][anchor]), int(m["rb"]), g.l_pac) for m in mates]
    assert any(d == r and g.pes[r][0] <= dist <= g.pes[r][1] for d, dist in hit)          # skipped initially
    assert not any(g.pes[d][0] <= dist <= g.pes[d][1] for d, dist in (rc.infer_dir(int(mine["rb"][0]), int(m["rb"]), g.l_pac) for m in mates))
    x = 4 * ((int(g.ref_cnt[0]) if end else 0) + anchor) + r
    g2 = dataclasses.replace(g, ref_len=g.ref_len.copy())
    g2.ref_len[x] += 1                                                                     # "funny things happening": never aligned
    for mode in MODES:
        opt = opt_of(orc.default_opt, o)
        a, b = orc.matesw_group(opt, g, mode), orc.matesw_group(opt, g2, mode)
        assert a[2] == b[2] + 1 and a[1].tobytes() != b[1].tobytes()


def test_scala_regions_of_each_orientation_are_the_hand_derived_ones(walked):
    g = rc.CASES["D_each_orientation"][0]
    for mode, table in ((po.RESCUE_SCALA, rc.D_SCALA), (po.RESCUE_C, rc.D_C)):
        cnt, regs, _ = walked["D_each_orientation", mode]
        sl = rc.pair_slices(cnt)
        for k, (r, rev, e) in enumerate(rc.D_ORDER):
            pr = regs[sl[k]]
            got = pr[0] if e == 0 else pr[cnt[2 * k]]
            assert cnt[2 * k + e] == 1 and got["hash"] == 0
            assert tuple(int(got[f]) for f in ("rb", "re", "qb", "qe", "score", "seedcov")) == table[r, rev], (mode, r, rev, e)


def _against_reference(letter):
    def test(orc, ref):
        for name, (g, o, claims) in rc.CASES.items():
            if not name.startswith(letter + "_") or claims.get("zero_len"):
                continue                                   # (what ksw_align2 does with an empty query profile is not relied on)
            opt = opt_of(orc.default_opt, o)
            cnt, regs, _n_sw, _ = orc.matesw_group(opt, g, po.RESCUE_C)
            rcnt, rregs = ref.matesw_group(opt, g)
            assert np.array_equal(cnt, rcnt), name
            region_fields_equal(regs, rregs, skip=("csub",))
    test.__name__ = f"test_oracle_equals_the_reference_c_on_{letter}"
    test.__doc__ = f"the oracle's C flavour against the reference's mem_group_matesw on the {letter} cases (csub aside, as in test_oracle_vs_ref.py)"
    return test


for _letter in "ABCDEFGI":
    globals()[f"test_oracle_equals_the_reference_c_on_{_letter}"] = _against_reference(_letter)
