"""The case table of tests/ext_cases.py through the row model and the oracle alone (no GPU): every case still is what its name says, so
that a later edit there -- or a changed ROWS_NARROW / ROWS4_NARROW in csrc/bpsw_extend_rows.h, which the tables are built from -- cannot
quietly turn the kernel-versus-oracle runs of tests/test_ext_forms_gpu.py into restatements of the easy case.  No case is skipped."""
import numpy as np
import pytest

import bpsw_hip
import ext_cases as ec
import ext_rows_model as erm


@pytest.fixture(scope="module")
def table(orc):
    """per case: the model's ten words and sides with the tail-row bound on and off, the oracle's ten words, the packed batch"""
    out = []
    for c in ec.cases():
        wire = bpsw_hip.wire_pack(ec.soa_of([c], c.sc))
        want, _ = orc.wire_extend(wire, np.array(c.sc.mat, np.int8), c.sc.zdrop, c.sc.zmode)
        out.append((c, wire, want, {b: erm.extension(wire, 0, c.sc, b) for b in (True, False)}))
    return out


def test_the_header_constants_are_read_from_its_text():
    c = erm.header_constants()
    assert 1 <= c["ROWS_NARROW"] <= 63 and c["ROWS_NARROW"] < c["ROWS4_NARROW"] <= 127      # (a layout must hold what it is handed)
    assert (ec.RN, ec.R4N) == (c["ROWS_NARROW"], c["ROWS4_NARROW"])
    assert (c["MAX_QLEN"], c["MAX_RLEN"]) == (1023, 4095)                                  # include/bpsw.h, and the issue's limits


def test_names_are_unique_and_scores_stay_within_int16():
    cs = ec.cases()
    assert len({c.name for c in cs}) == len(cs)
    for c in cs + ec.past_the_limits():
        for side in (c.left, c.right):
            if side is not None:
                assert 0 <= c.h0 and c.h0 + len(side[0]) * c.sc.amax <= 32767, c.name
        assert (c.left is None) != (c.right is None) or c.left is not None, c.name
        assert c.mat_max == c.sc.amax, c.name                                              # the packer's gap bounds use the matrix's maximum


def test_the_model_agrees_with_the_oracle_on_every_case(table, orc):
    """the ten words with the tail-row bound on and off (the bound must not change a result), and each side's six SWExtend fields of
    the first band against orc.sw_extend"""
    for c, wire, want, model in table:
        for bound in (True, False):
            got, sides = model[bound]
            assert np.array_equal(got, want), (c.name, bound, got, want)
        for qt, s, clip in zip((c.left, c.right), model[True][1], (c.sc.pen_clip5, c.sc.pen_clip3)):
            if s is None:
                continue
            q, t = qt
            six, _ = orc.sw_extend(np.array(q, np.uint8), np.array(t, np.uint8), np.array(c.sc.mat, np.int8), c.sc.o_del, c.sc.e_del, c.sc.o_ins,
                                   c.sc.e_ins, c.sc.w, clip, c.sc.zdrop, s.hinit, c.sc.zmode)
            assert np.array_equal(s.tries[0].res, six), (c.name, s.tries[0].res, six)


def test_every_case_reports_the_facts_it_is_named_for(table):
    for c, wire, want, model in table:
        F = ec.facts_of(c, model[c.bound][1])
        missing = [f for f in c.facts if f not in F] + [f for f in c.full if "full:" + f not in F]
        assert not missing, (c.name, missing)
        assert c.facts or c.full, c.name                                                   # no case without a reason


def test_the_table_reaches_every_fact_layout_transition_selector_and_full_form(table):
    seen = set()
    for c, wire, want, model in table:
        seen |= ec.facts_of(c, model[c.bound][1])
    assert not [f for f in ec.REQUIRED if f not in seen]
    assert len(set(ec.REQUIRED)) == len(ec.REQUIRED)


def test_the_models_phase_row_is_the_kernels_formula(table):
    """i_h1z = ceil((h0 - oDel) / eDel) - 1 is the first row with h1 == 0, for every case's gap costs and start score; u0 and qa are the
    tail rows' bound in the assembly loops' form: tail_row_bound(i) == max(u0 - i eDel, qa)"""
    for c, wire, want, model in table:
        for s, qt in zip(model[True][1], (c.left, c.right)):
            if s is None:
                continue
            for call in s.tries:
                assert all((r.h1 > 0) == (r.i < call.i_h1z) for r in call.rows), c.name
                for i in (len(qt[0]), len(qt[0]) + 7):
                    assert erm.tail_row_bound(len(qt[0]), i, s.hinit, c.sc.amax, c.sc.o_del, c.sc.e_del) == max(call.u0 - i * c.sc.e_del, call.qa), c.name


def test_the_batches_of_the_gpu_test(table):
    """what tests/test_ext_forms_gpu.py relies on: the short table has no flank above 255 bases (the resident kernel and the launched
    short kernel take all of it), every full-only case has one, and one past each limit is really past it"""
    for c, *_ in table:
        longest = max(len(s[0]) for s in (c.left, c.right) if s is not None)
        assert (longest > 255) == c.full_only, c.name
    q, r = ec.past_the_limits()
    assert len(q.right[0]) == erm.header_constants()["MAX_QLEN"] + 1 and len(r.right[1]) == erm.header_constants()["MAX_RLEN"] + 1
