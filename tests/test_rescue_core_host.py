"""csrc/bpsw_rescue_core.h -- the rules of the mate rescue, each stated once for the host layer, the JNI shim and worker2's prepare
step -- on the HOST, against the header alone.

tests/rescue_core_host/rescue_core_host.cpp is a program of its own under -fsanitize=address,undefined (no Python in the sanitized
process) that includes nothing of the library but the header.  It reads every group of tests/rescue_cases.py, in both forms (window
lengths shipped / coordinates only), and prints per flavour what the header decides: the first-round windows of the per-pair plan run
over the pairs with prefix sums of its own, the pairs it touches, the shim's verdict per pair, and the anchors of every end -- the
plan and the verdict once as the library runs them and once with the straight-line fast path compiled out.  Judged here against
rescue_cases.first_round_jobs, the oracle's output, and a statement of the anchors written below: what tests/test_rescue_plan_gpu.py
sees through counters on a device."""
import os
import subprocess

import numpy as np
import pytest

import pyoracle as po
import rescue_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "rescue_core_host", "rescue_core_host.cpp")
CSRC = os.path.join(ROOT, "cloud-scale-bwamem_amd", "csrc")
HDR = os.path.join(CSRC, "bpsw_rescue_core.h")
OUT = os.path.join(HERE, "rescue_core_host", "_build")
MODES = [po.RESCUE_C, po.RESCUE_SCALA]
FORMS = ["bytes", "coords"]


def opt_of(factory, overrides):
    opt = factory()
    for k, v in overrides.items():
        setattr(opt, k, v)
    return opt


def group_text(g, opt, form):
    ints = [0 if form == "bytes" else 1, g.group_size, g.l_pac, opt.flag, opt.max_matesw, opt.pen_unpaired]
    for p in g.pes:
        ints += [int(p[0]), int(p[1]), int(p[2])]
    ints += g.seq_len.tolist() + g.reg_cnt.tolist() + g.ref_cnt.tolist()
    ints.append(len(g.regs))
    for r in g.regs:
        ints += [int(r["rb"]), int(r["score"])]
    ints.append(len(g.ref_rb))
    ints += g.ref_rb.tolist() + g.ref_re.tolist()
    if form == "bytes":
        ints += g.ref_len.tolist()
    return " ".join(str(int(x)) for x in ints)


@pytest.fixture(scope="module")
def decided(orc):
    """{(name, form, mode): {what: [ints], "anchors": [[ints] per end]}} -- one build, one run of the program over all groups"""
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "rescue_core_host_san")
    if not (os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(SRC), os.path.getmtime(HDR))):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        "-o", exe, SRC], check=True)
    keys = [(name, form) for name in rc.CASES for form in FORMS]
    path = os.path.join(OUT, "groups.txt")
    with open(path, "w") as f:
        f.write(f"{len(keys)}\n")
        for name, form in keys:
            g, o, _ = rc.CASES[name]
            f.write(group_text(g, opt_of(orc.default_opt, o), form) + "\n")
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    out, cur = {}, None
    for line in p.stdout.splitlines():
        f = line.split()
        if f[0] == "group":
            name, form = keys[int(f[1])]
            assert FORMS[int(f[2])] == form
            cur = out[name, form, int(f[3])] = {"anchors": []}
            continue
        vals = [int(x) for x in f[2:]]
        assert len(vals) == int(f[1])
        if f[0] == "anchors":
            cur["anchors"].append(vals)
        else:
            cur[f[0]] = vals
    assert len(rc.CASES) == 98 and len(out) == 98 * len(FORMS) * len(MODES)
    return out


@pytest.fixture(scope="module")
def oracle_changed(orc):
    """{(name, mode): pairs whose lists the oracle's sequential walk changed}"""
    out = {}
    for name, (g, o, _) in rc.CASES.items():
        for mode in MODES:
            cnt, regs, _n_sw, _cells = orc.matesw_group(opt_of(orc.default_opt, o), g, mode)
            out[name, mode] = rc.changed_pairs(g, cnt, regs)
    return out


def test_first_round_windows_are_the_documented_lean_plan(orc, decided):
    for (name, form, mode), d in decided.items():
        g, o, _ = rc.CASES[name]
        assert len(d["windows"]) == rc.first_round_jobs(g, opt_of(orc.default_opt, o)), (name, form, mode)
        assert d["windows"] == sorted(set(d["windows"])), (name, form, mode)      # ascending, none twice: the first round is packed unsorted
        assert all(0 <= x < len(g.ref_rb) for x in d["windows"]), (name, form, mode)


def test_shim_verdict_covers_the_plan_and_the_plan_covers_what_the_walk_changed(decided, oracle_changed):
    some_changed = 0
    for (name, form, mode), d in decided.items():
        verdict, touched, changed = set(d["verdict"]), set(d["touched"]), set(oracle_changed[name, mode])
        assert verdict >= touched >= changed, (name, form, mode, sorted(verdict), sorted(touched), sorted(changed))
        some_changed += len(changed)
    assert some_changed > 100


def test_anchors_are_the_first_regions_within_pen_unpaired_of_the_best(orc, decided):
    for (name, form, mode), d in decided.items():
        g, o, _ = rc.CASES[name]
        opt = opt_of(orc.default_opt, o)
        want, at = [], 0
        for e in range(2 * g.group_size):
            score = g.regs["score"][at:at + int(g.reg_cnt[e])]
            passing = [j for j in range(len(score)) if score[j] >= score[0] - opt.pen_unpaired]
            want.append(passing[:max(0, min(opt.max_matesw, int(g.ref_cnt[e])))])
            at += int(g.reg_cnt[e])
        assert d["anchors"] == want, (name, form, mode)


def test_fast_path_decides_as_the_general_walk(orc, decided):
    """every list of every group is the same with the fast path compiled out; and the pairs that meet its precondition (stated here
    once more: one hit per end with a window row and a mate each, max_matesw >= 1, pen_unpaired >= 0) are there in numbers"""
    judged = 0
    for (name, form, mode), d in decided.items():
        assert d["windows"] == d["windows_walk"] and d["touched"] == d["touched_walk"] and d["verdict"] == d["verdict_walk"], (name, form, mode)
        g, o, _ = rc.CASES[name]
        opt = opt_of(orc.default_opt, o)
        if opt.flag & rc.NO_RESCUE or opt.max_matesw < 1 or opt.pen_unpaired < 0:
            continue
        per_pair = np.stack([g.reg_cnt, g.ref_cnt, g.seq_len], 1).reshape(g.group_size, 6)      # (rc, fc, sl) of end 0, of end 1
        fast = (per_pair[:, [0, 3]] == 1).all(1) & (per_pair[:, [1, 2, 4, 5]] >= 1).all(1)
        judged += int(fast.sum())
        if name.startswith("B_") and name.endswith("_fast"):       # the one-hit-per-end pairs are what the fast path is for
            assert fast.tolist() == [True], (name, form, mode)
    assert judged > 200
