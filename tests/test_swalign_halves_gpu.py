"""The half-wave packed form of the mate-rescue SW (csrc/bpsw_swalign.hip: swh_pass / swh_do_quartet -- four jobs per wavefront, a packed
pair in each 32-lane half, 30 lanes x 5 columns, mates of up to 150 bases) against the oracle, on tables built for what is new in it:
the half boundary, the per-half geometry (L0, D, stop, tLen), the keys stored every step and folded every eight, the quartet's tail
(a missing position, a single pair, one unit of two obtained), and the worker of the submission ring that takes two units with one ticket.

Every table runs three ways.  In this process: as one lone batch of at least sixteen jobs (a launch: swh_kernel, or swp_kernel<3> where
a mate has more than 150 bases) and in chunks of three to fifteen jobs (the ring: from SW_RING_PAIR_MIN_UNITS = 8 units on the host sends a batch to the half-wave
ring class, whose workers take two units per ticket, so the chunks of fifteen jobs run as quartets and the smaller ones pair by pair in
class 3); the ring's `submitted` counter says which way a batch went.  And once more in a child process started with BPSW_SW_HALVES=0, where
every batch takes the pair-per-wave form as before: the child compares against THE ARRAYS THIS PROCESS GOT, not against the oracle
again, so a divergence between the two forms is reported as one.  Two more children: BPSW_RING_LONE_LAUNCH=0 sends the lone batches
through the ring as well (17 to 58 jobs: quartets from odd and even unit counts), and BPSW_SW_KEYS_LDS=0 with BPSW_RING=0 runs every
batch, the chunks included, as a launch with the keys in HBM scratch (n = 1..15: trailing pairs, a missing position)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":      # the child: no conftest has set the paths
    sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "cloud-scale-bwamem_amd"), os.path.join(os.path.dirname(HERE), "oracle")]

import bpsw_hip  # noqa: E402
import sw_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

HW_QMAX = 150            # the longest mate the half-wave form takes: 30 lanes x 5 columns
PAIR_MIN_UNITS = 8       # SW_RING_PAIR_MIN_UNITS (csrc/bpsw_ring.h): a batch of this many units goes to the half-wave ring class
MATES = (1, 4, 5, 6, 145, 146, 147, 148, 149, 150)      # the first lane with a column at both ends of a half; a pad of <= C columns
# booking-group rounding (PK_G = 8) and the selector staging (PK_TBUF = 256 words per half)
WINDOWS = (0, 1, 7, 8, 9, 15, 16, 17, 255, 256, 257, 511, 512, 513)


# ---- the tables ------------------------------------------------------------------------------------------------------------------
def _lengths():
    """58 jobs = 14 quartets and a single pair.  Quartet q: its lower half's windows have WINDOWS[q] rows, its upper half's
    WINDOWS[q + 7] -- every length in either half, the halves always different (one stops hundreds of steps before the other);
    the mates cycle through MATES, so a quartet holds four different lengths; every length comes with both q_rev."""
    rng = np.random.default_rng(150)
    cases = []
    for k in range(58):
        q, half = k // 4, (k % 4) // 2
        ql = MATES[k % len(MATES)]
        rev = (k // len(MATES)) % 2
        tlen = WINDOWS[(q + 7 * half) % len(WINDOWS)]
        mate = sc._r(rng, ql)
        w = sc._embed(rng, mate, tlen, second=k % 3 == 0)
        cases.append(((sc._rc(mate) if rev else mate, w, rev), ("len", ql, tlen, rev)))
    seen = {(t[1], t[3]) for _, t in cases}
    assert all((ql, rev) in seen for ql in MATES for rev in (0, 1))
    return cases


def _long_windows(rows, n):
    """n jobs, the second with a window of `rows` rows and its copy in the last rows (the last key row is read); its partner in the other
    half of the quartet has a short window, in both orders"""
    rng = np.random.default_rng(rows)
    cases = []
    for k in range(n):
        mate = sc._r(rng, HW_QMAX - (k % 3))
        if k in (1, 6):
            body = mate[-50:] + sc._r(rng, 10) + mate
            w = sc._r(rng, rows - len(body)) + body
        else:
            w = sc._embed(rng, mate, int(rng.integers(1, 400)), second=k % 2 == 0)
        cases.append(((mate, w, 0), ("long", rows, k)))
    return cases


ISOLATION_SCORING = sc.M2X1       # a = 2: an exact copy of 126 bases scores 252, two below the cap -- H at the last column as large as it gets
STRONG = 126


def _isolation():
    """Quartet p = 0..3: position p holds an exact copy that ENDS IN THE WINDOW'S LAST ROW (its H / E / F and its key at the half's last
    column are at their largest while the neighbouring half's first lane reads what lanes 30 / 31 hand on); the other half holds two mates
    unrelated to their windows (one window longer than the strong job's: it runs on alone).  Quartets 4..7: the same with the unrelated
    half's windows shorter.  Whatever leaks over the boundary shows in the weak half's scores."""
    rng = np.random.default_rng(126)
    cases = []
    for p in range(8):
        strong = sc._r(rng, STRONG, (0, 1, 2))
        quartet = [None] * 4
        pos = p % 4
        quartet[pos] = ((strong, [3] * (600 - STRONG) + strong, 0), ("strong", p))
        partner = sc._r(rng, 140)
        quartet[pos ^ 1] = ((partner, sc._embed(rng, partner, 500, second=False), 0), ("partner", p))
        for g in range(2):
            other = 2 * (1 - pos // 2) + g
            rows = (600, 720)[g] if p < 4 else (590, 480)[g]
            quartet[other] = ((sc._r(rng, HW_QMAX - g), sc._r(rng, rows), g), ("weak", p, g))
        cases += quartet
    return cases


def _pass2():
    """default scoring, XSUBO | XSTART | 19: the second pass is wanted by the jobs that score 19 or more.  Quartets in which 0, 1, 3 and 4
    of the four want it, the odd one in every position."""
    rng = np.random.default_rng(19)

    def job(strong):
        mate = sc._r(rng, int(rng.integers(100, HW_QMAX + 1)))
        if strong:
            return (mate, sc._embed(rng, mate, int(rng.integers(300, 700)), second=True), 0), ("above",)
        w = sc._r(rng, int(rng.integers(300, 700)), (3,))                 # T rows: only the planted ten bases score
        mate = [b % 3 for b in mate]
        w[100:110] = mate[20:30]
        return (mate, w, 0), ("below",)

    cases = []
    for strong in ([0, 0, 0, 0], [1, 1, 1, 1]):
        cases += [job(s) for s in strong]
    for odd in range(4):
        cases += [job(int(k == odd)) for k in range(4)]          # wanted by one
        cases += [job(int(k != odd)) for k in range(4)]          # wanted by three
    return cases


def _cap():
    """M5X4 (maxScore = 251): an exact copy of 51 bases reaches the cap in pass 1 (score 255, no second pass) in one position of the quartet,
    longer mates run on beside it"""
    rng = np.random.default_rng(51)
    cases = []
    for p in range(4):
        quartet = []
        for k in range(4):
            if k == p:
                mate = sc._r(rng, 51, (0, 1, 2))
                quartet.append(((mate, [3] * 33 + mate + [3] * 47, 0), ("cap", p)))
            else:
                mate = sc._r(rng, (150, 100, 120, 57)[k], (0, 1, 2))       # thirty-five of its bases in a window of T: 175, below the cap
                w = [3] * (300 + 50 * k)
                w[200:235] = mate[10:45]
                quartet.append(((mate, w, 0), ("beside", p)))
        cases += quartet
    cases += cases[:2]        # (n = 18: and a trailing pair)
    return cases


def _stops():
    """XSTOP | 30: the row on which a pass stops on each of sixteen consecutive rows (every booking lane of a group of eight, both group
    phases), the stopping job in position k % 4 of quartet k (either slot of either half, four times each), beside three jobs that never reach 30 and run to the end of 400 rows"""
    rng = np.random.default_rng(30)
    cases = []
    for k, off in enumerate(sc.STOP_OFFSETS):
        quartet = [((sc._r(rng, 150, (0, 1)), sc._r(rng, 400, (2, 3)), 0), ("runs_on",)) for _ in range(4)]
        quartet[k % 4] = sc._stop(30, off, HW_QMAX - (k % 3))       # position k % 4: either slot of either half, four times each
        cases += quartet
    return cases


def _n_rows():
    """an N in the window of ONE half only, on rows 255 / 256 / 257 (the edge of the selector staging: with a 150-base mate a row is its own
    word): the patched step runs for both halves while one has no N.  Then N in the mate."""
    rng = np.random.default_rng(4)
    cases = []
    for x in (255, 256, 257):
        for half in (0, 1):
            for k in range(4):
                mate = sc._r(rng, HW_QMAX)
                cases.append(((mate, sc._n_window(rng, mate, (x,) if k // 2 == half else ()), 0), ("n", x, half)))
    for k in range(8):
        mate = sc._r(rng, HW_QMAX - k)
        clean = list(mate)
        mate[(17 * k) % len(mate)] = 4
        cases.append(((sc._rc(mate) if k % 2 else mate, sc._n_window(rng, clean, ()), k % 2), ("n_mate", k)))
    return cases


def _with_151():
    """the first twenty jobs of the length table and one mate of 151 bases: the batch that holds it takes the pair-per-wave form"""
    rng = np.random.default_rng(151)
    mate = sc._r(rng, HW_QMAX + 1)
    return _lengths()[:20] + [((mate, sc._embed(rng, mate, 400, second=True), 0), ("q151",))]


def _tables():
    out = {}

    def add(name, scoring, xtra, cases, sizes):
        out[name] = (sc._batch("halves_" + name, scoring, xtra, cases), sizes)

    lengths = _lengths()
    add("lengths", sc.DEFAULT, sc.XTRA, lengths, (4, 8, 12))
    add("lengths_odd_chunks", sc.DEFAULT, sc.XTRA, lengths[2:], (3, 5, 7, 9, 11, 13, 15))
    for s in (sc.M2X3, sc.DEFAULT_G5241, sc.GENERAL, sc.HI254, sc.B254):          # SAME_OE false; the bias and cap at their ends
        add("lengths_" + s.name, s, sc.XTRA, lengths, (8, 12, 15))
    add("rows1024", sc.DEFAULT, sc.XTRA, _long_windows(1024, 18), (8, 10))          # the resident kernel's last window
    add("rows1025", sc.DEFAULT, sc.XTRA, _long_windows(1025, 17), (8, 9))           # ... and the first that is a launch at any size
    add("rows1536", sc.DEFAULT, sc.XTRA, _long_windows(1536, 17), (8, 9))           # the last window whose keys stay in LDS: 52 KB + 11 KB static
    add("rows1537", sc.DEFAULT, sc.XTRA, _long_windows(1537, 17), (8, 9))           # the keys in HBM scratch
    add("isolation", ISOLATION_SCORING, sc.XTRA, _isolation(), (4, 8, 12))
    add("pass2", sc.DEFAULT, sc.XTRA, _pass2(), (4, 8, 12))
    add("cap", sc.M5X4, sc.XTRA, _cap(), (4, 8, 6))
    add("stops", sc.DEFAULT, sc.KSW_XSTART | sc.KSW_XSTOP | 30, _stops(), (4, 8, 12))
    add("n_rows", sc.DEFAULT, sc.XTRA, _n_rows(), (4, 8, 12))
    add("n_rows_g5241", sc.DEFAULT_G5241, sc.XTRA, _n_rows(), (12, 8))
    add("with_151", sc.DEFAULT, sc.XTRA, _with_151(), (8, 13))
    for name, (b, _) in out.items():
        assert 16 <= len(b.pairs) < 100 and all(len(q) <= HW_QMAX + 1 for q, _, _ in b.pairs), name
    return out


TABLES = _tables()
SMALL_N = tuple(range(1, 10))      # batches of n = 1..9 jobs: an odd unit count, a last unit of one job, one unit of two obtained


def _ways(name):
    """the batches of a table: (key, batch) -- the lone batch, then its chunks"""
    batch, sizes = TABLES[name]
    out = [(f"{name}|lone", batch)]
    # fifteen jobs from every sixteen: the quartets stay where they are in the table, and eight units make the ring's workers pair them
    for at in range(0, len(batch.pairs) - 2, 16):
        out.append((f"{name}|c15_{at}", sc.Batch(f"{batch.name}[{at}:{at + 15}]", batch.scoring, batch.xtra, batch.pairs[at:at + 15], batch.tags[at:at + 15])))
    out += [(f"{name}|chunk{k}", b) for k, b in enumerate(sc.chunks(batch, sizes))]
    if name == "lengths_odd_chunks":
        out += [(f"{name}|n{n}", sc.Batch(f"{batch.name}[:{n}]", batch.scoring, batch.xtra, batch.pairs[:n], batch.tags[:n])) for n in SMALL_N]
    return out


def _call(ctx, batch):
    s0 = ctx.ring_stats()[1]
    got = ctx.swalign2_batch(sc.apply(bpsw_hip.default_opt(), batch.scoring), batch.xtra, **sc.jobs_from(batch.pairs))
    return got, ctx.ring_stats()[1] - s0


# ---- this process ----------------------------------------------------------------------------------------------------------------
GOT = {}          # key -> the (n, 7) array this process got
REACHED = {}      # form -> keys


@pytest.fixture(scope="module", autouse=True)
def _quiet_device():
    """the lone-launch rule of sw_stage_run asks for no extension call on the device in the last 20 ms; once, before the first table"""
    time.sleep(0.03)


def _form(batch, through_ring):
    """the form a batch takes BY THE HOST'S RULES, restated (launch_sw_kernel, sw_stage_run's choice of the ring class): the library reports no kernel
    name.  The ring's counter says whether a batch went through the ring; nothing says whether a worker paired its units -- the results
    and the counter are the same either way -- so REACHED records what the dispatch is written to do, not a proof that it did."""
    n, mq, _ = sc.geometry(batch)
    if through_ring:
        return "half-wave ring, two units" if mq <= HW_QMAX and (n + 1) // 2 >= PAIR_MIN_UNITS else "ring, a single unit"
    if mq <= HW_QMAX and n > 2:
        return "half-wave launch"
    return "swp_kernel<3>" if HW_QMAX < mq <= 171 and n > 1 else "other"


def _run_table(ctx, orc, name):
    for key, batch in _ways(name):
        if key in GOT:
            continue
        want = sc.want(orc, batch)
        got, moved = _call(ctx, batch)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (f"{key} / {batch.scoring.name}: {bad.size}/{len(want)} jobs differ, first {bad[:5]} {[batch.tags[k] for k in bad[:5]]}: "
                               f"got {got[bad[:3]]} want {want[bad[:3]]}")
        ring = sc.takes_ring(batch, os.environ)
        assert moved == (1 if ring else 0), f"{key}: {len(batch.pairs)} jobs went {'through the ring' if moved else 'through a launch'}"
        GOT[key] = got
        REACHED.setdefault(_form(batch, ring), []).append(key)


@pytest.mark.parametrize("name", list(TABLES))
def test_table(ctx, orc, name):
    _run_table(ctx, orc, name)
    keys = [k for k, _ in _ways(name)]
    launch, two, one = (REACHED.get(f, []) for f in ("half-wave launch", "half-wave ring, two units", "ring, a single unit"))
    assert keys[0] in (REACHED.get("swp_kernel<3>", []) if name == "with_151" else launch)
    if name.startswith("rows1") and name != "rows1024":       # a chunk that holds the long window is a launch too
        assert any(k in launch for k in keys[1:]) and any(k in one for k in keys[1:])
    else:
        assert all(k in two + one for k in keys[1:]) and any(k in two for k in keys[1:]) and any(k in one for k in keys[1:])


def test_weak_half_equals_the_pair_run_alone(ctx, orc):
    """half isolation, said directly: the pair beside the strong job, run as a batch of its own (one unit: the pair-per-wave form), gives the
    seven fields it gave inside the quartet"""
    _run_table(ctx, orc, "isolation")
    batch, _ = TABLES["isolation"]
    inside = GOT["isolation|lone"]
    for q in range(len(batch.pairs) // 4):
        strong = next(k for k in range(4) if batch.tags[4 * q + k][0] == "strong")
        at = 4 * q + 2 * (1 - strong // 2)
        alone, moved = _call(ctx, sc.Batch("weak_pair", batch.scoring, batch.xtra, batch.pairs[at:at + 2], batch.tags[at:at + 2]))
        assert moved == 1
        assert np.array_equal(alone, inside[at:at + 2]), (q, strong, alone, inside[at:at + 2])
        assert inside[4 * q + strong][0] == 2 * STRONG and inside[4 * q + strong][1] == 599      # the copy ends in the window's last row


def test_a_151_base_mate_takes_the_pair_form(ctx, orc):
    _run_table(ctx, orc, "with_151")
    batch, _ = TABLES["with_151"]
    assert sc.geometry(batch)[1] == HW_QMAX + 1 and "with_151|lone" in REACHED.get("swp_kernel<3>", [])
    assert "with_151|c15_0" in REACHED.get("half-wave ring, two units", [])      # (a chunk without it: no mate above 150 bases)
    assert "with_151|c15_16" in REACHED.get("ring, a single unit", [])


# ---- the other forms: child processes --------------------------------------------------------------------------------------------
CHILD_ENV = {"duo": {"BPSW_SW_HALVES": "0"}, "ring_always": {"BPSW_RING_LONE_LAUNCH": "0"}, "keys_hbm": {"BPSW_SW_KEYS_LDS": "0", "BPSW_RING": "0"}}
CHILD_TABLES = {"duo": list(TABLES), "ring_always": list(TABLES), "keys_hbm": ["lengths", "lengths_odd_chunks", "lengths_m2x3_g5241", "rows1536", "rows1537", "isolation", "stops", "n_rows"]}


def child_main(mode, path):
    """the same batches in a process with another switch, against the arrays the default process got"""
    ctx = bpsw_hip.Context(0)
    stored = np.load(path)
    bad, n = [], 0
    try:
        for name in CHILD_TABLES[mode]:
            for key, batch in _ways(name):
                got, moved = _call(ctx, batch)
                if moved != (1 if sc.takes_ring(batch, os.environ) else 0):
                    bad.append(f"{key}: went the other way (the ring's counter moved by {moved})")
                if not np.array_equal(got, stored[key]):
                    rows = np.nonzero((got != stored[key]).any(axis=1))[0]
                    bad.append(f"{key}: the two forms DIVERGE on jobs {rows[:5]} {[batch.tags[k] for k in rows[:5]]}: here {got[rows[:3]]} default process {stored[key][rows[:3]]}")
                n += 1
    finally:
        ctx.close()
    print(f"child {mode}: {n} batches compared, {len(bad)} differ")
    for line in bad[:10]:
        print(line)
    return 1 if bad else 0


@pytest.mark.parametrize("mode", list(CHILD_ENV))
def test_other_form_gives_the_same_arrays(ctx, orc, tmp_path, mode):
    """duo: BPSW_SW_HALVES=0, every batch in the pair-per-wave form, as a launch and through the ring as here.  ring_always: the lone
    batches through the ring too, two units per ticket.  keys_hbm: the half-wave launch with its two key rows in HBM scratch, for the lone
    batches and for the chunks (n = 3..15: trailing pairs, a missing position)."""
    for name in CHILD_TABLES[mode]:
        _run_table(ctx, orc, name)
    path = os.path.join(str(tmp_path), "default_process.npz")
    np.savez(path, **{k: v for k, v in GOT.items() if k.split("|")[0] in CHILD_TABLES[mode]})
    env = {k: v for k, v in os.environ.items() if k not in ("BPSW_SW_HALVES", "BPSW_SW_KEYS_LDS", "BPSW_RING", "BPSW_RING_LONE_LAUNCH")}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, path], env=dict(env, **CHILD_ENV[mode]), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " 0 differ" in r.stdout, r.stdout[-500:]


def test_forms_reached():
    """which forms this process ran, from the tables' definitions (mate lengths and batch sizes) and the ring's counter -- by the
    restated rules of _form, see there: were no batch ever sent to the half-wave ring class, this test would not notice.  It returns without asserting under a
    narrower selection of this file's tests."""
    if not set(TABLES) <= {k.split("|")[0] for k in GOT}:
        return
    for form in ("half-wave launch", "half-wave ring, two units", "ring, a single unit", "swp_kernel<3>"):
        assert REACHED.get(form), f"not reached: {form}"
    assert "other" not in REACHED, REACHED["other"]
    sizes = {len(b.pairs) for name in TABLES for _, b in _ways(name)}
    assert set(SMALL_N) <= sizes and {n % 4 for n in sizes} == {0, 1, 2, 3}


if __name__ == "__main__":
    sys.exit(child_main(sys.argv[1], sys.argv[2]))
