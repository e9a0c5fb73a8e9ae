"""What the SAM entries refuse, and with which words: bpsw_sam_se_batch, bpsw_align_se_batch, bpsw_sam_pe_batch, bpsw_sam_pe_batch_ex
(text on the calling thread and on the device), bpsw_align_pe_batch and bpsw_worker2_batch.

A characterisation table: each row is an input that the library turns away before it launches anything, with the return code and
the exact bpsw_last_error text.  The text-capacity rows run two reads or one pair without regions (two unaligned records), so all
they launch is the seeding of worker1 and the two text kernels.  Inputs that an entry does not check are not in the table: name
offsets and id_step in paired mode, the flags of the align entries' tail (looked at only after worker1 ran), an empty or
out-of-pool read and a null region array in bpsw_worker2_batch (the rescue reads them first)."""
import ctypes as C

import numpy as np
import pytest

import bpsw_hip
import fmi_util as fu
from bpsw_hip import PeStat, Pairs, SeReads

pytestmark = pytest.mark.gpu

ARG, CAPACITY = -1, -3
DEV = bpsw_hip.SAM_TEXT_DEVICE
L_PAC = 1500


@pytest.fixture(scope="module")
def loaded(ctx):
    """a 1 500-base reference with its contig table and index on the context's device"""
    g = np.random.default_rng(1500).integers(0, 4, L_PAC).astype(np.uint8)
    idx, _ = fu.build_index(g, 8)
    ctx.ref_load(fu.pack_pac(g), L_PAC)
    ctx.bns_load(np.array([0], np.int64), np.array([L_PAC], np.int32), ["chrA"])
    ctx.fmi_load(idx)
    yield ctx
    ctx.fmi_unload()


class Batch:
    """two reads (single-end) or one pair, 40 bases each, without regions; the arrays stay alive with the object"""

    def __init__(self, paired, **over):
        rng = np.random.default_rng(7)
        self.a = dict(read_len=np.array([40, 40], np.int32), read_off=np.array([0, 40], np.int64),
                      read_pool=rng.integers(0, 4, 80).astype(np.uint8), qual_pool=np.full(80, 70, np.uint8),
                      name_off=np.array([0, 2, 4] if not paired else [0, 2], np.int64), name_pool=np.frombuffer(b"r0r1\0", np.uint8).copy(),
                      reg_cnt=np.zeros(2, np.int32), regs=None)
        self.st = st = Pairs() if paired else SeReads()
        if paired:
            st.group_size, st.id0 = 1, 3
            for r in range(4):
                st.pes[r].failed = 1
        else:
            st.n_reads, st.id0, st.id_step = 2, 3, 1
        st.read_pool_bytes = 80
        scalars = ("n_reads", "group_size", "id_step", "read_pool_bytes")
        for k, v in over.items():
            if k in scalars:
                setattr(st, k, v)
            else:
                self.a[k] = v if v is None or isinstance(v, np.ndarray) else np.array(v, self.a[k].dtype)
        for k, v in self.a.items():
            setattr(st, k, None if v is None else v.ctypes.data)


class Out:
    def __init__(self, cap=4096):
        self.buf = np.zeros(max(cap, 1), np.uint8)
        self.cap = cap
        self.off = np.full(3, -1, np.int64)
        self.need = C.c_size_t(77)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# the entries as call(lib, h, opt, sopt, topt, g, flags, buf, cap, off, need); any pointer may be None
def _sam_se(lib, h, opt, sopt, topt, g, flags, buf, cap, off, need):
    return lib.bpsw_sam_se_batch(h, opt, topt, g, flags, buf, cap, off, need, None)


def _align_se(lib, h, opt, sopt, topt, g, flags, buf, cap, off, need):
    return lib.bpsw_align_se_batch(h, opt, sopt, topt, g, 0, 0, flags, buf, cap, off, need)


def _sam_pe(lib, h, opt, sopt, topt, g, flags, buf, cap, off, need):
    return lib.bpsw_sam_pe_batch(h, opt, topt, g, buf, cap, off, need, None)


def _sam_pe_ex(lib, h, opt, sopt, topt, g, flags, buf, cap, off, need):
    return lib.bpsw_sam_pe_batch_ex(h, opt, topt, g, flags, buf, cap, off, need, None)


def _align_pe(lib, h, opt, sopt, topt, g, flags, buf, cap, off, need):
    return lib.bpsw_align_pe_batch(h, opt, sopt, topt, g, None, 0, 0, bpsw_hip.RESCUE_C, flags, buf, cap, off, need, None)


def _worker2(lib, h, opt, sopt, topt, g, flags, buf, cap, off, need):
    return lib.bpsw_worker2_batch(h, opt, topt, g, bpsw_hip.RESCUE_C, buf, cap, off, need, None, None, 0, None)


# name -> (call, paired, flags of a good call, who, the who of its tail, takes sopt)
ENTRIES = {
    "sam_se": (_sam_se, False, 0, "sam_se", "sam_se", False),
    "sam_se_dev": (_sam_se, False, DEV, "sam_se", "sam_se", False),
    "align_se": (_align_se, False, 0, "align_se", "sam_se", True),
    "sam_pe": (_sam_pe, True, 0, "sam_pe", "sam_pe", False),
    "sam_pe_ex": (_sam_pe_ex, True, 0, "sam_pe", "sam_pe", False),
    "sam_pe_ex_dev": (_sam_pe_ex, True, DEV, "sam_pe", "sam_pe", False),
    "align_pe": (_align_pe, True, 0, "align_pe", "sam_pe", True),
    "worker2": (_worker2, True, 0, "worker2", "sam_pe", False),
}
TAILS = ("sam_se", "sam_se_dev", "sam_pe", "sam_pe_ex", "sam_pe_ex_dev")   # the entries that take region lists and check them
SIZE = {False: ("n_reads", "negative number of reads"), True: ("group_size", "negative group size")}


def _run(ctx, entry, batch, flags=None, out=None, null=()):
    """one call with the pieces named in `null` passed as NULL -> (rc, last error, Out)"""
    call, paired, good_flags = ENTRIES[entry][:3]
    out = out or Out()
    opt, sopt, topt = bpsw_hip.default_opt(), bpsw_hip.default_seed_opt(), bpsw_hip.default_tail_opt()
    arg = dict(h=ctx.h, opt=C.byref(opt), sopt=C.byref(sopt), topt=C.byref(topt), g=C.byref(batch.st), off=_p(out.off), buf=_p(out.buf))
    for k in null:
        arg[k] = None
    rc = call(ctx.lib, arg["h"], arg["opt"], arg["sopt"], arg["topt"], arg["g"], good_flags if flags is None else flags, arg["buf"],
              out.cap, arg["off"], C.byref(out.need))
    return rc, ctx.lib.bpsw_last_error().decode(), out


def _refused(ctx, entry, batch, code, text, **kw):
    rc, err, _ = _run(ctx, entry, batch, **kw)
    assert (rc, err) == (code, text), (entry, rc, err)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_null_arguments(loaded, entry):
    _, paired, _, who, _, takes_sopt = ENTRIES[entry]
    b = Batch(paired)
    own = ["h", "g", "off", "topt"] + (["opt"] if who in ("align_se", "align_pe", "worker2") else []) + (["sopt"] if takes_sopt else [])
    for k in own:
        _refused(loaded, entry, b, ARG, f"{who}: null argument", null=(k,))
    if "opt" not in own:   # the tail entries leave the options to the scoring check
        _refused(loaded, entry, b, ARG, "tail: null options", null=("opt",))


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_null_arrays(loaded, entry):
    paired, who = ENTRIES[entry][1], ENTRIES[entry][3]
    text = f"{who}: null read arrays" if not paired else f"{who}: null group arrays"
    arrays = ["read_len", "read_off", "read_pool"]
    if entry != "worker2":
        arrays += ["name_off", "name_pool"]
    if entry in ("sam_pe", "sam_pe_ex", "sam_pe_ex_dev", "worker2"):
        arrays.append("reg_cnt")
    for f in arrays:
        _refused(loaded, entry, Batch(paired, **{f: None}), ARG, text)
    if entry in ("sam_se", "sam_se_dev"):
        _refused(loaded, entry, Batch(paired, reg_cnt=None), ARG, "sam_se: null region counts")


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_negative_batch_size(loaded, entry):
    paired, who = ENTRIES[entry][1], ENTRIES[entry][3]
    field, text = SIZE[paired]
    _refused(loaded, entry, Batch(paired, **{field: -1}), ARG, f"{who}: {text}")


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e != "worker2"])
def test_empty_batch(loaded, entry):
    paired = ENTRIES[entry][1]
    rc, _, out = _run(loaded, entry, Batch(paired, **{SIZE[paired][0]: 0}))
    assert rc == 0 and out.off[0] == 0 and out.need.value == 0


def test_empty_batch_align_pe_statistics(loaded):
    """out_pes of an empty batch: the statistics handed in, or those of no pairs at all (every orientation failed)"""
    lib = loaded.lib
    opt, sopt, topt = bpsw_hip.default_opt(), bpsw_hip.default_seed_opt(), bpsw_hip.default_tail_opt()
    b, out = Batch(True, group_size=0), Out()
    given = (PeStat * 4)()
    for r in range(4):
        given[r].low, given[r].high, given[r].failed, given[r].avg, given[r].std = 10 + r, 500 + r, r & 1, 250.5 + r, 30.25 + r
    for pes0 in (given, None):
        got = (PeStat * 4)()
        rc = lib.bpsw_align_pe_batch(loaded.h, C.byref(opt), C.byref(sopt), C.byref(topt), C.byref(b.st), pes0, 0, 0, bpsw_hip.RESCUE_C, 0,
                                     _p(out.buf), out.cap, _p(out.off), C.byref(out.need), got)
        assert rc == 0 and out.off[0] == 0 and out.need.value == 0
        have = [(got[r].low, got[r].high, got[r].failed, got[r].avg, got[r].std) for r in range(4)]
        want = [(10 + r, 500 + r, r & 1, 250.5 + r, 30.25 + r) for r in range(4)] if pes0 is not None else [(0, 0, 1, 0.0, 0.0)] * 4
        assert have == want


@pytest.mark.parametrize("entry", list(TAILS) + ["worker2"])
def test_negative_region_count(loaded, entry):
    paired, who = ENTRIES[entry][1], ENTRIES[entry][3]
    _refused(loaded, entry, Batch(paired, reg_cnt=[0, -1]), ARG, f"{who}: negative region count")


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e != "worker2"])
def test_read_empty_or_outside_its_pool(loaded, entry):
    paired, who = ENTRIES[entry][1], ENTRIES[entry][3]
    text = f"{who}: read outside its pool (or empty)"
    _refused(loaded, entry, Batch(paired, read_len=[40, 0]), ARG, text)
    _refused(loaded, entry, Batch(paired, read_len=[40, 41]), ARG, text)      # one byte past the pool
    _refused(loaded, entry, Batch(paired, read_pool_bytes=79), ARG, text)
    _refused(loaded, entry, Batch(paired, read_off=[0, -1]), ARG, text)


@pytest.mark.parametrize("entry", ["sam_se", "sam_se_dev", "align_se"])
def test_single_end_names_and_ids(loaded, entry):
    who = ENTRIES[entry][3]
    _refused(loaded, entry, Batch(False, name_off=[0, 4, 2]), ARG, f"{who}: name offsets must ascend")
    _refused(loaded, entry, Batch(False, name_off=[-1, 2, 4]), ARG, f"{who}: name offsets must ascend")
    _refused(loaded, entry, Batch(False, id_step=-1), ARG, f"{who}: negative id_step")


@pytest.mark.parametrize("entry", ["sam_se", "sam_se_dev", "sam_pe_ex", "sam_pe_ex_dev", "align_pe"])
def test_unknown_flag(loaded, entry):
    _, paired, good, who = ENTRIES[entry][:4]
    for flags in (2, good | 0x40, -1 & ~DEV):
        _refused(loaded, entry, Batch(paired), ARG, f"{who}: unknown flag", flags=flags)


@pytest.mark.parametrize("entry", TAILS)
def test_null_region_array(loaded, entry):
    paired, who = ENTRIES[entry][1], ENTRIES[entry][3]
    _refused(loaded, entry, Batch(paired, reg_cnt=[1, 0]), ARG, f"{who}: null region array")


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_text_capacity(loaded, entry):
    """a buffer one byte short and no buffer at all: BPSW_ERR_CAPACITY, *out_needed and out_off as of the call that fits"""
    paired, tail = ENTRIES[entry][1], ENTRIES[entry][4]
    b = Batch(paired)
    rc, _, fits = _run(loaded, entry, b)
    assert rc == 0, loaded.lib.bpsw_last_error()
    need = int(fits.need.value)
    assert need == fits.off[2] > fits.off[1] > fits.off[0] == 0
    text = f"{tail}: text buffer too small (see *out_needed)"
    rc, err, short = _run(loaded, entry, b, out=Out(need - 1))
    assert (rc, err) == (CAPACITY, text) and short.need.value == need and np.array_equal(short.off, fits.off)
    rc, err, none = _run(loaded, entry, b, out=Out(need), null=("buf",))
    assert (rc, err) == (CAPACITY, text) and none.need.value == need and np.array_equal(none.off, fits.off)
    rc, _, exact = _run(loaded, entry, b, out=Out(need))
    assert rc == 0 and exact.buf[:need].tobytes() == fits.buf[:need].tobytes()
