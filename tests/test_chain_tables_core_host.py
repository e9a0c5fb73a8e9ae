"""The resident chains, as far as they can be held without a device: the per-read arithmetic of csrc/bpsw_chain_tables_core.h
(what chain_tables_kernel calls) compiled for the HOST in a program of its own (tests/chain_tables_host/chain_tables_host.cpp,
with csrc/bpsw_chain.cpp for bpsw_chain_seeds) under -fsanitize=address,undefined: generated reads -- without seeds first, last
and in runs, one of 3 000 seeds, one of 2 000 single-seed chains -- are chained, pooled the way the chain stage pools them, scanned
sequentially and put through the table function, against the arrays bpsw_chain2aln_batch's host loop builds from the same chains.
And csrc/bpsw_chain_dev.hip compiles for gfx950 with its new kernels free of scratch memory."""
import os
import re
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "cloud-scale-bwamem_amd", "csrc")
SRC = os.path.join(HERE, "chain_tables_host", "chain_tables_host.cpp")
HDR = os.path.join(CSRC, "bpsw_chain_tables_core.h")
CHAIN = os.path.join(CSRC, "bpsw_chain.cpp")
OUT = os.path.join(HERE, "chain_tables_host", "_build")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HIP_INC = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "include")   # bpsw_chain.cpp includes the internal header
if not os.path.isdir(os.path.join(HIP_INC, "hip")):
    HIP_INC = "/opt/rocm/include"      # (where tests/host_san/Makefile looks)
INC = ["-I" + CSRC, "-I" + os.path.join(ROOT, "include")]


def _fresh(target, *deps):
    return os.path.exists(target) and os.path.getmtime(target) >= max(os.path.getmtime(d) for d in deps)


def test_tables_core_under_address_and_undefined_sanitizers():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "chain_tables_host_san")
    if not _fresh(exe, SRC, HDR, CHAIN):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-D__HIP_PLATFORM_AMD__", "-DHIP_INCLUDE_HIP_HIP_EXT_H"] + INC + ["-isystem", HIP_INC, "-o", exe, SRC, CHAIN, "-lpthread"], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"chain tables core: (\d+) reads, (\d+) without seeds, (\d+) without chains, (\d+) chains, (\d+) seeds, largest chain (\d+): equal",
                  p.stdout)
    assert m, p.stdout
    reads, empty, no_chain, chains, seeds, largest = (int(x) for x in m.groups())
    assert reads > 400 and empty > 20 and no_chain >= empty and chains > 2000 + 400 and seeds > chains and largest > 1


def test_the_chain_stage_compiles_for_gfx950_and_its_new_kernels_have_no_scratch():
    os.makedirs(OUT, exist_ok=True)
    src = os.path.join(CSRC, "bpsw_chain_dev.hip")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Werror", "-Wno-unused-function",
                        "-Rpass-analysis=kernel-resource-usage"] + INC + ["-c", src, "-o", os.path.join(OUT, "bpsw_chain_dev.o")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    names = re.findall(r"Function Name: (\S+)", p.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stderr)]
    assert len(scratch) == len(names), (names, scratch)
    for k in ("chain_emit_resident_kernel", "chain_host_merge_kernel", "chain_tables_kernel"):
        mine = [s for nm, s in zip(names, scratch) if k in nm]
        assert mine == [0], (k, list(zip(names, scratch)))
