"""csrc/bpsw_sam_core.h WITH A MATE -- the bytes of a paired SAM line, what sam_len_kernel and sam_write_kernel (csrc/bpsw_sam_se.hip)
compile for bpsw_sam_pe_batch_ex -- on the HOST: tests/sam_pe_host/sam_pe_host.cpp holds it against an independent snprintf-based
writer of mem_aln2sam with m != NULL over more than 20 000 generated lines in pairs of reads, as a program of its own under
-fsanitize=address,undefined (every line written into a heap block of exactly its length), and asserts what the core relies on:
the mate record the tail prints against is the first line of the other read.  No GPU, no Python in the sanitized process.  The
same file must also compile for gfx950."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "sam_pe_host", "sam_pe_host.cpp")
HDR = os.path.join(ROOT, "cloud-scale-bwamem_amd", "csrc", "bpsw_sam_core.h")
OUT = os.path.join(HERE, "sam_pe_host", "_build")
INC = ["-I" + os.path.dirname(HDR)]


def _fresh(target):
    return os.path.exists(target) and os.path.getmtime(target) >= max(os.path.getmtime(SRC), os.path.getmtime(HDR))


def test_core_with_a_mate_equals_an_independent_writer_under_address_and_undefined_sanitizers():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "sam_pe_host_san")
    if not _fresh(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"] + INC + ["-o", exe, SRC], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "sam core with a mate:" in p.stdout and "equal to the independent writer" in p.stdout, p.stdout


def test_core_with_a_mate_compiles_for_gfx950_in_both_kernels():
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} not found: the device build of bpsw_sam_core.h cannot be checked")
    os.makedirs(OUT, exist_ok=True)
    obj = os.path.join(OUT, "sam_pe_host_gfx950.o")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Werror", "-x", "hip", "-c"] + INC + ["-o", obj, SRC],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
