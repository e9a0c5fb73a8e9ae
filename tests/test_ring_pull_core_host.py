"""csrc/bpsw_ring_pull_core.h -- which byte ranges a resident rescue worker pulls for a unit, their widening to 16-byte chunks and the
slice layout -- on the HOST, and the resident kernels that compile it for gfx950.

tests/ring_pull_host/ring_pull_host.cpp is a program of its own under -fsanitize=address,undefined (no Python in the sanitized
process).  It plans and pulls every unit of generated job tables -- batches of 1, 2, 3, 4, 5, 15, 16 and 17 jobs, mates of 1, 149, 150,
151 and 256 bases, windows of 0, 1, 255, 256, 257, 1 023, 1 024, 1 535 and 1 536 rows at every alignment, one mate shared by four jobs,
coordinate mode, the last window on the block's last byte, and descriptors of random words -- out of a heap block of exactly the
block's length into a heap slice of exactly the class's capacity, and checks what its header comment lists.  The kernels that
compile the header must keep what they had: no scratch, no VGPR spill, the same waves per SIMD."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "ring_pull_host", "ring_pull_host.cpp")
CSRC = os.path.join(ROOT, "cloud-scale-bwamem_amd", "csrc")
HDR = os.path.join(CSRC, "bpsw_ring_pull_core.h")
OUT = os.path.join(HERE, "ring_pull_host", "_build")


def test_core_plans_and_pulls_every_unit_under_the_sanitizers():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "ring_pull_host_san")
    if not (os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(SRC), os.path.getmtime(HDR))):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-I" + CSRC, "-o", exe, SRC], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"ring pull core: (\d+) units planned, (\d+) pulled \((\d+) chunks\), (\d+) beyond their slice, (\d+) with a shared mate, "
                  r"(\d+) windows on the block's last byte", p.stdout)
    assert m, p.stdout
    units, pulled, chunks, misfit, shared, last = (int(x) for x in m.groups())
    assert units == pulled + misfit and pulled > 2000 and chunks > 100 * pulled // 10 and misfit > 20 and shared > 40 and last > 10


# waves per SIMD of the three resident kernels (the launch bounds of csrc/bpsw_swalign.hip: class 3, the half-wave class, class 5)
RESIDENT = {"swp_resident_kernelILi3ELb0E": 5, "swp_resident_kernelILi3ELb1E": 4, "swp_resident_kernelILi5ELb0E": 4}


def test_resident_kernels_compile_for_gfx950_without_scratch():
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail(f"{hipcc} not found: the device build of bpsw_ring_pull_core.h cannot be checked")
    os.makedirs(OUT, exist_ok=True)
    obj = os.path.join(OUT, "swalign_gfx950.o")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(CSRC, "bpsw_swalign.hip"), "-o", obj], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    remarks = p.stderr
    for kernel, waves in RESIDENT.items():
        m = re.search(r"Function Name: \S*" + kernel + r".*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?VGPRs Spill: (\d+)",
                      remarks, re.S)
        assert m, f"no resource remark for {kernel}:\n{remarks[-2000:]}"
        assert (int(m.group(1)), int(m.group(3))) == (0, 0), f"{kernel}: scratch {m.group(1)}, VGPR spills {m.group(3)}"
        assert int(m.group(2)) == waves, f"{kernel}: {m.group(2)} waves per SIMD, not {waves}"
