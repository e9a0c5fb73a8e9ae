"""The staged block (csrc/bpsw_stage.h: StageLayout, StageIn, StageOut) compiled for the HOST as a stand-alone program
(tests/stage_host/stage_host.cpp) with AddressSanitizer and UBSan, and run: part offsets against the closed form the kernels index
by, parts inside the block and clear of each other, parts without bytes or without a source skipped, a smaller block staged over a
larger one, and the literal offsets of sw_stage_begin's block for five jobs.  No GPU and nothing preloaded: the program has its own
main, the two buffer types are stand-ins that allocate exactly what is asked for, hipMemcpyAsync is a memcpy."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "cloud-scale-bwamem_amd", "csrc")


def test_stage_host_under_asan_and_ubsan():
    out = os.path.join(HERE, "stage_host", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "stage_host")
    src = os.path.join(HERE, "stage_host", "stage_host.cpp")
    hdr = os.path.join(CSRC, "bpsw_stage.h")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan",   # the runtimes inside the program: nothing about the process's library order matters
                        "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + CSRC, "-o", exe, src], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "stage_host OK" in r.stdout, r.stdout[-4000:]
