"""The seeding plan on the device, as far as it can be held without one: the per-read arithmetic of csrc/bpsw_seed_plan_core.h
(what seed_plan_count_kernel and seed_plan_fill_kernel call) compiled for the HOST in a program of its own
(tests/seed_plan_host/seed_plan_host.cpp) under -fsanitize=address,undefined, with a sequential scan between count and fill,
against the loop seed_run runs on the calling thread -- on 10 007 generated reads: without intervals, with exactly 16 and with more
(second-pass rows), rows with nothing kept, kept zero-width intervals first, last and in runs, x2 up to 2^31 - 1 so that the sums pass
2^32.  And the device scan (csrc/bpsw_scan.hip) compiles for gfx950 without scratch memory."""
import os
import re
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "cloud-scale-bwamem_amd", "csrc")
SRC = os.path.join(HERE, "seed_plan_host", "seed_plan_host.cpp")
HDR = os.path.join(CSRC, "bpsw_seed_plan_core.h")
OUT = os.path.join(HERE, "seed_plan_host", "_build")
INC = ["-I" + CSRC, "-I" + os.path.join(ROOT, "include")]
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _fresh(target, *deps):
    return os.path.exists(target) and os.path.getmtime(target) >= max(os.path.getmtime(d) for d in deps)


def test_plan_core_under_address_and_undefined_sanitizers():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "seed_plan_host_san")
    if not _fresh(exe, SRC, HDR):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"] + INC + ["-o", exe, SRC], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"seed plan core: (\d+) reads, (\d+) in the second pass, (\d+) intervals, (\d+) kept \((\d+) of zero width\), (\d+) occurrences: equal",
                  p.stdout)
    assert m, p.stdout
    reads, second, intervals, kept, zero, occ = (int(x) for x in m.groups())
    assert reads >= 10_000 and second > 500 and 0 < kept < intervals and zero > 1000 and occ > 2**32


def test_the_scan_compiles_for_gfx950_without_scratch():
    os.makedirs(OUT, exist_ok=True)
    src = os.path.join(CSRC, "bpsw_scan.hip")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Werror", "-Rpass-analysis=kernel-resource-usage"] + INC +
                       ["-c", src, "-o", os.path.join(OUT, "bpsw_scan.o")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    names = re.findall(r"Function Name: (\S+)", p.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stderr)]
    for k in ("scan_reduce_kernel", "scan_tiles_kernel", "scan_apply_kernel"):
        assert any(k in nm for nm in names), (k, names)
    assert len(scratch) == len(names) and not any(scratch), list(zip(names, scratch))
