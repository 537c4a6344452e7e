"""The recipe of the stand-alone sanitizer programs (tests/native/*_sanitize.cpp): host sources
compiled with clang under AddressSanitizer + UndefinedBehaviorSanitizer into a program with its own
main, which is then run.  Nothing is loaded into Python and nothing runs on the GPU."""
from __future__ import annotations

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
CSRC = os.path.join(ROOT, "of-spmm_amd", "csrc")

FLAGS = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-fopenmp", "-ffp-contract=off", "-Wall", "-Werror",
         "-Wno-unknown-pragmas", "-Wno-duplicate-decl-specifier"]


def build_and_run(tmp_path, program, csrc_sources, flags=("-Wno-unused-function",)):
    """Builds tests/native/<program>.cpp with the named files of csrc/ and runs it: exit code 0,
    "OK" as the last word on stdout and no UBSan report."""
    exe = tmp_path / program
    subprocess.run([CLANG, *FLAGS, *flags, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", program + ".cpp"),
                    *[os.path.join(CSRC, s) for s in csrc_sources], "-o", str(exe)], check=True)
    supp = tmp_path / "lsan.supp"
    supp.write_text("leak:___kmp_allocate\n")  # the OpenMP runtime's own thread-pool state
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               LSAN_OPTIONS=f"suppressions={supp}", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK") and "runtime error" not in r.stderr, r.stdout + r.stderr
