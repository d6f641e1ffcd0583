"""CPU: what the host-side checks share -- the sanitizer build of a stand-alone tests/<name>.cpp and the library's exported
symbols.  The programs have their own main(): nothing is loaded into Python and nothing needs a device."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_under_sanitizers(name, tmp_path, timeout, args=()):
    """Builds tests/<name>.cpp with plain g++ under AddressSanitizer + UndefinedBehaviorSanitizer (warnings are errors), runs
    it with `args` and asserts that it ended clean: exit status 0, its "N checks passed" line, no report of either sanitizer.
    Skips without g++.  Returns the completed process."""
    if shutil.which("g++") is None:
        pytest.skip("g++ is not available")
    exe = tmp_path / name
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DEKF_HOST_ONLY",
           "-Wall", "-Werror", "-I", os.path.join(ROOT, "slam-duckietown_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", name + ".cpp"), "-o", str(exe)]
    if not exe.exists():                                              # (a second run with other arguments)
        built = subprocess.run(cmd, capture_output=True, text=True)
        assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=timeout,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert "checks passed" in run.stdout and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    return run


def exported_symbols(path):
    """The dynamic symbols the shared library at `path` defines: name -> nm's type letter ("T": a function)."""
    nm = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1]: ln.split()[-2] for ln in nm.splitlines() if len(ln.split()) >= 2}
