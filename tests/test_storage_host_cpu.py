"""claymore_amd/csrc/mpm_storage.hpp on the host: the owning buffers every device array of the engine lives in, over malloc / free stand-ins
for the runtime calls (tools/hostcheck/hip/hip_runtime.h), under a sanitizer in a stand-alone program."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

HOSTCHECK = os.path.join(ROOT, "tools", "hostcheck")


def test_storage_selftest_runs_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tools/hostcheck/storage_selftest.cpp - a program of its own that includes only the header - built with -fsanitize=address,undefined and
    run as a child process: alloc(0), the zero fill, grow's copy and tail, every failure half-way through a growth, moves, reset, a
    std::vector of structs of buffers that reallocates, and no allocation left at exit.  Nothing sanitised is loaded into this process."""
    exe = str(tmp_path / "storage_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + HOSTCHECK,
                           "-I" + entry.CSRC, "-o", exe, os.path.join(HOSTCHECK, "storage_selftest.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "storage_selftest ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
