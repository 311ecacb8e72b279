"""Axis slabs of the Phase-A filter program on the host (tests/cpp/axis_slabs_check.hip): what the builder classes and how it stores it, and
equal candidate bits of the axis loops and the general slab loop in a host restatement of both.  The program runs once plain and once under
AddressSanitizer + UBSan (host code only; a stand-alone program, nothing is preloaded)."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_axis_slabs_host(tmp_path, sanitize):
    exe = tmp_path / "axis_slabs_check"
    lib = ROOT / "amber_amd" / "lib"
    # the Cornell box comes from the host model (amber_host.cc), which references the C ABI: resolved against the real library, never called
    flags = ["-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = ["hipcc", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + flags + \
          ["-o", str(exe), str(ROOT / "tests" / "cpp" / "axis_slabs_check.hip"), str(ROOT / "amber_amd" / "csrc" / "amber" / "amber_host.cc"),
           "-L" + str(lib), "-lamber_hip", "-Wl,-rpath," + str(lib)]
    subprocess.run(["make", "-C", str(ROOT / "amber_amd" / "csrc")], check=True, capture_output=True)
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env={"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0", "PATH": "/usr/bin:/bin", "LD_LIBRARY_PATH": "/opt/rocm/lib"})
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
