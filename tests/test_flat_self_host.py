"""The flat-self shortcut of the two-phase engine on the host (tests/cpp/flat_self_check.hip): which program triangles the host marks, and the
theorem the shortcut rests on -- a ray that starts at ResolveHit's pos of a marked triangle gets t = +-0 or NaN from that triangle, whatever its
direction -- on random marked triangles in a restatement of the kernels' binary32 operations.  The program runs once plain and once under
AddressSanitizer + UBSan (host code only; a stand-alone program, nothing is preloaded)."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_flat_self_host(tmp_path, sanitize):
    exe = tmp_path / "flat_self_check"
    lib = ROOT / "amber_amd" / "lib"
    # the Cornell box comes from the host model (amber_host.cc), which references the C ABI: resolved against the real library, never called
    flags = ["-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = ["hipcc", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + flags + \
          ["-o", str(exe), str(ROOT / "tests" / "cpp" / "flat_self_check.hip"), str(ROOT / "amber_amd" / "csrc" / "amber" / "amber_host.cc"),
           "-L" + str(lib), "-lamber_hip", "-Wl,-rpath," + str(lib)]
    subprocess.run(["make", "-C", str(ROOT / "amber_amd" / "csrc")], check=True, capture_output=True)
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env={"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0", "PATH": "/usr/bin:/bin", "LD_LIBRARY_PATH": "/opt/rocm/lib"})
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
