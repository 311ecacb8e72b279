"""The exact divider of the render kernels' pixel bookkeeping (amber_amd/csrc/hip/exact_div.h) against `/` and `%` on the host (no GPU needed).

A stand-alone program (tests/exact_division_main.cc: its own main, the host compiler, nothing of the library, nothing loaded into python)
includes the header and checks quotient and remainder for the divisors 1, 2, 3, 5, 7, 8, 63, 64, 65, 1000, 1023, 1024, 1025, 3840, 65535,
65536, 65537, 2^31 - 1, 2^31, 2^31 + 1, 2^32 - 1 and 10 000 seeded random ones, each with the dividends 0, 1, d - 1, d, d + 1, k * d - 1,
k * d, k * d + 1 for 64 seeded k, 2^31 - 1, 2^31 + 1, 2^32 - 2, 2^32 - 1 and 10 000 seeded random ones.  Built twice: -O2, and -O2 with
AddressSanitizer + UBSan.  Zero mismatches, and no sanitizer report."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CXX = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)


@pytest.mark.parametrize("sanitize", [False, True], ids=["O2", "O2-asan-ubsan"])
def test_quotient_and_remainder_equal_the_hardware_division(tmp_path, sanitize):
    assert CXX is not None, "no host C++ compiler (c++, g++, clang++): the divider's exhaustive check cannot run"
    exe = tmp_path / "exact_division"
    flags = ["-O2", "-std=c++17", "-Wall", "-Werror"] + (["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else [])
    subprocess.run([CXX, *flags, "-I", str(ROOT / "amber_amd" / "csrc" / "hip"), "-o", str(exe), str(ROOT / "tests" / "exact_division_main.cc")],
                   check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print("\n" + r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"divisors (\d+), pairs checked (\d+), mismatches (\d+)", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) == 21 + 10000 and int(m.group(2)) > 10021 * 10000 and int(m.group(3)) == 0
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
