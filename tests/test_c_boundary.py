"""The guard of the C ABI (amber_amd/csrc/hip/c_boundary.h): no exception crosses an extern "C" function (no GPU needed).

A stand-alone program (tests/c_boundary_main.cc: its own main, the host compiler, nothing of the library, nothing loaded into python) includes
the header and runs Guarded over callables that return a code, throw std::bad_alloc, std::system_error, another std::exception and an int,
checking the code and the text of amber_hip_last_error() for each -- and std::bad_alloc once more under a global operator new that fails while
the handler runs: the code is still AMBER_ENOMEM, the message empty, nothing thrown, nothing terminated.  Built twice: -O2, and -O2 with
AddressSanitizer + UBSan.  Zero failures, and no sanitizer report."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CXX = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)


@pytest.mark.parametrize("sanitize", [False, True], ids=["O2", "O2-asan-ubsan"])
def test_no_exception_leaves_guarded(tmp_path, sanitize):
    assert CXX is not None, "no host C++ compiler (c++, g++, clang++): the guard's check cannot run"
    exe = tmp_path / "c_boundary"
    flags = ["-O2", "-std=c++17", "-Wall", "-Werror"] + (["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else [])
    subprocess.run([CXX, *flags, "-I", str(ROOT / "amber_amd" / "csrc" / "hip"), "-o", str(exe), str(ROOT / "tests" / "c_boundary_main.cc")],
                   check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print("\n" + r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"cases (\d+), failures (\d+)", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) == 7 and int(m.group(2)) == 0
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
