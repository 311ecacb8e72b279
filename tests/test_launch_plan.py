"""The arithmetic that splits a render pass into launches (amber_amd/csrc/hip/launch_plan.h): samples per launch and record slots (no GPU needed).

A stand-alone program (tests/launch_plan_main.cc: its own main, the host compiler, nothing of the library, nothing loaded into python) includes
the header alone and compares the path, item and light launches it plans -- the probe launch, density x 1.5, the shorter launches of a dense
scene, the test hook, bands too large for one launch, nothing and one sample left -- with values worked out by hand from the launch loops the
arithmetic came from.  Built twice: -O2, and -O2 with AddressSanitizer + UBSan.  Zero failures, and no sanitizer report."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CXX = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)


@pytest.mark.parametrize("sanitize", [False, True], ids=["O2", "O2-asan-ubsan"])
def test_launches_are_planned_as_worked_out_by_hand(tmp_path, sanitize):
    assert CXX is not None, "no host C++ compiler (c++, g++, clang++): the launch plan's check cannot run"
    exe = tmp_path / "launch_plan"
    flags = ["-O2", "-std=c++17", "-Wall", "-Werror"] + (["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else [])
    subprocess.run([CXX, *flags, "-I", str(ROOT / "amber_amd" / "csrc" / "hip"), "-o", str(exe), str(ROOT / "tests" / "launch_plan_main.cc")],
                   check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print("\n" + r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"cases (\d+), failures (\d+)", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) == 29 and int(m.group(2)) == 0
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
