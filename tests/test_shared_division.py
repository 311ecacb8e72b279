"""The shared-denominator division of the render kernels (amber_amd/csrc/hip/shared_div.h) against `n / d` on the host (no GPU needed).

A stand-alone program (tests/shared_division_main.cc: its own main, the host compiler, nothing of the library, nothing loaded into python)
includes the header and runs the host restatement -- the reciprocal seed is a parameter there, v_rcp_f32 on the device:
  * 1.0e8 (numerator, denominator) pairs inside the guard's range (2^-20 <= |d| < 2^40, n = +-0 or
    2^-60 <= |n| < 2^41): every exponent pair with all-zeros, all-ones and neighbouring mantissas, n within 2 ulp of d, +-0 numerators, then
    seeded random pairs in which a quarter of the mantissas are all zeros, all ones or next to them; each pair with the seed at RN(1 / d) and
    one ulp either side of it;
  * the guards (SharedDivSafe3 / SharedDivSafe2 / SharedNormalizeSafe) against the range said in float compares: one ulp inside and outside
    every boundary in every slot, zeros, subnormals, inf, NaN, all-ones mantissas, and 2.0e7 groups of random bit patterns and random
    vectors; where Normalize's guard accepts, the components are below 2^41 (the bound it does not test) and the three quotients equal `/`.
Built twice: -O2 (1.0e8 pairs), and -O2 with AddressSanitizer + UBSan (1.0e7 pairs), run directly.

Figures of this program, one run (they do not depend on the machine):
  pairs checked 100000000, mismatches with the seed at RN 0, one ulp below 0, one ulp above 0, zero sign errors 0,
  guard cases 20017298, guard errors 0
A denominator with an all-ones mantissa (a sixteenth of the denominators here; Normalize's everyday case, the length just below 1 of a
vector that was unit length already) is the one kind for which the refinement depends on the last bit of its seed: n = 0x1p-13,
d = 0x1.fffffep-14, seed 0x1p+13 (RN(1 / d) = 0x1.000002p+13): the refined reciprocal 2^13 (1 + 2^-24) and then the corrected quotient
1 + 2^-24 are ties that round to even, back to where they started, and the refinement alone returns 1 where the quotient is
0x1.000002p+0 (407 925 of these 1.0e8 pairs, +-2^j / +-(2^k - ulp), with either off seed, none with the seed at RN).  SharedReciprocal
therefore returns RN(1 / d) itself for such a denominator, from its bits.  Beyond this program: 0 mismatches over all 2^24 numerators of
two binades under the all-ones denominators of nine binades and both signs with seeds up to two ulp off, 0 of 2.0e9 uniformly random pairs,
and 0 over all 2^24 numerators under each of 40 other denominators (the sixteen mantissas below all ones among them), three seeds each."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CXX = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
SUMMARY = re.compile(r"pairs checked (\d+), mismatches with the seed at RN (\d+), one ulp below (\d+), one ulp above (\d+), zero sign errors (\d+), "
                     r"guard cases (\d+), guard errors (\d+)")


def run_program(tmp_path, sanitize, pairs):
    assert CXX is not None, "no host C++ compiler (c++, g++, clang++): the division's host check cannot run"
    exe = tmp_path / "shared_division"
    flags = ["-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + (["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else [])
    subprocess.run([CXX, *flags, "-I", str(ROOT / "amber_amd" / "csrc" / "hip"), "-o", str(exe), str(ROOT / "tests" / "shared_division_main.cc")],
                   check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([str(exe), str(pairs)], capture_output=True, text=True, timeout=600)
    print("\n" + r.stdout + r.stderr)
    m = SUMMARY.search(r.stdout)
    assert m, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    keys = ("pairs", "rn", "below", "above", "zero_sign", "guard_cases", "guard_errors")
    return dict(zip(keys, (int(g) for g in m.groups())))


@pytest.fixture(scope="module")
def full_run(tmp_path_factory):
    return run_program(tmp_path_factory.mktemp("shared_division"), False, 100_000_000)


def test_quotients_equal_the_division_with_the_seed_at_the_nearest_float(full_run):
    assert full_run["pairs"] >= 100_000_000 and full_run["rn"] == 0, full_run


def test_quotients_equal_the_division_with_the_seed_one_ulp_off(full_run):
    assert full_run["pairs"] >= 100_000_000 and full_run["below"] == 0 and full_run["above"] == 0, full_run


def test_zero_numerators_keep_the_ieee_sign(full_run):
    assert full_run["zero_sign"] == 0, full_run


def test_the_guards_accept_the_range_and_nothing_else(full_run):
    assert full_run["guard_cases"] > 20_000_000 and full_run["guard_errors"] == 0, full_run


def test_the_program_is_clean_under_asan_and_ubsan(tmp_path):
    got = run_program(tmp_path, True, 10_000_000)
    assert got["pairs"] >= 10_000_000 and got["rn"] == 0 and got["zero_sign"] == 0 and got["guard_errors"] == 0, got
