"""The square root of the render kernels from one reciprocal-square-root seed (amber_amd/csrc/hip/exact_sqrt.h) against sqrtf on the host (no GPU needed).

A stand-alone program (tests/exact_sqrt_main.cc: its own main, the host compiler, -ffp-contract=off, nothing of the library, nothing loaded into
python) includes the header and runs the host restatement -- the seed is a parameter there, v_rsq_f32 on the device:
  * roots: ExactSqrt(x, seed) against sqrtf(x), which the host rounds correctly, with the seed at the float nearest to 1 / sqrt(x) and at every
    offset from -3 to +3 ulp of it: ALL 2^24 operands of [1, 2) and [2, 4) (both exponent parities), all 2^23 mantissas of the lowest binade
    of the guard's range (2^-60) and of the highest (2^59), and every 251st mantissa plus the extreme ones of each of the 120 binades;
  * the guards (ExactSqrtSafe, ExactSqrtSafe2, ExactNormalizeSafe) against the range said in float compares: one ulp inside and outside each
    bound, +-0, subnormals, negatives, inf, NaN, and 2.4e7 groups of random bit patterns;
  * Normalize: 1.0e8 vectors of magnitudes 2^-15 ... 2^15 (exact zeros and components next to zero among them), a third of them normalised
    beforehand; the length is ExactSqrt's (seed offsets -3 ... +3 in turn), the reciprocal of shared_div.h starts from h + h moved by every
    offset from -3 to +3 ulp, and the three quotients must equal `/`.
Built twice: -O2 (everything), and -O2 with AddressSanitizer + UBSan (a tenth: every tenth mantissa, 1.0e7 vectors), run directly.

Figures of this program, one run (they do not depend on the machine):
  roots checked 262961384, root mismatches 0, guard cases 124022169, guard errors 0, vectors checked 100000000, all-ones lengths 8576975,
  quotient mismatches 0, h + h from RN(1 / l) in ulp: lowest -2, highest 2
  vectors with h + h at -2, -1, 0, +1, +2 ulp of RN(1 / l): 73881, 23487225, 66506169, 9859253, 73472; none further."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CXX = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
SUMMARY = re.compile(r"roots checked (\d+), root mismatches (\d+), guard cases (\d+), guard errors (\d+), vectors checked (\d+), all-ones lengths (\d+), "
                     r"quotient mismatches (\d+), h \+ h from RN\(1 / l\) in ulp: lowest (-?\d+), highest (-?\d+)")
EXHAUSTIVE_ROOTS = 7 * 4 * (1 << 23)            # seven seeds, four whole binades


def run_program(tmp_path, sanitize, vectors, stride):
    assert CXX is not None, "no host C++ compiler (c++, g++, clang++): the square root's host check cannot run"
    exe = tmp_path / "exact_sqrt"
    flags = ["-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + (["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else [])
    subprocess.run([CXX, *flags, "-I", str(ROOT / "amber_amd" / "csrc" / "hip"), "-o", str(exe), str(ROOT / "tests" / "exact_sqrt_main.cc")],
                   check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([str(exe), str(vectors), str(stride)], capture_output=True, text=True, timeout=600)
    print("\n" + r.stdout + r.stderr)
    m = SUMMARY.search(r.stdout)
    assert m, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    keys = ("roots", "root_mismatches", "guard_cases", "guard_errors", "vectors", "all_ones", "quotient_mismatches", "seed_low", "seed_high")
    got = dict(zip(keys, (int(g) for g in m.groups())))
    got["exit"] = r.returncode
    return got


@pytest.fixture(scope="module")
def full_run(tmp_path_factory):
    return run_program(tmp_path_factory.mktemp("exact_sqrt"), False, 100_000_000, 1)


def test_roots_equal_sqrtf_with_the_seed_up_to_three_ulp_off(full_run):
    """All 2^24 operands of two adjacent binades, all mantissas of the range's first and last binade, strided ones between: seven seeds each."""
    assert full_run["roots"] > EXHAUSTIVE_ROOTS and full_run["root_mismatches"] == 0, full_run


def test_the_guards_accept_the_range_and_nothing_else(full_run):
    assert full_run["guard_cases"] > 24_000_000 and full_run["guard_errors"] == 0, full_run


def test_normalize_from_the_root_s_seed_equals_the_divisions(full_run):
    """1e8 vectors; the reciprocal seeded with h + h and with every offset to +-3 ulp of it; lengths with an all-ones mantissa well represented."""
    assert full_run["vectors"] >= 100_000_000 and full_run["quotient_mismatches"] == 0 and full_run["exit"] == 0, full_run
    assert full_run["all_ones"] >= full_run["vectors"] // 20, full_run


def test_the_root_s_half_reciprocal_is_within_two_ulp_of_the_reciprocal(full_run):
    """h + h against RN(1 / l): the offsets the program applies on top of it (+-3) leave a margin of one ulp beyond what v_rsq_f32 may add."""
    assert -2 <= full_run["seed_low"] and full_run["seed_high"] <= 2, full_run


def test_the_program_is_clean_under_asan_and_ubsan(tmp_path):
    got = run_program(tmp_path, True, 10_000_000, 10)
    assert got["roots"] > EXHAUSTIVE_ROOTS // 10 and got["vectors"] >= 10_000_000, got
    assert got["root_mismatches"] == 0 and got["guard_errors"] == 0 and got["quotient_mismatches"] == 0 and got["exit"] == 0, got
