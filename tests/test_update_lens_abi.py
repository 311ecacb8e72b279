"""amber_hip_pt_update_lens at the ABI level (no GPU): the declaration in include/amber_hip.h, its mirror in amber_amd/api.py, the exported symbol,
and the host-only lens derivation (scene_prep.h) under AddressSanitizer + UBSan: the same bytes through create's path and through the update's."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

import amber_amd as A
from amber_amd import api

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "amber_hip.h").read_text()


def test_header_declares_the_entry_point_and_python_mirrors_it():
    decl = re.search(r"int\s+amber_hip_pt_update_lens\(amber_hip_pt\*,\s*const AmberFlatThinLens\* lens,\s*const AmberFlatObject\* blades\s*,\s*uint32_t mode\s*,\s*"
                     r"AmberUpdateInfo\* info\s*\);", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    assert decl, "amber_hip.h does not declare amber_hip_pt_update_lens as the issue gives it"
    assert "amber_hip_pt_update_lens" in api.ABI_SYMBOLS and "amber_hip_pt_update_lens" not in api.LAB_SYMBOLS
    assert callable(getattr(A.PathTracer, "update_lens", None))
    assert (A.UPDATE_REFIT, A.UPDATE_REBUILD) == (0, 1)


def test_abi_version_is_still_3():
    assert re.search(r"#define AMBER_HIP_ABI_VERSION 3\b", HEADER)


def test_both_libraries_export_the_symbol():
    lib_dir = ROOT / "amber_amd" / "lib"
    for name in (api.PRODUCT_LIB, api.LAB_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", str(lib_dir / name)], capture_output=True, text=True, check=True).stdout
        assert re.search(r" T amber_hip_pt_update_lens$", out, re.M), name


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_lens_derivation_is_the_same_through_create_and_update_under_asan_ubsan(tmp_path):
    """tests/lens_sanitize.hip: DevLens and DevBlade[] byte for byte, a thin lens and a pinhole, engine BVH asked for and chosen by AUTO."""
    exe = tmp_path / "lens_sanitize"
    # the scenes come from the host object model through the product library's C interface; the derivation itself is header code and instrumented
    # -fno-gpu-sanitize: the sanitizers instrument the host code only, never a device code object
    cmd = ["hipcc", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-gpu-sanitize", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-o", str(exe), str(ROOT / "tests" / "lens_sanitize.hip"),
           "-L" + str(ROOT / "amber_amd" / "lib"), "-lamber_hip", "-Wl,-rpath," + str(ROOT / "amber_amd" / "lib")]
    subprocess.run(["make", "-C", str(ROOT / "amber_amd" / "csrc")], check=True, capture_output=True)
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env={"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0", "PATH": "/usr/bin:/bin", "LD_LIBRARY_PATH": "/opt/rocm/lib"})
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("identical through create and update") == 5
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
