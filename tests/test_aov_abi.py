"""The first-hit AOV entry points at the ABI level (no GPU): their declarations and the 32-byte struct in include/amber_hip.h, the mirror in
amber_amd/api.py and the exported symbols."""
import ctypes
import re
import subprocess
from pathlib import Path

import amber_amd as A
from amber_amd import api

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "amber_hip.h").read_text()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
NAMES = ("amber_hip_pt_aov_pass", "amber_hip_pt_aov_clear", "amber_hip_pt_aov_download", "amber_hip_pt_device_aov")


def test_header_declares_the_four_functions():
    for decl in (r"int\s+amber_hip_pt_aov_pass\(amber_hip_pt\*,\s*uint32_t first_sample,\s*uint32_t n_samples\s*\);",
                 r"int\s+amber_hip_pt_aov_clear\(amber_hip_pt\*\s*\);",
                 r"int\s+amber_hip_pt_aov_download\(amber_hip_pt\*,\s*AmberAovPixel\* out\s*\);",
                 r"int\s+amber_hip_pt_device_aov\(amber_hip_pt\*,\s*void\*\* dptr,\s*uint64_t\* n_pixels\s*\);"):
        assert re.search(decl, CODE), "amber_hip.h does not declare " + decl


def test_the_struct_is_32_bytes_in_the_given_order():
    assert re.search(r"typedef struct \{\s*float albedo\[3\];\s*float depth;\s*float normal\[3\];\s*float coverage;\s*\} AmberAovPixel;", CODE)
    assert ctypes.sizeof(api.AovPixel) == 32 and A.AovPixel is api.AovPixel
    assert [(n, ctypes.sizeof(t)) for n, t in api.AovPixel._fields_] == [("albedo", 12), ("depth", 4), ("normal", 12), ("coverage", 4)]
    assert (api.AovPixel.albedo.offset, api.AovPixel.depth.offset, api.AovPixel.normal.offset, api.AovPixel.coverage.offset) == (0, 12, 16, 28)


def test_python_mirrors_them():
    for name in NAMES:
        assert name in api.ABI_SYMBOLS and name not in api.LAB_SYMBOLS, name
    for method in ("aov_pass", "aov_clear", "aov_download", "device_aov"):
        assert callable(getattr(A.PathTracer, method, None)), method


def test_abi_version_is_still_3():
    assert re.search(r"#define AMBER_HIP_ABI_VERSION 3\b", HEADER)


def test_both_libraries_export_the_symbols(amber):
    lib_dir = ROOT / "amber_amd" / "lib"
    for lib in (api.PRODUCT_LIB, api.LAB_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", str(lib_dir / lib)], capture_output=True, text=True, check=True).stdout
        for name in NAMES:
            assert re.search(r" T " + name + r"$", out, re.M), (lib, name)
