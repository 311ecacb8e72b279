"""amber_hip_pt_resolve at the ABI level (no GPU): the declaration in include/amber_hip.h, its mirror in amber_amd/api.py and the exported symbol."""
import re
import subprocess
from pathlib import Path

import amber_amd as A
from amber_amd import api

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "amber_hip.h").read_text()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)


def test_header_declares_the_entry_point_and_python_mirrors_it():
    decl = re.search(r"int\s+amber_hip_pt_resolve\(amber_hip_pt\*,\s*uint32_t n_samples,\s*uint32_t format,\s*void\* out,\s*uint64_t out_bytes,\s*uint32_t flags\s*\);", CODE)
    assert decl, "amber_hip.h does not declare amber_hip_pt_resolve as the issue gives it"
    assert "amber_hip_pt_resolve" in api.ABI_SYMBOLS and "amber_hip_pt_resolve" not in api.LAB_SYMBOLS
    assert callable(getattr(A.PathTracer, "resolve", None))


def test_constants_have_the_header_values():
    assert re.search(r"enum\s*\{\s*AMBER_RESOLVE_MEAN_F32\s*=\s*0,\s*AMBER_RESOLVE_RGB8\s*=\s*1,\s*AMBER_RESOLVE_RGBA8\s*=\s*2\s*\}", CODE)
    assert re.search(r"enum\s*\{\s*AMBER_RESOLVE_HOST\s*=\s*1u,\s*AMBER_RESOLVE_MIRROR_X\s*=\s*2u\s*\}", CODE)
    assert (A.RESOLVE_MEAN_F32, A.RESOLVE_RGB8, A.RESOLVE_RGBA8) == (0, 1, 2)
    assert (A.RESOLVE_HOST, A.RESOLVE_MIRROR_X) == (1, 2)
    assert (api.RESOLVE_MEAN_F32, api.RESOLVE_RGB8, api.RESOLVE_RGBA8, api.RESOLVE_HOST, api.RESOLVE_MIRROR_X) == (0, 1, 2, 1, 2)


def test_abi_version_is_still_3():
    assert re.search(r"#define AMBER_HIP_ABI_VERSION 3\b", HEADER)


def test_both_libraries_export_the_symbol(amber):
    lib_dir = ROOT / "amber_amd" / "lib"
    for name in (api.PRODUCT_LIB, api.LAB_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", str(lib_dir / name)], capture_output=True, text=True, check=True).stdout
        assert re.search(r" T amber_hip_pt_resolve$", out, re.M), name
