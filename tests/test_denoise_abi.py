"""amber_hip_pt_denoise at the ABI level (no GPU): the declaration and the 32-byte struct in include/amber_hip.h, their mirror in amber_amd/api.py, the
exported symbol and the defaults of PathTracer.denoise."""
import ctypes
import inspect
import re
import subprocess
from pathlib import Path

import amber_amd as A
from amber_amd import api

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "amber_hip.h").read_text()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
NAME = "amber_hip_pt_denoise"


def test_header_declares_the_entry_point():
    decl = re.search(r"int\s+amber_hip_pt_denoise\(amber_hip_pt\*,\s*uint32_t n_samples,\s*const AmberDenoiseParams\* params,\s*uint32_t format,\s*void\* out,"
                     r"\s*uint64_t out_bytes,\s*uint32_t flags\s*\);", CODE)
    assert decl, "amber_hip.h does not declare amber_hip_pt_denoise as the issue gives it"


def test_the_struct_is_32_bytes_in_the_given_order():
    assert re.search(r"typedef struct \{\s*uint32_t levels;\s*float k_normal;\s*float k_albedo;\s*float k_depth;\s*float k_color;\s*uint32_t reserved\[3\];\s*\} AmberDenoiseParams;", CODE)
    P = api.DenoiseParams
    assert ctypes.sizeof(P) == 32 and A.DenoiseParams is P
    assert [(n, ctypes.sizeof(t)) for n, t in P._fields_] == [("levels", 4), ("k_normal", 4), ("k_albedo", 4), ("k_depth", 4), ("k_color", 4), ("reserved", 12)]
    assert (P.levels.offset, P.k_normal.offset, P.k_albedo.offset, P.k_depth.offset, P.k_color.offset, P.reserved.offset) == (0, 4, 8, 12, 16, 20)
    assert [t for _, t in P._fields_[:5]] == [ctypes.c_uint32] + [ctypes.c_float] * 4


def test_python_mirrors_it():
    assert NAME in api.ABI_SYMBOLS and NAME not in api.LAB_SYMBOLS
    assert callable(getattr(A.PathTracer, "denoise", None))
    sig = inspect.signature(A.PathTracer.denoise)
    assert list(sig.parameters) == ["self", "n_samples", "levels", "k_normal", "k_albedo", "k_depth", "k_color", "format", "mirror", "out"]
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(levels=5, k_normal=4.0, k_albedo=100.0, k_depth=10.0, k_color=0.25, format=A.RESOLVE_RGB8, mirror=False, out=None)


def test_abi_version_is_still_3():
    assert re.search(r"#define AMBER_HIP_ABI_VERSION 3\b", HEADER)


def test_both_libraries_export_the_symbol(amber):
    lib_dir = ROOT / "amber_amd" / "lib"
    for name in (api.PRODUCT_LIB, api.LAB_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", str(lib_dir / name)], capture_output=True, text=True, check=True).stdout
        assert re.search(r" T " + NAME + r"$", out, re.M), name
