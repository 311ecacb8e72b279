"""amber_hip_pt_temporal and its three companions at the ABI level (no GPU): the declarations and the two 32-byte structs in include/amber_hip.h, their
mirror in amber_amd/api.py, the exported symbols and the defaults of PathTracer.temporal."""
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
NAMES = ["amber_hip_pt_temporal", "amber_hip_pt_temporal_reset", "amber_hip_pt_history_download", "amber_hip_pt_device_history"]


def test_header_declares_the_entry_points():
    assert re.search(r"int\s+amber_hip_pt_temporal\(amber_hip_pt\*,\s*uint32_t n_samples,\s*const AmberTemporalParams\* params,\s*uint32_t format,\s*void\* out,"
                     r"\s*uint64_t out_bytes,\s*uint32_t flags\s*\);", CODE)
    assert re.search(r"int\s+amber_hip_pt_temporal_reset\(amber_hip_pt\*\);", CODE)
    assert re.search(r"int\s+amber_hip_pt_history_download\(amber_hip_pt\*,\s*AmberHistoryPixel\* out\);", CODE)
    assert re.search(r"int\s+amber_hip_pt_device_history\(amber_hip_pt\*,\s*void\*\* dptr,\s*uint64_t\* n_pixels\);", CODE)


def test_the_structs_are_32_bytes_in_the_given_order():
    assert re.search(r"typedef struct \{\s*uint32_t levels;\s*uint32_t max_history;\s*float k_normal, k_albedo, k_depth, k_color;\s*uint32_t reserved\[2\];\s*\} AmberTemporalParams;", CODE)
    assert re.search(r"typedef struct \{\s*float color\[3\];\s*float length;\s*float m1, m2;\s*float pad\[2\];\s*\} AmberHistoryPixel;", CODE)
    P = api.TemporalParams
    assert ctypes.sizeof(P) == 32 and A.TemporalParams is P
    assert [(n, ctypes.sizeof(t)) for n, t in P._fields_] == [("levels", 4), ("max_history", 4), ("k_normal", 4), ("k_albedo", 4), ("k_depth", 4), ("k_color", 4), ("reserved", 8)]
    assert [getattr(P, n).offset for n, _ in P._fields_] == [0, 4, 8, 12, 16, 20, 24]
    assert [t for _, t in P._fields_[:6]] == [ctypes.c_uint32] * 2 + [ctypes.c_float] * 4
    Hp = api.HistoryPixel
    assert ctypes.sizeof(Hp) == 32 and A.HistoryPixel is Hp
    assert [(n, getattr(Hp, n).offset, ctypes.sizeof(t)) for n, t in Hp._fields_] == [("color", 0, 12), ("length", 12, 4), ("m1", 16, 4), ("m2", 20, 4), ("pad", 24, 8)]


def test_python_mirrors_them():
    for name in NAMES:
        assert name in api.ABI_SYMBOLS and name not in api.LAB_SYMBOLS
    for method in ("temporal", "temporal_reset", "history_download", "device_history"):
        assert callable(getattr(A.PathTracer, method, None)), method
    sig = inspect.signature(A.PathTracer.temporal)
    assert list(sig.parameters) == ["self", "n_samples", "levels", "max_history", "k_normal", "k_albedo", "k_depth", "k_color", "format", "mirror", "out"]
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(levels=5, max_history=32, k_normal=4.0, k_albedo=100.0, k_depth=10.0, k_color=0.25, format=A.RESOLVE_RGB8, mirror=False, out=None)


def test_the_denoise_contracts_point_to_the_new_call():
    for call in ("amber_hip_pt_denoise", "amber_hip_pt_denoise_variance"):
        contract = HEADER[:HEADER.index("int  " + call + "(")]
        assert "amber_hip_pt_temporal" in contract[contract.rindex("Not part of it"):], call


def test_abi_version_is_still_3():
    assert re.search(r"#define AMBER_HIP_ABI_VERSION 3\b", HEADER)


def test_both_libraries_export_the_symbols_and_the_product_nothing_else(amber):
    lib_dir = ROOT / "amber_amd" / "lib"
    for lib in (api.PRODUCT_LIB, api.LAB_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", str(lib_dir / lib)], capture_output=True, text=True, check=True).stdout
        for name in NAMES:
            assert re.search(r" T " + name + r"$", out, re.M), (lib, name)
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib_dir / api.PRODUCT_LIB)], capture_output=True, text=True, check=True).stdout
    exported = sorted(m.group(1) for m in re.finditer(r" T (amber_\w+)$", out, re.M))
    assert exported == sorted(api.ABI_SYMBOLS)                                 # the product's export list is still exactly ABI_SYMBOLS
