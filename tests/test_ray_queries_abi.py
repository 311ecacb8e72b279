"""amber_hip_pt_cast_rays / amber_hip_pt_occluded at the ABI level (no GPU): the declarations in include/amber_hip.h, their mirrors in
amber_amd/api.py, the exported symbols."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np

import amber_amd as A
from amber_amd import api

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "amber_hip.h").read_text()
SYMBOLS = ("amber_hip_pt_cast_rays", "amber_hip_pt_occluded")
CTYPES = {"float": ctypes.c_float, "uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32}


def test_header_declares_both_functions_and_python_lists_them():
    assert re.search(r"int\s+amber_hip_pt_cast_rays\(amber_hip_pt\*,\s*uint64_t n,\s*const AmberRay\* rays,\s*AmberRayHit\* hits,\s*uint32_t flags\);", HEADER)
    assert re.search(r"int\s+amber_hip_pt_occluded\s*\(amber_hip_pt\*,\s*uint64_t n,\s*const AmberRay\* rays,\s*uint8_t\* occluded,\s*uint32_t flags\);", HEADER)
    flag = re.search(r"enum \{ AMBER_RAYS_HOST = (\d+)u \};", HEADER)
    assert flag and int(flag.group(1)) == A.RAYS_HOST == 1
    for name in SYMBOLS:
        assert name in api.ABI_SYMBOLS and name not in api.LAB_SYMBOLS


def _header_fields(struct):
    """[(name, ctype)] of a one-line struct of the header; `float origin[3]` becomes an array type"""
    body = re.search(r"typedef struct \{([^}]*)\} " + struct + ";", HEADER).group(1)
    fields = []
    for stmt in body.split(";"):
        words = stmt.split()
        if words:
            m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", words[1])
            fields.append((m.group(1), CTYPES[words[0]] * int(m.group(2)) if m.group(2) else CTYPES[words[0]]))
    return fields


def test_the_two_structs_have_the_headers_layout():
    for struct, mirror, record in (("AmberRay", api.Ray, api._RAY), ("AmberRayHit", api.RayHit, api._RAY_HIT)):
        fields = _header_fields(struct)
        assert [n for n, _ in fields] == [n for n, _ in mirror._fields_], struct
        offset = 0
        for (name, ctype), (_, mtype) in zip(fields, mirror._fields_):     # every member is 4-byte aligned: the C compiler packs them back to back
            assert ctypes.sizeof(ctype) == ctypes.sizeof(mtype) and ctype._type_ == mtype._type_, (struct, name)   # element type (arrays) / type code (scalars)
            assert getattr(ctype, "_length_", 0) == getattr(mtype, "_length_", 0), (struct, name)
            assert getattr(mirror, name).offset == offset == record.fields[name][1], (struct, name)
            offset += ctypes.sizeof(ctype)
        assert ctypes.sizeof(mirror) == offset == record.itemsize == 32, struct
    assert api.Ray.t_max.offset == 12 and api.Ray.dir.offset == 16                     # origin.w of the first float4 is t_max
    assert api.RayHit.object.offset == 4 and api.RayHit.pos.offset == 8 and api.RayHit.normal.offset == 20
    assert api._RAY_HIT["object"] == np.int32


def test_both_libraries_export_both_symbols():
    lib_dir = ROOT / "amber_amd" / "lib"
    for name in (api.PRODUCT_LIB, api.LAB_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", str(lib_dir / name)], capture_output=True, text=True, check=True).stdout
        for sym in SYMBOLS:
            assert re.search(r" T " + sym + "$", out, re.M), (name, sym)


def test_abi_version_is_still_three():
    assert re.search(r"#define AMBER_HIP_ABI_VERSION 3\b", HEADER)
    for name in (api.PRODUCT_LIB, api.LAB_LIB):
        lib = ctypes.CDLL(str(ROOT / "amber_amd" / "lib" / name))
        assert lib.amber_hip_abi_version() == 3, name
