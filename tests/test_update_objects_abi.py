"""amber_hip_pt_update_objects at the ABI level (no GPU): the declaration in include/amber_hip.h, its mirror in amber_amd/api.py, the exported symbol."""
import ctypes
import re
import subprocess
from pathlib import Path

import amber_amd as A
from amber_amd import api

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "amber_hip.h").read_text()


def test_header_declares_the_entry_point_and_python_mirrors_it():
    decl = re.search(r"int\s+amber_hip_pt_update_objects\(amber_hip_pt\*,\s*uint32_t first,\s*uint32_t count,\s*const AmberFlatObject\* objects,\s*uint32_t mode,\s*AmberUpdateInfo\* info", HEADER)
    assert decl, "amber_hip.h does not declare amber_hip_pt_update_objects as the issue gives it"
    enum = re.search(r"enum \{ AMBER_UPDATE_REFIT = (\d+), AMBER_UPDATE_REBUILD = (\d+) \};", HEADER)
    assert enum and (int(enum.group(1)), int(enum.group(2))) == (A.UPDATE_REFIT, A.UPDATE_REBUILD) == (0, 1)
    assert "amber_hip_pt_update_objects" in api.ABI_SYMBOLS and "amber_hip_pt_update_objects" not in api.LAB_SYMBOLS


def test_update_info_has_the_headers_layout():
    body = re.search(r"typedef struct \{([^}]*)\} AmberUpdateInfo;", HEADER).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    sizes = {"uint32_t": (4, ctypes.c_uint32), "float": (4, ctypes.c_float), "double": (8, ctypes.c_double)}
    fields = []
    for stmt in body.split(";"):
        words = stmt.replace(",", " ").split()
        if words:
            fields += [(name, sizes[words[0]][1]) for name in words[1:]]
    assert [(n, t) for n, t in fields] == [(n, t) for n, t in api.UpdateInfo._fields_]
    offset = 0
    for name, ctype in fields:                                            # natural alignment, as the C compiler lays the struct out
        size = ctypes.sizeof(ctype)
        offset = (offset + size - 1) // size * size
        assert getattr(api.UpdateInfo, name).offset == offset, name
        offset += size
    assert ctypes.sizeof(api.UpdateInfo) == (offset + 7) // 8 * 8 == 32


def test_abi_version_and_build_info_are_what_they_were():
    assert re.search(r"#define AMBER_HIP_ABI_VERSION 3\b", HEADER)
    assert ctypes.sizeof(api.BuildInfo) == 40


def test_both_libraries_export_the_symbol():
    lib_dir = ROOT / "amber_amd" / "lib"
    for name in (api.PRODUCT_LIB, api.LAB_LIB):
        out = subprocess.run(["nm", "-D", "--defined-only", str(lib_dir / name)], capture_output=True, text=True, check=True).stdout
        assert re.search(r" T amber_hip_pt_update_objects$", out, re.M), name
