"""amber_hip_pm_build / amber_hip_pm_gather / amber_hip_pm_release, the part that needs no GPU: the layout of the three structs in the binding, in the
restatement and as a C compiler lays the header out, the declarations, the flag, the export lists of both libraries, and the ABI version, which stays 3."""
import ctypes
import json
import re
import shutil
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "amber_hip.h").read_text()
LAB_HEADER = (ROOT / "include" / "amber_hip_lab.h").read_text()
QUERY_OFFSETS = (("pos", 0), ("radius", 12), ("normal", 16), ("object", 28), ("dir_out", 32), ("pad0", 44), ("weight", 48), ("pad1", 60))
RESULT_OFFSETS = (("rgb", 0), ("n_used", 12), ("r2_used", 16), ("n_in_radius", 20), ("pad", 24))
INFO_OFFSETS = (("n_photons", 0), ("n_dropped", 8), ("dims", 16), ("n_doublings", 28), ("cell_size", 32), ("lo", 36), ("hi", 48), ("max_cell_count", 60), ("build_ms", 64))


def test_struct_layouts(amber):
    import photon_map_reference as R
    assert amber.GATHER_QUERY_DTYPE.itemsize == 64 and amber.GATHER_RESULT_DTYPE.itemsize == 32 and ctypes.sizeof(amber.PhotonMapInfo) == 72
    for dtype, offsets in ((amber.GATHER_QUERY_DTYPE, QUERY_OFFSETS), (amber.GATHER_RESULT_DTYPE, RESULT_OFFSETS)):
        assert list(dtype.names) == [n for n, _ in offsets]
        for name, off in offsets:
            assert dtype.fields[name][1] == off, name
    assert [n for n, _ in amber.PhotonMapInfo._fields_] == [n for n, _ in INFO_OFFSETS]
    for name, off in INFO_OFFSETS:
        assert getattr(amber.PhotonMapInfo, name).offset == off, name
    assert R.QUERY == amber.GATHER_QUERY_DTYPE and R.RESULT == amber.GATHER_RESULT_DTYPE
    assert amber.PM_RAW_SUM == 2 and amber.api.RAYS_HOST == 1


def test_the_header_declares_what_the_binding_states():
    flat = " ".join(HEADER.split())
    assert ("typedef struct { float pos[3]; float radius; float normal[3]; int32_t object; float dir_out[3]; uint32_t pad0; float weight[3]; uint32_t pad1; } AmberGatherQuery;"
            in flat)
    assert "typedef struct { float rgb[3]; uint32_t n_used; float r2_used; uint32_t n_in_radius; uint32_t pad[2]; } AmberGatherResult;" in flat
    assert ("typedef struct { uint64_t n_photons, n_dropped; uint32_t dims[3]; uint32_t n_doublings; float cell_size; float lo[3]; float hi[3]; uint32_t max_cell_count; "
            "double build_ms; } AmberPhotonMapInfo;" in flat)
    assert "enum { AMBER_PM_RAW_SUM = 2u };" in flat
    assert re.search(r"int amber_hip_pm_build\(amber_hip_pt\*, const AmberPhoton\* photons, uint64_t n, float cell_size, uint32_t flags /\* AMBER_PHOTONS_HOST \*/, "
                     r"AmberPhotonMapInfo\* info /\* may be NULL \*/\);", flat)
    assert re.search(r"int amber_hip_pm_gather\(amber_hip_pt\*, uint64_t n, const AmberGatherQuery\* q, AmberGatherResult\* out, uint32_t k /\* 0: no cap \*/, "
                     r"uint32_t flags /\* AMBER_RAYS_HOST \| AMBER_PM_RAW_SUM \*/\);", flat)
    assert "int amber_hip_pm_release(amber_hip_pt*);" in flat
    assert re.search(r"#define AMBER_HIP_ABI_VERSION 3\b", HEADER)
    lab = " ".join(LAB_HEADER.split())
    assert "int amber_hip_kat_pm_stage_ms(amber_hip_pt*, double* build_ms, double* gather_ms);" in lab
    assert ("int amber_hip_kat_bsdf(amber_hip_pt*, uint32_t n, const int32_t* object, const float* normal, const float* dir_out, const float* dir_in, float* rgb_out);"
            in lab)


def test_the_header_compiles_as_c_with_these_layouts(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    lines = ['#include <stddef.h>', '#include "amber_hip.h"', '#include "amber_hip_lab.h"',
             "_Static_assert(sizeof(AmberGatherQuery) == 64 && sizeof(AmberGatherResult) == 32 && sizeof(AmberPhotonMapInfo) == 72, \"sizes\");"]
    for struct, offsets in (("AmberGatherQuery", QUERY_OFFSETS), ("AmberGatherResult", RESULT_OFFSETS), ("AmberPhotonMapInfo", INFO_OFFSETS)):
        lines += [f'_Static_assert(offsetof({struct}, {name}) == {off}, "{struct}.{name}");' for name, off in offsets]
    lines += ["int (*build)(amber_hip_pt*, const AmberPhoton*, uint64_t, float, uint32_t, AmberPhotonMapInfo*) = amber_hip_pm_build;",
              "int (*gather)(amber_hip_pt*, uint64_t, const AmberGatherQuery*, AmberGatherResult*, uint32_t, uint32_t) = amber_hip_pm_gather;",
              "int (*release)(amber_hip_pt*) = amber_hip_pm_release;",
              "int flags = AMBER_RAYS_HOST | AMBER_PM_RAW_SUM | AMBER_PHOTONS_HOST;"]
    src = tmp_path / "pm_abi.c"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_symbols_are_product_abi_in_both_libraries(amber):
    from amber_amd.api import ABI_SYMBOLS, LAB_LIB, LAB_SYMBOLS, PRODUCT_LIB
    names = ["amber_hip_pm_build", "amber_hip_pm_gather", "amber_hip_pm_release"]
    lab_names = ["amber_hip_kat_pm_stage_ms", "amber_hip_kat_bsdf"]
    assert all(n in ABI_SYMBOLS and n not in LAB_SYMBOLS for n in names) and all(n in LAB_SYMBOLS and n not in ABI_SYMBOLS for n in lab_names)
    assert all(hasattr(amber.PathTracer, n) for n in ("pm_build", "pm_gather", "pm_release", "kat_pm_stage_ms", "kat_bsdf"))
    lib_dir = amber.library_path().parent
    code = "import ctypes, json, sys; lib = ctypes.CDLL(sys.argv[1]); print(json.dumps([[hasattr(lib, n) for n in sys.argv[2:]], lib.amber_hip_abi_version()]))"
    for name, want in ((PRODUCT_LIB, [[True] * 3 + [False] * 2, 3]), (LAB_LIB, [[True] * 5, 3])):
        out = subprocess.run([sys.executable, "-c", code, str(lib_dir / name)] + names + lab_names, capture_output=True, text=True, check=True).stdout
        assert json.loads(out) == want, name
