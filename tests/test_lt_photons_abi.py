"""amber_hip_lt_trace_photons, the part that needs no GPU: the layout of AmberPhoton and AmberPhotonInfo in the binding and in the header, the
constants, the export lists of both libraries, the declaration in include/amber_hip.h, and the ABI version, which stays 3."""
import ctypes
import json
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "amber_hip.h").read_text()


def test_struct_layouts(amber):
    assert ctypes.sizeof(amber.Photon) == 64 and amber.PHOTON_DTYPE.itemsize == 64 and ctypes.sizeof(amber.PhotonInfo) == 32
    offsets = (("pos", 0), ("object", 12), ("dir_out", 16), ("path", 28), ("weight", 32), ("sample", 44), ("normal", 48), ("bounce", 60))
    for name, off in offsets:
        assert getattr(amber.Photon, name).offset == off == amber.PHOTON_DTYPE.fields[name][1], name
    assert [n for n, _ in amber.Photon._fields_] == [n for n, _ in offsets] == list(amber.PHOTON_DTYPE.names)
    for name, off in (("n_photons", 0), ("n_written", 8), ("n_rays", 16), ("n_launches", 24), ("n_repeats", 28)):
        assert getattr(amber.PhotonInfo, name).offset == off, name
    import photon_reference
    assert photon_reference.PHOTON == amber.PHOTON_DTYPE


def test_the_header_declares_what_the_binding_states(amber):
    flat = " ".join(HEADER.split())
    assert ("typedef struct { float pos[3]; int32_t object; float dir_out[3]; uint32_t path; float weight[3]; uint32_t sample; float normal[3]; uint32_t bounce; } AmberPhoton;"
            in flat)
    assert "typedef struct { uint64_t n_photons, n_written, n_rays; uint32_t n_launches, n_repeats; } AmberPhotonInfo;" in flat
    assert re.search(r"int amber_hip_lt_trace_photons\(amber_hip_pt\*, uint32_t first_sample, uint32_t n_samples, uint32_t path_begin, uint32_t path_end, "
                     r"uint32_t surfaces, AmberPhoton\* out, uint64_t capacity, AmberPhotonInfo\* info /\* may be NULL \*/, uint32_t flags\);", flat)
    values = {m.group(1): int(m.group(2)) for m in re.finditer(r"AMBER_(PHOTONS?_[A-Z]+) = (\d+)u", HEADER)}
    assert values == {"PHOTON_DIFFUSE": 1, "PHOTON_SPECULAR": 2, "PHOTON_LIGHT": 4, "PHOTON_EYE": 8, "PHOTON_ALL": 15, "PHOTONS_HOST": 1}
    assert (amber.PHOTON_DIFFUSE, amber.PHOTON_SPECULAR, amber.PHOTON_LIGHT, amber.PHOTON_EYE, amber.PHOTON_ALL, amber.PHOTONS_HOST) == (1, 2, 4, 8, 15, 1)
    assert re.search(r"#define AMBER_PHOTON_CAPACITY0 65536u", HEADER) and amber.PHOTON_CAPACITY0 == 65536
    assert re.search(r"#define AMBER_HIP_ABI_VERSION 3\b", HEADER)


def test_symbol_is_product_abi_in_both_libraries(amber):
    from amber_amd.api import ABI_SYMBOLS, LAB_LIB, LAB_SYMBOLS, PRODUCT_LIB
    assert "amber_hip_lt_trace_photons" in ABI_SYMBOLS and "amber_hip_lt_trace_photons" not in LAB_SYMBOLS
    assert "amber_hip_kat_photon_stage_ms" in LAB_SYMBOLS and "amber_hip_kat_photon_stage_ms" not in ABI_SYMBOLS
    assert amber.load_library().amber_hip_abi_version() == 3
    lib_dir = amber.library_path().parent
    code = ("import ctypes, json, sys; lib = ctypes.CDLL(sys.argv[1]); "
            "print(json.dumps([hasattr(lib, 'amber_hip_lt_trace_photons'), hasattr(lib, 'amber_hip_kat_photon_stage_ms'), lib.amber_hip_abi_version()]))")
    for name, want in ((PRODUCT_LIB, [True, False, 3]), (LAB_LIB, [True, True, 3])):
        out = subprocess.run([sys.executable, "-c", code, str(lib_dir / name)], capture_output=True, text=True, check=True).stdout
        assert json.loads(out) == want, name
