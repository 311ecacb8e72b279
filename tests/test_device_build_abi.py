"""CPU tests of the device-build feature's interface (AMBER_PT_FLAG_DEVICE_BUILD): the new entry points are declared, listed and exported
where they belong -- amber_hip_pt_build_info in the product, amber_hip_kat_bvh_dump in the lab library only -- without a new ABI version, and
the binary64 plane rounding the device builder calls obeys the host builder's inequalities (tests/cpp/plane_word_outward_check.cpp)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "amber_amd" / "lib"


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_build_info_is_part_of_the_product_abi_and_the_dump_of_the_lab_build_only(amber):
    from amber_amd.api import ABI_SYMBOLS, LAB_SYMBOLS
    assert "amber_hip_pt_build_info" in ABI_SYMBOLS and "amber_hip_pt_build_info" not in LAB_SYMBOLS
    assert "amber_hip_kat_bvh_dump" in LAB_SYMBOLS and "amber_hip_kat_bvh_dump" not in ABI_SYMBOLS
    product, lab = _exports(LIB / "libamber_hip.so"), _exports(LIB / "libamber_hip_lab.so")
    assert "amber_hip_pt_build_info" in product and "amber_hip_pt_build_info" in lab
    assert "amber_hip_kat_bvh_dump" in lab and "amber_hip_kat_bvh_dump" not in product
    header, lab_header = (ROOT / "include" / "amber_hip.h").read_text(), (ROOT / "include" / "amber_hip_lab.h").read_text()
    assert re.search(r"int\s+amber_hip_pt_build_info\(amber_hip_pt\*, AmberBuildInfo\* out\);", header)
    assert "amber_hip_kat_bvh_dump" in lab_header and "amber_hip_kat_bvh_dump" not in header
    assert re.search(r"AMBER_PT_FLAG_DEVICE_BUILD = 8u", header)
    for name in ("AMBER_BUILD_NONE", "AMBER_BUILD_HOST", "AMBER_BUILD_DEVICE", "AMBER_BUILD_HOST_FALLBACK"):
        assert name in header


def test_the_abi_version_is_still_3_and_python_mirrors_the_header(amber):
    header = (ROOT / "include" / "amber_hip.h").read_text()
    assert re.search(r"#define AMBER_HIP_ABI_VERSION 3\b", header)
    assert amber.load_library().amber_hip_abi_version() == 3
    assert amber.api.PT_FLAG_DEVICE_BUILD == 8 == amber.PT_FLAG_DEVICE_BUILD
    values = {m.group(1): int(m.group(2)) for m in re.finditer(r"(AMBER_BUILD_[A-Z_]+) = (\d+)", header)}
    assert (values["AMBER_BUILD_NONE"], values["AMBER_BUILD_HOST"], values["AMBER_BUILD_DEVICE"], values["AMBER_BUILD_HOST_FALLBACK"]) == \
        (amber.api.BUILD_NONE, amber.api.BUILD_HOST, amber.api.BUILD_DEVICE, amber.api.BUILD_HOST_FALLBACK)
    assert (values["AMBER_BUILD_REASON_DEPTH"], values["AMBER_BUILD_REASON_WIDE"], values["AMBER_BUILD_REASON_BOUNDS"]) == \
        (amber.api.BUILD_REASON_DEPTH, amber.api.BUILD_REASON_WIDE, amber.api.BUILD_REASON_BOUNDS)
    import ctypes
    assert ctypes.sizeof(amber.api.BuildInfo) == 40                      # six uint32, two doubles (include/amber_hip.h)
    assert ctypes.sizeof(amber.api.BvhDumpInfo) == 52


def test_the_device_builders_kernels_live_in_a_file_of_their_own():
    """The new kernels change no existing instantiation: they are in bvh_device_build.inc, which pt_host.hip includes and the Makefile lists."""
    inc = (ROOT / "amber_amd" / "csrc" / "hip" / "bvh_device_build.inc").read_text()
    assert inc.count("__global__") >= 8
    assert '#include "bvh_device_build.inc"' in (ROOT / "amber_amd" / "csrc" / "hip" / "pt_host.hip").read_text()
    assert "hip/bvh_device_build.inc" in (ROOT / "amber_amd" / "csrc" / "Makefile").read_text()
    # the formulae exist once: the device code calls bvh_build.h's functions
    for fn in ("amber_bvh::ObjectBox(", "amber_bvh::PadBox(", "amber_bvh::PlaneWordOutward(", "amber_bvh::F16AxisGrid("):
        assert fn in inc, fn


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_outward_binary16_planes_in_binary64_obey_the_host_builders_inequalities(tmp_path):
    exe = tmp_path / "plane_word_outward_check"
    src = ROOT / "tests" / "cpp" / "plane_word_outward_check.cpp"
    r = subprocess.run(["hipcc", "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " 0 violations" in r.stdout, r.stdout + r.stderr


def test_the_host_model_and_the_command_line_name_the_option(amber):
    """HipPathTracingOptions.device_build is OR-ed into every handle's flags by amber_host.cc; bin/amber lists --device-build in its usage text."""
    csrc = ROOT / "amber_amd" / "csrc" / "amber"
    assert re.search(r"bool device_build = false;", (csrc / "rendering.h").read_text())
    assert (csrc / "amber_host.cc").read_text().count("options_.device_build ? AMBER_PT_FLAG_DEVICE_BUILD : 0u") == 2        # path tracing and light tracing
    exe = LIB.parent / "bin" / "amber"
    r = subprocess.run([str(exe), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--device-build" in r.stderr + r.stdout
