"""The scout, pt_megakernel<ENGINE_TWO_PHASE | AMBER_KERNEL_SCOUT>, holds the headline loop's resource figures (no GPU needed).

It is the loop of pt_megakernel<ENGINE_TWO_PHASE> (tests/test_headline_kernel_spills.py) without the path weight, and the flagship workload now runs it: no
scratch, six waves per SIMD, no SGPR parked in a VGPR lane inside the persistent loop, and no more lane reads there than the full kernel's loop has (11).
The full kernel itself must not have moved: tests/test_headline_kernel_spills.py and tests/test_host_model.py keep pinning it by its own symbol."""
import re
import shutil
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SCOUT = "_ZN12_GLOBAL__N_113pt_megakernelILi514ELb0ELb0EEEvNS_10RenderArgsE"      # 514 = ENGINE_TWO_PHASE | AMBER_KERNEL_SCOUT (0x200)
FULL = "_ZN12_GLOBAL__N_113pt_megakernelILi2ELb0ELb0EEEvNS_10RenderArgsE"
FULL_LOOP_LANE_READS = 11
VGPRS_AT_SIX_WAVES = 80                                                          # 512 registers per SIMD lane, allocated in blocks of 8: 6 waves of <= 80


@pytest.fixture(scope="module")
def listing():
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc on this box")
    sys.path.insert(0, str(ROOT / "tools"))
    import check_spill_placement as lint
    return lint.compile_to_asm([])


def persistent_loop(listing, kernel):
    body = listing[listing.index("\n" + kernel + ":"):]
    lines = body[:body.index("s_endpgm")].splitlines()
    header = next(i for i, line in enumerate(lines) if "=>This Loop Header: Depth=1" in line)
    label = re.match(r"^(\.LBB\d+_\d+):", lines[header])
    assert label, lines[header]
    back = [i for i, line in enumerate(lines) if line.split() == ["s_branch", label.group(1)]]
    assert back and back[-1] > header + 2500, back                              # the loop is the kernel
    return [line.strip() for line in lines[header:back[-1] + 1]]


def metadata(listing, kernel):
    """The kernel's entry in the listing's amdhsa.kernels metadata as a dict of its scalar fields."""
    at = listing.index(".name:           " + kernel)
    start = listing.rindex("  - .agpr_count:", 0, at)
    end = listing.find("  - .agpr_count:", at)
    entry = listing[start:end if end > 0 else None]
    return {k: v for k, v in re.findall(r"^\s+-?\s*\.(\w+):\s+(\S+)\s*$", entry, re.M)}


def test_the_scout_has_no_scratch_and_six_waves(listing):
    md = metadata(listing, SCOUT)
    print("\nscout:", {k: md[k] for k in ("private_segment_fixed_size", "vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count")})
    assert int(md["private_segment_fixed_size"]) == 0 and int(md["vgpr_spill_count"]) == 0
    assert int(md["vgpr_count"]) <= VGPRS_AT_SIX_WAVES                          # occupancy >= 6
    assert int(md["group_segment_fixed_size"]) <= 160 * 1024 // 6               # ... and LDS does not cap it lower: a workgroup is one wave per SIMD, six of them share a CU's 160 KB


def test_the_scouts_loop_parks_nothing_and_reads_no_more_lanes_than_the_full_loop(listing):
    scout, full = persistent_loop(listing, SCOUT), persistent_loop(listing, FULL)
    count = lambda loop, op: sum(1 for line in loop if line.startswith(op))
    reads, writes = count(scout, "v_readlane_b32"), count(scout, "v_writelane_b32")
    valu = lambda loop: sum(1 for line in loop if line.startswith("v_"))
    print(f"\nscout loop: {len(scout)} lines, {valu(scout)} VALU, {reads} v_readlane_b32, {writes} v_writelane_b32; "
          f"full loop: {len(full)} lines, {valu(full)} VALU, {count(full, 'v_readlane_b32')} v_readlane_b32")
    assert writes == 0
    assert reads <= FULL_LOOP_LANE_READS, reads
    assert valu(scout) < valu(full)                                             # the point of it: fewer vector instructions per trip
    assert not any(line.startswith(("v_div_scale_f64", "v_div_fmas_f64")) for line in scout)      # the eye weight's binary64 quotients are gone
