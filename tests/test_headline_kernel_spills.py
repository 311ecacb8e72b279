"""The persistent loop of the headline kernel, pt_megakernel<ENGINE_TWO_PHASE>, stays (nearly) free of SGPR-spill lane reads (no GPU needed).

The kernel lives at its SGPR limit, and what does not fit is parked in the lanes of a VGPR: a v_writelane_b32 to park, a v_readlane_b32 (plus
hazard s_nops) to fetch -- VALU instructions that compute nothing, in a kernel bound by VALU issue.  Before the cold kernel arguments were read
next to their use (pt_args.h, ColdArgs) the loop held 91 lane reads of loop-invariant kernel arguments (193 lane operations in the whole kernel);
since then it holds 11 (30 in the whole kernel): loop-invariant scalars of the per-bounce code, derived once from the scene record (loop guards
of the closest hit, candidate masks, the depth test).  tests/test_host_model.py pins the count of the whole kernel; this one pins the loop."""
import re
import shutil
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
KERNEL = "_ZN12_GLOBAL__N_113pt_megakernelILi2ELb0ELb0EEEvNS_10RenderArgsE"
LOOP_LANE_OPS_BEFORE, LOOP_LANE_OPS = 91, 11


def test_the_persistent_loop_has_no_spill_writes_and_few_spill_reads():
    """Between the persistent loop's header (the first `=>This Loop Header: Depth=1` label) and the s_branch back to it: at most 11
    v_readlane_b32 / v_writelane_b32 (91 before this change), and no v_writelane_b32 at all -- an invariant is never parked again inside the loop."""
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc on this box")
    sys.path.insert(0, str(ROOT / "tools"))
    import check_spill_placement as lint
    product = lint.compile_to_asm([])
    body = product[product.index("\n" + KERNEL + ":"):]
    lines = body[:body.index("s_endpgm")].splitlines()
    header = next(i for i, line in enumerate(lines) if "=>This Loop Header: Depth=1" in line)
    label = re.match(r"^(\.LBB\d+_\d+):", lines[header])
    assert label, lines[header]
    back = [i for i, line in enumerate(lines) if line.split() == ["s_branch", label.group(1)]]
    assert back and back[-1] > header + 3000, back                          # the loop is the kernel: some 3500 instructions
    loop = [line.strip() for line in lines[header:back[-1] + 1]]
    reads = sum(1 for line in loop if line.startswith("v_readlane_b32"))
    writes = sum(1 for line in loop if line.startswith("v_writelane_b32"))
    print(f"\npt_megakernel<2,false,false>: {len(loop)} lines in the persistent loop, {reads} v_readlane_b32, {writes} v_writelane_b32 (before: {LOOP_LANE_OPS_BEFORE} reads)")
    assert writes == 0
    assert reads + writes <= LOOP_LANE_OPS, reads
