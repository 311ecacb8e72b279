"""Accumulation without owners on synthetic records: amber_hip_kat_accumulate (the product's EmitRecords / CloseRecords, rank / scan / place / reduce
kernels and host state, fed by the caller's records) against tests/path_accumulate_reference.py, bit for bit, at the shapes where each branch of
reduce_flagged_kernel, the scan carry, the slot reservation and the bitmap bookkeeping can go wrong; then the product's own emitters on the same
branches (a scene in which most paths reach a light, against the oracle).

Which branch a shape reaches: n_samples % 32 != 0 -> bit by bit; otherwise the word walk, with sixteen-word uint4 trips where the pixel's first word is
a multiple of four (nw = n_samples / 32 >= 16), the scalar tail for nw % 16 words, and alternating alignment from pixel to pixel when nw is odd."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import path_accumulate_reference as R

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

SPHERES = dict(
    materials=[(4, (3.0, 2.0, 1.0), 0.0), (0, (0.7, 0.7, 0.7), 0.0), (2, (0.9, 0.9, 0.9), 0.0)],
    objects=[(1, 0, [0.0, 2.0, 0.0, 0.5]), (1, 1, [0.0, -100.5, 0.0, 100.0]), (1, 1, [-0.6, 0.0, 0.0, 0.5]), (1, 2, [0.6, 0.0, 0.0, 0.5])],
    transform=[1, 0, 0, 0, 0, 1, 0, 0.3, 0, 0, 1, 3.0, 0, 0, 0, 1], focal_length=0.05, focus_distance=3.0, radius=0.02, n_blades=6,
)
# pixels -> (width, height, rows or None)
FRAME = {1: (1, 1, None), 3: (3, 1, None), 16: (4, 4, None), 50: (10, 5, None), 64: (8, 8, None), 77: (11, 7, None), 255: (51, 5, None), 256: (16, 16, None),
         257: (257, 3, (1, 2)), 300: (20, 15, None), 512: (32, 16, None), 1000: (40, 27, (1, 26)), 262145: (2405, 109, None), 262400: (640, 410, None)}


@pytest.fixture(scope="module")
def scene(amber):
    if not amber.is_lab():
        pytest.fail("the suite runs on the lab build")
    return amber.HostScene.create(**SPHERES)


def handle(amber, scene, n_pixels, **kw):
    w, h, rows = FRAME[n_pixels]
    pt = amber.PathTracer(scene, amber.Sensor.default(w, h), seed=3, rows=rows, **kw)
    assert pt.band_shape[0] * pt.band_shape[1] == n_pixels
    return pt


class Ledger:
    """A handle and what its framebuffer and ray total must hold: every launch is added to both and compared."""

    def __init__(self, pt, n_pixels):
        self.pt, self.n_pixels = pt, n_pixels
        self.fb, self.rays = np.zeros((n_pixels, 3), np.float32), 0

    def launch(self, n_samples, q, rgb, rays=0, expect=None, **kw):
        info = self.pt.kat_accumulate(n_samples, q, rgb, rays=rays, **kw)
        self.fb = expect if expect is not None else R.accumulate(self.fb, self.n_pixels, n_samples, q, rgb)
        self.rays += rays
        self.check()
        assert info["flags_dirty"] or info["flag_words_set"] == 0, info           # the bitmap is zero whenever the host believes it is
        assert info["flags_dirty"] == (1 if n_samples % 32 else 0), info          # (a launch that stood leaves it dirty only where pixels do not own words)
        return info

    def check(self):
        img, rays = self.pt.download()
        ok = R.same(img, self.fb)
        assert ok.all(), f"{int((~ok).sum())} of {ok.size} components differ, first at {np.flatnonzero(~ok)[:8]}"
        assert rays == self.rays

    def twice(self, n_samples, q, rgb, rays=0, **kw):
        """Onto the cleared framebuffer, then once more onto the result: fb + P, not a longer chain."""
        first = self.launch(n_samples, q, rgb, rays=rays, **kw)
        self.launch(n_samples, q, rgb, rays=rays + 1, **kw)
        return first


# ---- the table ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.DENSE_CASES) + list(R.SPARSE_CASES))
def test_table(amber, scene, name):
    n_pixels, n_samples, density = {**R.DENSE_CASES, **R.SPARSE_CASES}[name]
    q, rgb = R.make_case(n_pixels, n_samples, density, R.case_seed(name))
    led = Ledger(handle(amber, scene, n_pixels), n_pixels)
    info = led.twice(n_samples, q, rgb, rays=1000)
    n_records = int((q != R.MARKER).sum())
    assert info["n_repeats"] == 0 and info["n_launches"] == 1 and n_records <= info["rec_count"] and info["rec_count"] % 64 == 0
    led.pt.close()


def test_scan_carry_one_sample(amber, scene):
    """262 145 pixels: 1025 rank blocks, the last one a single pixel behind the carry of rec_scan_blocks_kernel's first pass."""
    n_pixels = 262145
    q, rgb = R.make_case(n_pixels, 1, 0.01, 77, forced=(0, 255, 256, 262143, 262144))
    led = Ledger(handle(amber, scene, n_pixels), n_pixels)
    led.twice(1, q, rgb, rays=5)
    led.pt.close()


def test_scan_carry_words(amber, scene):
    """262 400 pixels x 32 samples at density 0.01: records in the first and the last rank block and on either side of block 1024."""
    n_pixels, n = 262400, 32
    forced = (0, 255 * n + 7, 262143 * n + 31, 262144 * n, 262144 * n + 9, 262399 * n + 31)
    q, rgb = R.make_case(n_pixels, n, 0.01, 78, forced=forced)
    led = Ledger(handle(amber, scene, n_pixels), n_pixels)
    led.twice(n, q, rgb, rays=6)
    led.pt.close()


def test_path_indices_past_2_31(amber, scene):
    """262 400 pixels x 8192 samples: pixel 262 144 begins at path 2^31, so the bitmap positions, the pixel quotients and the word offsets of the last 256
    pixels need all 32 bits.  (A render launch stays below 2^30 paths; the kernels are written for any 32-bit path index.)  Records in six pixels, on
    either side of 2^31; the reference is taken over those pixels alone -- every other pixel has no record and stays +0."""
    n_pixels, n = 262400, 8192
    pixels = np.array([0, 1000, 262143, 262144, 262145, 262399])
    rng = np.random.default_rng(86)
    local = R.lit_paths(rng, len(pixels), n, 0.05, forced=(0, n - 1, 3 * n, 5 * n + n - 1))       # path indices as if the six pixels were the band
    q = (pixels[local // n].astype(np.uint64) * n + local % n).astype(np.uint32)
    assert (q >= 1 << 31).sum() > 1000 and (q < 1 << 31).sum() > 1000
    rgb = R.values(rng, len(q))
    order = rng.permutation(len(q))
    qi, ci, _ = R.interleave(rng, q[order], rgb[order])
    led = Ledger(handle(amber, scene, n_pixels), n_pixels)
    for rays in (12, 13):                                                # onto the cleared buffer, then onto the result
        expect = led.fb.copy()
        expect[pixels] = R.accumulate(led.fb[pixels], len(pixels), n, local[order], rgb[order])
        led.launch(n, qi, ci, rays=rays, expect=expect)
    assert led.fb[pixels].any(axis=1).all() and np.count_nonzero(led.fb.any(axis=1)) == len(pixels)
    led.pt.close()


def test_untouched_pixels(amber, scene):
    """Every record in pixels 0, 255, 256, 511 of 512: the reduction skips the rest, and the exclusive prefixes cross empty pixels and a block edge."""
    q, rgb = R.make_case(512, 64, 1.0, 79, only_pixels=(0, 255, 256, 511))
    assert int((q != R.MARKER).sum()) == 4 * 64
    led = Ledger(handle(amber, scene, 512), 512)
    led.twice(64, q, rgb, rays=7)
    assert not led.fb[1:255].any() and led.fb[[0, 255, 256, 511]].any(axis=1).all()
    led.pt.close()


# ---- values -------------------------------------------------------------------------------------------------------------------------------

def test_special_values(amber, scene):
    """-0, infinities, the canonical NaN, subnormals and FLT_MAX pairs that overflow within a chunk, among ordinary records, on 16 x 64.
    (Subnormals are kept by this build: a difference in pixel 4 or 5 alone would be a finding about the build's denormal mode.)"""
    n_pixels, n = 16, 64
    rng = np.random.default_rng(80)
    big, tiny, nan, inf = np.float32(np.finfo(np.float32).max), np.float32(1e-45), np.float32(np.nan), np.float32(np.inf)
    assert R.bits(nan) == 0x7FC00000
    rec = {}
    for k in (0, 3, 8, 40, 63):
        rec[0 * n + k] = [-0.0, -0.0, -0.0]                              # pixel 0: only -0 records: emitted, and the pixel stays +0
    rec.update({1 * n + 2: [inf, -inf, inf], 1 * n + 5: [-inf, -inf, 1.0], 1 * n + 20: [1.0, inf, -inf]})       # NaN within a chunk, -inf, NaN across chunks
    rec.update({2 * n + 0: [nan, 1.0, 2.0], 2 * n + 9: [1.0, nan, 2.0], 2 * n + 63: [3.0, 4.0, 5.0]})
    rec.update({3 * n + 1: [big, big, -big], 3 * n + 2: [big, -big, -big], 3 * n + 3: [-big, big, big],          # overflow within a chunk, then back: inf stays
                3 * n + 17: [big, 1.0, 1.0], 3 * n + 25: [big, 1.0, 1.0]})                                         # ... and across chunks
    for k in range(0, 64, 3):
        rec[4 * n + k] = (tiny * rng.integers(-(1 << 17), 1 << 17, 3).astype(np.float32)).tolist()              # pixel 4: subnormals only
    rec.update({5 * n + 4: [1e-40, 1.17549435e-38, -1e-40], 5 * n + 5: [-1e-40, -1.17549421e-38, 3e-45], 5 * n + 30: [2e-45, 1e-39, 1e-38]})
    lit = np.array([p for p in R.lit_paths(rng, n_pixels, n, 0.5) if p >= 6 * n], np.uint32)
    q = np.concatenate([np.array(list(rec), np.uint32), lit])
    rgb = np.concatenate([np.array(list(rec.values()), np.float32), R.values(rng, len(lit))])
    order = rng.permutation(len(q))
    q, rgb, _ = R.interleave(rng, q[order], rgb[order])
    led = Ledger(handle(amber, scene, n_pixels), n_pixels)
    led.twice(n, q, rgb, rays=8)
    assert not R.bits(led.fb[0]).any()                                  # +0, not -0
    assert np.isnan(led.fb[1]).sum() >= 2 and np.isnan(led.fb[2, :2]).all() and np.isinf(led.fb[3, 0])
    assert (np.abs(led.fb[4]) < np.float32(1.2e-38)).all() and led.fb[4].any()          # the reference itself keeps the subnormals
    led.pt.close()


# ---- slots --------------------------------------------------------------------------------------------------------------------------------

def slot_case(counts, seed, n_pixels=16, n=64):
    """Records on n_pixels x n spread over trips with exactly these emit counts."""
    rng = np.random.default_rng(seed)
    lit = rng.permutation(n_pixels * n)[: sum(counts)].astype(np.uint32)
    q, rgb, used = R.interleave(rng, lit, R.values(rng, len(lit)), counts=list(counts))
    assert list(used) == list(counts) and len(q) == 64 * len(counts)
    return q, rgb


@pytest.mark.parametrize("capacity, repeats", [(128, 0), (127, 1), (64, 1)])
def test_slots_exact_fit_and_one_short(amber, scene, capacity, repeats):
    """128 records of one wave: two blocks, rec_count == 128.  A buffer of 128 slots stands; 127, or 64, is one launch repeated -- rays counted once."""
    q, rgb = slot_case((64, 64), 81)
    led = Ledger(handle(amber, scene, 16), 16)
    info = led.launch(64, q, rgb, rays=123, n_waves=1, rec_capacity=capacity)
    assert info["n_repeats"] == repeats and info["n_launches"] == 1 + repeats
    assert info["rec_count"] == 128
    led.pt.close()


@pytest.mark.parametrize("counts, rec_count", [((40, 40), 128), ((64, 1), 128), ((24, 40), 64), ((40, 24, 64, 1), 192)])
def test_slots_straddle_and_exact_fit_of_a_block(amber, scene, counts, rec_count):
    """40 then 40: the second trip straddles two blocks (n > room).  64 then 1: a block filled exactly, then one record in a new one whose 63 other
    slots are closed.  24 then 40: n == room.  The buffer has exactly the slots the wave reserves."""
    q, rgb = slot_case(counts, 82)
    led = Ledger(handle(amber, scene, 16), 16)
    info = led.launch(64, q, rgb, rays=9, n_waves=1, rec_capacity=rec_count)
    assert info["n_repeats"] == 0 and info["rec_count"] == rec_count
    led.launch(64, q, rgb, rays=10, n_waves=1, rec_capacity=rec_count)
    led.pt.close()


def test_unused_slots_do_not_show_stale_records(amber, scene):
    """A large call fills the record buffer; a later call on the same handle ends with a trip that leaves 63 slots of its block unused.  What the
    earlier call left there must not be placed again."""
    led = Ledger(handle(amber, scene, 16), 16)
    q, rgb = slot_case((64,) * 12, 83)
    led.launch(64, q, rgb, rays=1, n_waves=1)
    q, rgb = slot_case((64, 1), 84)
    info = led.launch(64, q, rgb, rays=2, n_waves=1)
    assert info["rec_count"] == 128
    q, rgb = slot_case((3,), 85)
    info = led.launch(64, q, rgb, rays=3, n_waves=1)
    assert info["rec_count"] == 64
    led.pt.close()


# ---- waves, sequences, engines ------------------------------------------------------------------------------------------------------------

def test_any_number_of_waves_gives_the_same_bits(amber, scene):
    n_pixels, n_samples, density = R.DENSE_CASES["300x512"]
    q, rgb = R.make_case(n_pixels, n_samples, density, R.case_seed("300x512"))
    expect = R.accumulate(np.zeros((n_pixels, 3), np.float32), n_pixels, n_samples, q, rgb)
    for n_waves in (1, 4, 61, 1024):
        led = Ledger(handle(amber, scene, n_pixels), n_pixels)
        info = led.launch(n_samples, q, rgb, rays=n_waves, expect=expect, n_waves=n_waves)
        assert info["n_repeats"] == 0, (n_waves, info)
        led.pt.close()


def test_launches_in_sequence_on_one_handle(amber, scene):
    """64, 33, 64, a 64 whose first attempt runs out of slots, 32, then a launch without items: the bitmap is cleared by the reduction, by the host
    after 33 samples and after the launch that ran out; the reference is cumulative."""
    n_pixels = 16
    led = Ledger(handle(amber, scene, n_pixels), n_pixels)
    small = 192
    plan = [(64, 0.1, small, 0), (33, 0.2, small, 0), (64, 0.1, small, 0), (64, 1.0, small, 1), (32, 0.3, 0, 0)]
    for k, (n, density, capacity, repeats) in enumerate(plan):
        q, rgb = R.make_case(n_pixels, n, density, 90 + k)
        info = led.launch(n, q, rgb, rays=100 + k, n_waves=1, rec_capacity=capacity)
        assert info["n_repeats"] == repeats and info["n_launches"] == 1 + repeats, (k, info)
        assert (info["rec_count"] > small) == bool(repeats)
    before = led.fb.copy()
    info = led.launch(64, np.zeros(0, np.uint32), np.zeros((0, 3), np.float32), rays=17)
    assert info["rec_count"] == 0 and info["n_launches"] == 1 and np.array_equal(R.bits(before), R.bits(led.fb))
    q, rgb = R.make_case(n_pixels, 64, 0.5, 99)
    led.launch(64, q, rgb, rays=1)
    led.pt.close()


def test_any_engine(amber, scene):
    n_pixels, n_samples, density = R.DENSE_CASES["77x544"]
    q, rgb = R.make_case(n_pixels, n_samples, density, R.case_seed("77x544"))
    expect = R.accumulate(np.zeros((n_pixels, 3), np.float32), n_pixels, n_samples, q, rgb)
    for engine, flags in ((amber.ENGINE_LIST, 0), (amber.ENGINE_TWO_PHASE, 0), (amber.ENGINE_BVH, 0), (amber.ENGINE_BVH, amber.api.PT_FLAG_BVH_POOL),
                          (amber.ENGINE_BVH, amber.api.PT_FLAG_BVH_ITEMS), (amber.ENGINE_REFERENCE_BVH, 0), (amber.ENGINE_WAVEFRONT, 0)):
        led = Ledger(handle(amber, scene, n_pixels, engine=engine, flags=flags), n_pixels)
        led.launch(n_samples, q, rgb, rays=11, expect=expect)
        led.pt.close()


def test_a_launch_after_product_passes(amber, scene):
    """The hook on a handle that has rendered: the product's passes and the synthetic launch share the bitmap and the record buffer."""
    n_pixels = 300
    led = Ledger(handle(amber, scene, n_pixels), n_pixels)
    led.pt.render_pass(0, 33)                                            # leaves the bitmap dirty
    img, rays = led.pt.download()
    led.fb, led.rays = img.reshape(n_pixels, 3).copy(), rays
    assert not (np.signbit(led.fb) & (led.fb == 0)).any()
    q, rgb = R.make_case(n_pixels, 64, 0.5, 100)
    led.launch(64, q, rgb, rays=4)
    led.pt.close()
    # ... and the other way round: launches without items between two passes change neither the image nor what the next pass finds in the bitmap
    a, b = handle(amber, scene, n_pixels), handle(amber, scene, n_pixels)
    a.render_pass(0, 33); b.render_pass(0, 33)
    none = (np.zeros(0, np.uint32), np.zeros((0, 3), np.float32))
    assert a.kat_accumulate(64, *none, rays=5)["flags_dirty"] == 0 and a.kat_accumulate(33, *none, rays=6)["flags_dirty"] == 1
    a.render_pass(33, 64); b.render_pass(33, 64)
    (ia, ra), (ib, rb) = a.download(), b.download()
    assert ra == rb + 11 and np.array_equal(R.bits(ia), R.bits(ib)) and ia.any()
    a.close(); b.close()


# ---- refusals and the ABI -----------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing(amber, scene):
    n_pixels, n = 16, 64
    led = Ledger(handle(amber, scene, n_pixels), n_pixels)
    q, rgb = R.make_case(n_pixels, n, 0.5, 110)
    led.launch(n, q, rgb, rays=31)                                       # the buffer now has a slot per item plus the slack
    one = np.ones((2, 3), np.float32)
    refused = [
        dict(n_samples=n, q=[5, n_pixels * n], rgb=one),                 # out of range by one
        dict(n_samples=n, q=[5, 0xFFFFFFFE], rgb=one),
        dict(n_samples=n, q=[7, 7], rgb=one),                            # twice
        dict(n_samples=0, q=[0, 1], rgb=one),
        dict(n_samples=n, q=[0, 1], rgb=one, n_waves=0),
        dict(n_samples=n, q=[0, 1], rgb=one, rec_capacity=64),           # below what the buffer holds
        dict(n_samples=1 << 28, q=[0, 1], rgb=one),                      # 16 pixels x 2^28 samples = 2^32 paths
    ]
    for k, kw in enumerate(refused):
        with pytest.raises(amber.AmberError, match="amber error -1"):
            led.pt.kat_accumulate(rays=1000, **kw)
        led.check()
        q, rgb = R.make_case(n_pixels, n, 0.3, 111 + k)
        led.launch(n, q, rgb, rays=1)
    led.pt.close()


def test_the_product_does_not_export_the_hook(amber):
    lib = ROOT / "amber_amd" / "lib" / amber.api.PRODUCT_LIB
    code = "import ctypes, json, sys; lib = ctypes.CDLL(sys.argv[1]); print(json.dumps([hasattr(lib, n) for n in ('amber_hip_pt_render_pass', 'amber_hip_kat_accumulate')]))"
    out = subprocess.run([sys.executable, "-c", code, str(lib)], capture_output=True, text=True, check=True).stdout
    assert json.loads(out) == [True, False]
    assert "amber_hip_kat_accumulate" in amber.api.LAB_SYMBOLS and "amber_hip_kat_accumulate" not in amber.api.ABI_SYMBOLS
    assert "int amber_hip_kat_accumulate(amber_hip_pt*, uint32_t n_samples," in (ROOT / "include" / "amber_hip_lab.h").read_text()
    assert "amber_hip_kat_accumulate" not in (ROOT / "include" / "amber_hip.h").read_text()
    import ctypes as C
    assert C.sizeof(amber.api.AccumulateInfo) == 20 and [n for n, _ in amber.api.AccumulateInfo._fields_] == ["n_launches", "n_repeats", "rec_count", "flag_words_set", "flags_dirty"]
    assert "typedef struct { uint32_t n_launches, n_repeats, rec_count, flag_words_set, flags_dirty; } AmberAccumulateInfo;" in (ROOT / "include" / "amber_hip_lab.h").read_text()


# ---- the join with the product kernels ---------------------------------------------------------------------------------------------------

JOIN_W, JOIN_H, JOIN_SEED = 24, 16, 5
JOIN_SINGLE = (64, 544, 1056)
JOIN_SEQUENCE = ((0, 544), (544, 33), (577, 512))


@pytest.fixture(scope="module")
def join(amber):
    """The oracle's images of the dense scene, computed once: one launch of 64, 544 and 1056 samples, and the three passes on one framebuffer."""
    import oracle_binding as O
    from test_round3_gpu import LIGHT_BOX
    osc = O.Scene.create(**LIGHT_BOX)
    one, _ = osc.render_xorshift(JOIN_W, JOIN_H, JOIN_SEED, 0, 1, chunk=1)
    assert (one.sum(axis=2) > 0).mean() > 0.5                            # more than half of the paths carry a record
    single = {n: osc.render_xorshift(JOIN_W, JOIN_H, JOIN_SEED, 0, n, threads=16) for n in JOIN_SINGLE}
    seq, casts = np.zeros((JOIN_H, JOIN_W, 3), np.float32), 0
    for first, n in JOIN_SEQUENCE:
        _, c = osc.render_xorshift(JOIN_W, JOIN_H, JOIN_SEED, first, n, threads=16, out=seq)
        casts += c.casts
    return amber.HostScene.create(**LIGHT_BOX), single, (seq, casts)


@pytest.mark.parametrize("engine", ["two_phase", "list", "bvh_pool", "bvh_paths"])
def test_product_emitters_on_the_dense_branches(amber, join, engine):
    """render_pass at 64 (word walk, two words), 544 (uint4 trip + tail, alignment alternating) and 1056 samples (two trips + tail) of a scene in which
    most paths end on a light, then 544 + 33 + 512 on one handle (fast path, bit by bit with the host's clear, aligned trips): image bits and ray
    count against the oracle.  bvh_paths: engine BVH without a scheduler flag renders this shallow tree with the path-granular pt_megakernel."""
    hs, single, (seq, seq_casts) = join
    kw = {"two_phase": dict(engine=amber.ENGINE_TWO_PHASE), "list": dict(engine=amber.ENGINE_LIST),
          "bvh_pool": dict(engine=amber.ENGINE_BVH, flags=amber.api.PT_FLAG_BVH_POOL), "bvh_paths": dict(engine=amber.ENGINE_BVH)}[engine]
    sn = amber.Sensor.default(JOIN_W, JOIN_H)
    for n in JOIN_SINGLE:
        ref, cnt = single[n]
        pt = amber.PathTracer(hs, sn, seed=JOIN_SEED, **kw)
        pt.render_pass(0, n)
        img, rays = pt.download()
        assert rays == cnt.casts and np.array_equal(R.bits(img), R.bits(ref)), (engine, n)
        pt.close()
    pt = amber.PathTracer(hs, sn, seed=JOIN_SEED, **kw)
    for first, n in JOIN_SEQUENCE:
        pt.render_pass(first, n)
    img, rays = pt.download()
    assert rays == seq_casts and np.array_equal(R.bits(img), R.bits(seq)), engine
    pt.close()
