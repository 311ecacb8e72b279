"""The square root from one v_rsq_f32 seed on the device (csrc/hip/exact_sqrt.h through amber_hip_kat_sqrt / amber_hip_kat_sqrt_sweep).

mode 0 (Sqrt1: v_rsq_f32, two multiplies, five fma; the wave falls back to __builtin_sqrtf when a lane is out of 2^-60 <= x < 2^60) must give the
bits of mode 1 (__builtin_sqrtf as hipcc compiles it: the parent's code) for EVERY one of the 2^32 bit patterns -- a one-operand function can be
checked exhaustively, and the sweep kernel does it on the device -- and both the bits of NumPy's binary32 sqrt, which is correctly rounded (NaN
results: NaN on both sides; payloads are compared with mode 1 only).  The sweep also reports how far v_rsq_f32 lies from the float nearest to
1 / sqrt(x): inside the +-3 ulp that tests/test_exact_sqrt.py covers on the host.  mode 4 is the two-operand form (one guard, one vote), mode 2
the fused Normalize (root and three quotients from the one seed) against mode 3 (the plain form) and a NumPy restatement with every operation
rounded to binary32 in the source's order.  Whole waves of 64 are the unit that can go wrong (the guards are wave votes).

Figures of one run on an MI355X: 0 mismatches over the 2^32 patterns, 1 006 632 960 of them in range, v_rsq_f32 at -1 ... +1 ulp of the nearest
float over every operand of the range; the module takes 1.9 s, the sweep 0.25 s of it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
HOST_SEED_WINDOW = 3                    # tests/exact_sqrt_main.cc: seeds from -3 to +3 ulp of the nearest float
LO, HI = 2.0 ** -60, 2.0 ** 60          # the fast form's range


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def from_bits(b):
    return np.asarray(b, np.uint32).view(np.float32)


def ulp(v, k):
    return from_bits(bits(F(v)) + np.uint32(k & 0xffffffff))[0]


def numpy_normalize(v):
    with np.errstate(all="ignore"):
        s = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        return v / np.sqrt(s)[:, None]


def check_roots(amber, x, label):
    """mode 0 against mode 1 (all bits) and NumPy (all bits but NaN payloads); the same values in pairs through mode 4."""
    x = np.ascontiguousarray(x, F).reshape(-1)
    with np.errstate(all="ignore"):
        want = np.sqrt(x)
    fast, plain = amber.kat_sqrt(0, x), amber.kat_sqrt(1, x)
    differ = np.flatnonzero(bits(fast) != bits(plain))
    assert differ.size == 0, (label, differ.size, x[differ[:4]].tolist(), fast[differ[:4]].tolist(), plain[differ[:4]].tolist())
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(fast), nan), label
    differ = np.flatnonzero((bits(fast) != bits(want)) & ~nan)
    assert differ.size == 0, (label, differ.size, x[differ[:4]].tolist(), fast[differ[:4]].tolist(), want[differ[:4]].tolist())
    pairs = np.stack([x, x[::-1]], 1)                      # lane k holds items k and n - 1 - k: another partner for every value
    both = amber.kat_sqrt(4, pairs)
    assert np.array_equal(bits(both[:, 0]), bits(plain)) and np.array_equal(bits(both[:, 1]), bits(plain[::-1])), label


def check_normalize(amber, v, label):
    v = np.ascontiguousarray(v, F).reshape(-1, 3)
    fused, plain, want = amber.kat_sqrt(2, v), amber.kat_sqrt(3, v), numpy_normalize(v)
    differ = np.flatnonzero((bits(fused) != bits(plain)).any(axis=1))
    assert differ.size == 0, (label, differ.size, v[differ[:4]].tolist(), fused[differ[:4]].tolist(), plain[differ[:4]].tolist())
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(fused), nan), label
    differ = np.flatnonzero(((bits(fused) != bits(want)) & ~nan).any(axis=1))
    assert differ.size == 0, (label, differ.size, v[differ[:4]].tolist(), fused[differ[:4]].tolist(), want[differ[:4]].tolist())


@pytest.fixture(scope="module")
def sweep(amber):
    """All 2^32 bit patterns in four calls of 2^30."""
    return [amber.kat_sqrt_sweep(k << 30, 1 << 30) for k in range(4)]


def test_every_bit_pattern_has_the_bits_of_the_plain_square_root(sweep):
    assert [s["mismatches"] for s in sweep] == [0, 0, 0, 0], [(s["mismatches"], [hex(b) for b in s["offenders"]]) for s in sweep]
    assert sum(s["in_range"] for s in sweep) == 120 << 23            # the 120 binades of 2^-60 <= x < 2^60, positive only
    assert sweep[2]["in_range"] == 0 and sweep[3]["in_range"] == 0   # a set sign bit is out of range


def test_the_hardware_seed_lies_inside_the_window_the_host_check_covers(sweep):
    low, high = min(s["seed_low"] for s in sweep), max(s["seed_high"] for s in sweep)
    print(f"\nv_rsq_f32 against the float nearest to 1 / sqrt(x), all in-range operands: {low:+d} ... {high:+d} ulp")
    assert -HOST_SEED_WINDOW <= low and high <= HOST_SEED_WINDOW, (low, high)


def test_every_mantissa_of_two_exponents(amber):
    """All 2^23 mantissas of [1, 2) and of [2, 4): both exponent parities, 64 MiB."""
    check_roots(amber, from_bits(np.arange(1 << 24, dtype=np.uint32) + np.uint32(0x3f800000)), "two binades")


SPECIAL = np.concatenate([
    np.array([0.0, -0.0, 1.0, -1.0, 2.0, 3.0, 4.0, 0.1, 0.25, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.1754942e-38, 1.17549435e-38, 3.4028235e38, 1e-30, 1e30, -1e-30, -2.0 ** -60], F),
    from_bits([0x7f800001, 0xffc00000, 0x7fffffff, 0xffc12345, 0x3fffffff, 0x3f7fffff, 0x3f800001, 0x007fffff, 0x00800001, 0x00000001, 0x80000001]),   # NaNs with payloads, all-ones mantissas, subnormals
    np.array([f(b, k) for b in (LO, HI, 2.0 ** -40) for k in (-1, 0, 1) for f in (ulp, lambda v, j: -ulp(v, j))], F),                              # one ulp either side of every bound, both signs
])


def test_structured_cases(amber):
    """+-0, one ulp inside and outside the bounds, subnormals, inf, NaN (payloads travel), negatives: every value next to every other one in
    the two-operand form, and in whole waves of its own; then a last wave that is not full."""
    a, b = np.meshgrid(SPECIAL, SPECIAL, indexing="ij")
    x = np.concatenate([a.ravel(), np.repeat(SPECIAL, 64)])
    check_roots(amber, x, "structured")
    check_roots(amber, x[:-37], "structured, a last wave that is not full")
    pairs = amber.kat_sqrt(4, np.stack([a.ravel(), b.ravel()], 1))
    plain_a, plain_b = amber.kat_sqrt(1, a.ravel()), amber.kat_sqrt(1, b.ravel())
    assert np.array_equal(bits(pairs[:, 0]), bits(plain_a)) and np.array_equal(bits(pairs[:, 1]), bits(plain_b))
    with np.errstate(all="ignore"):
        v = np.stack([a.ravel(), b.ravel(), np.resize(SPECIAL[::-1], a.size)], 1)
    check_normalize(amber, v, "structured vectors")
    check_normalize(amber, v[:-37], "structured vectors, a last wave that is not full")


def test_one_lane_of_a_wave_out_of_range(amber):
    """Waves in which exactly ONE lane is out of range (a different lane and a different reason per wave): the whole wave takes the fallback and
    the 63 lanes in range get the same bits from it; then the same waves with every lane in range; the last wave is not full."""
    rng = np.random.default_rng(11)
    n = 6 * 256 - 19
    inside = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), n)).astype(F)
    x = inside.copy()
    reasons = [0.0, -0.0, 1e-42, np.inf, np.nan, -1.0, ulp(LO, -1), HI, 3e38, 1e-37, -1e-30, from_bits([0x7f800001])[0]]
    for w in range((n + 63) // 64):
        x[min(w * 64 + (w * 7 + 3) % 64, n - 1)] = reasons[w % len(reasons)]
    check_roots(amber, x, "one lane out of range")
    check_roots(amber, inside, "every lane in range")
    v = rng.uniform(-3.0, 3.0, (n, 3)).astype(F)
    inside_v = v.copy()
    vector_reasons = [(0, 0.0, 0.0, 0.0), (1, np.inf, 1.0, 1.0), (2, np.nan, 1.0, 1.0), (0, 1e-25, 0.0, 0.0), (1, 1e-30, 1.0, 1.0), (2, 2.0 ** 31, 1.0, 1.0), (0, 1e-45, 1.0, 1.0), (1, 3e38, 0.0, 0.0)]
    for w in range((n + 63) // 64):
        slot, value, b, c = vector_reasons[w % len(vector_reasons)]
        row = np.array([b, c, c], F)
        row[slot] = value
        v[min(w * 64 + (w * 5 + 1) % 64, n - 1)] = row
    check_normalize(amber, v, "one vector of a wave out of range")
    check_normalize(amber, inside_v, "every vector in range")


def test_normalize_random_groups_at_scene_magnitudes(amber):
    """2^22 vectors of a Cornell path's size (directions, cross products with components next to zero, exact zeros); a third of unit length."""
    rng = np.random.default_rng(20261019)
    n = 1 << 22
    v = (rng.standard_normal((n, 3)) * np.exp(rng.uniform(-12.0, 3.0, (n, 1)))).astype(F)
    v[rng.random((n, 3)) < 0.125] = 0.0
    v[rng.random((n, 3)) < 0.0625] *= F(-0.0)
    with np.errstate(all="ignore"):
        v[::3] = numpy_normalize(v[::3])
    check_normalize(amber, v, "random")


def test_normalize_every_length_of_a_binade(amber):
    """All 2^23 lengths of [0.5, 1) -- 0x1.fffffep-1 is the length of a vector that was normalised already -- as (l, 0, 0) and as a general
    direction rescaled to about that length."""
    n = 1 << 23
    l = from_bits(np.arange(n, dtype=np.uint32) | np.uint32(0x3f000000))
    axis = np.zeros((n, 3), F)
    axis[:, 0] = l
    check_normalize(amber, axis, "axis vectors")
    rng = np.random.default_rng(5)
    d = numpy_normalize(rng.standard_normal((n, 3)).astype(F))
    check_normalize(amber, d * l[:, None], "rescaled directions")
