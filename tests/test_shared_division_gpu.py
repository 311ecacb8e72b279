"""The shared-denominator division on the device (csrc/hip/shared_div.h through amber_hip_kat_division) against the plain operator and NumPy.

mode 0 (Div3: one v_rcp_f32 and its refinement per denominator, the compiler's own correction steps per numerator, the wave falling back to the
plain expressions when a lane is out of range) must give the bits of mode 1 (`a / d, b / d, c / d` as hipcc compiles them: the parent's code)
EVERYWHERE, NaN payloads included, and both the bits of NumPy's binary32 `/`, which is correctly rounded (NaN results: NaN on both sides).
mode 2 (Normalize through the shared form, Normalize's own guard) against mode 3 (the plain form) the same way, and against a NumPy
restatement of Normalize with every operation rounded to binary32 in the source's order (x x + y y + z z left to right, sqrt, three divisions).
Whole waves of 64 are the unit that can go wrong (the guard is a wave vote); the largest inputs are what the cases ask for (2^22 random groups,
all 2^23 mantissas of a denominator), a few tenths of a second each."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def from_bits(b):
    return np.asarray(b, np.uint32).view(np.float32)


def numpy_div3(x):
    with np.errstate(all="ignore"):
        return x[:, :3] / x[:, 3:4]


def numpy_normalize(x):
    with np.errstate(all="ignore"):
        v = x[:, :3]
        s = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        return v / np.sqrt(s)[:, None]


def check(amber, x, label):
    """Div3 against the plain operator (all bits) and NumPy (all bits but NaN payloads); Normalize the same on {a, b, c}."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 4)
    for shared, plain, ref in ((0, 1, numpy_div3), (2, 3, numpy_normalize)):
        got, par, want = amber.kat_division(shared, x), amber.kat_division(plain, x), ref(x)
        differ = np.flatnonzero((bits(got) != bits(par)).any(axis=1))
        assert differ.size == 0, (label, shared, differ.size, x[differ[:4]].tolist(), got[differ[:4]].tolist(), par[differ[:4]].tolist())
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (label, shared)
        differ = np.flatnonzero(((bits(got) != bits(want)) & ~nan).any(axis=1))
        assert differ.size == 0, (label, shared, differ.size, x[differ[:4]].tolist(), got[differ[:4]].tolist(), want[differ[:4]].tolist())


def ulp(v, k):
    return from_bits(bits(F(v)) + np.uint32(k & 0xffffffff))[0]


SPECIAL = np.concatenate([
    np.array([0.0, -0.0, 1.0, -1.0, 3.0, 0.1, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.1754942e-38, 1.17549435e-38, 3.4028235e38, 1e-30, 1e30], F),
    from_bits([0x7f800001, 0xffc00000, 0x7fffffff, 0x3fffffff, 0x3f7fffff, 0x3f800001, 0x007fffff, 0x00800001]),     # NaNs with payloads, all-ones mantissas
    np.concatenate([[ulp(b, -1), F(b), ulp(b, 1), -ulp(b, -1), -F(b), -ulp(b, 1)] for b in (2.0 ** -20, 2.0 ** 40, 2.0 ** -60, 2.0 ** 41)]).astype(F),   # one ulp either side of every guard boundary
])


def test_random_groups_at_scene_magnitudes(amber):
    """2^22 groups: numerators of a Cornell path's size (positions up to a few units, directions, cross products with components next to zero),
    denominators 1e-3 ... 1e3; every eighth numerator exactly +-0."""
    rng = np.random.default_rng(20261018)
    n = 1 << 22
    x = np.empty((n, 4), F)
    x[:, :3] = (rng.standard_normal((n, 3)) * np.exp(rng.uniform(-12.0, 3.0, (n, 1)))).astype(F)
    x[:, :3][rng.random((n, 3)) < 0.125] = 0.0
    x[:, :3][rng.random((n, 3)) < 0.0625] *= F(-0.0)                  # some -0 (and +0 where the sign was negative)
    x[:, 3] = (np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n)) * rng.choice([-1.0, 1.0], n)).astype(F)
    check(amber, x, "random")


def test_every_mantissa_of_the_denominator(amber):
    """All 2^23 denominators of [0.5, 1) -- a length just below 1 is Normalize's common case, and 0x1.fffffep-1 the denominator for which the
    operation sequence depends on its seed (tests/test_shared_division.py) -- under a power of two, 3 and one random numerator each."""
    rng = np.random.default_rng(7)
    n = 1 << 23
    x = np.empty((n, 4), F)
    x[:, 3] = from_bits(np.arange(n, dtype=np.uint32) | np.uint32(0x3f000000))
    x[:, 0] = 1.0
    x[:, 1] = -3.0
    x[:, 2] = rng.uniform(-2.0, 2.0, n).astype(F)
    got, par, want = amber.kat_division(0, x), amber.kat_division(1, x), numpy_div3(x)
    assert np.array_equal(bits(got), bits(par))
    assert np.array_equal(bits(got), bits(want))
    # powers of two over the all-ones denominators of other binades, and numerators next to the denominator
    d = np.concatenate([from_bits(np.uint32(0x7fffff) | (np.arange(127 - 20, 127 + 40, dtype=np.uint32) << 23)), from_bits(np.uint32(0x7ffffd) | (np.arange(127 - 20, 127 + 40, dtype=np.uint32) << 23))])
    y = np.stack([np.ones_like(d), d * F(0.5), from_bits((bits(d) & np.uint32(0xff800000)) | np.uint32(0x555553)), d], 1)
    check(amber, np.concatenate([y, -y, y * np.array([1, -1, 1, -1], F)]), "all-ones denominators")


def test_structured_cases(amber):
    """+-0, one ulp inside and outside every guard boundary, subnormals, inf, NaN (payloads travel), all-ones mantissas, in every slot;
    n = d +- k ulp."""
    s = SPECIAL
    a, d = np.meshgrid(s, s, indexing="ij")
    a, d = a.ravel(), d.ravel()
    one, two = np.ones_like(a), np.full_like(a, -2.0)
    groups = [np.stack(g, 1) for g in ((a, one, two, d), (one, a, two, d), (one, two, a, d), (a, a, a, d), (d, a, d, a), (a, d, one, one))]
    rng = np.random.default_rng(3)
    dd = (np.exp(rng.uniform(-10, 10, 4096)) * rng.choice([-1.0, 1.0], 4096)).astype(F)
    near = np.stack([from_bits(bits(dd) + np.uint32(k & 0xffffffff)) for k in (-2, -1, 0, 1, 2)], 1)
    groups += [np.stack([near[:, i], near[:, j], -near[:, 2], dd], 1) for i, j in ((0, 1), (3, 4), (2, 2))]
    x = np.concatenate(groups).astype(F)
    check(amber, x, "structured")
    check(amber, x[:-37], "structured, a last wave that is not full")


def test_one_lane_of_a_wave_out_of_range(amber):
    """Six blocks of four waves in which exactly ONE lane is out of range (a different lane and a different reason per wave): the whole wave
    takes the fallback, and the 63 lanes in range get the same bits from it; then the same waves with every lane in range."""
    rng = np.random.default_rng(11)
    n = 6 * 256
    x = np.empty((n, 4), F)
    x[:, :3] = rng.uniform(-3.0, 3.0, (n, 3)).astype(F)
    x[:, 3] = rng.uniform(0.05, 4.0, n).astype(F)
    inside = x.copy()
    reasons = [(3, 0.0), (3, 1e-42), (3, 2.0 ** 40), (3, np.inf), (3, np.nan), (3, ulp(2.0 ** -20, -1)), (0, np.inf), (1, np.nan), (2, 1e-30), (0, 1e-44), (1, 2.0 ** 41), (2, -3e38)]
    for w in range(n // 64):
        slot, value = reasons[w % len(reasons)]
        x[w * 64 + (w * 7 + 3) % 64, slot] = value
    with np.errstate(all="ignore"):
        for shared, want in ((0, numpy_div3(x)), (2, numpy_normalize(x))):
            ok = ~np.isnan(want)
            assert np.array_equal(bits(amber.kat_division(shared, x))[ok], bits(want)[ok]), shared
    check(amber, x, "one lane out of range")
    check(amber, inside, "every lane in range")
