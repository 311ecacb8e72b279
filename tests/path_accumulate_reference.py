"""The accumulation contract of a path launch restated in numpy from its text, not from the device code, and the synthetic
record lists that tests/test_path_accumulate.py feeds to amber_hip_kat_accumulate.

A launch covers n_samples samples of n_pixels band pixels; path q = pixel * n_samples + sample ends with the measurement m(q), +0 unless a record
says otherwise.  Every operation is binary32 and rounded alone.  For every pixel and every chunk of ACCUM_CHUNK = 8 consecutive samples, counted from
sample 0 of the launch,
    s = +0;  s = s + m(k) for every sample k of the chunk in order (unlit samples add their +0: they are NOT left out);  fb[pixel] = fb[pixel] + s
chunk by chunk.  The device leaves the +0 terms (and chunks, and pixels, without a record) out; that this changes no bit is what equality with this
file proves.

PRECONDITION: the framebuffer going in holds no -0 (the product only ever adds to a buffer cleared to +0, and x + y is -0 only when both are).
NaN: a result is compared as "NaN in the same component" (same()); inputs use only the canonical quiet NaN.  Everything else bit for bit.
"""
import numpy as np

ACCUM_CHUNK = 8
MARKER = np.uint32(0xFFFFFFFF)          # q of an item that emits nothing


def dense(n_pixels: int, n_samples: int, q, rgb) -> np.ndarray:
    """m as an array (n_pixels, n_samples, 3): +0 everywhere but where a record says otherwise.  Items with q == MARKER are not records."""
    q = np.asarray(q, np.uint32).reshape(-1)
    rgb = np.asarray(rgb, np.float32).reshape(-1, 3)
    keep = q != MARKER
    q, rgb = q[keep].astype(np.int64), rgb[keep]
    assert (q < n_pixels * n_samples).all() and len(np.unique(q)) == len(q)
    m = np.zeros((n_pixels * n_samples, 3), np.float32)
    m[q] = rgb
    return m.reshape(n_pixels, n_samples, 3)


def accumulate_dense(fb, m: np.ndarray, chunk: int = ACCUM_CHUNK) -> np.ndarray:
    """fb (n_pixels * 3 values, float32, never modified) after a launch with the measurements m (n_pixels, n_samples, 3); one rounded binary32
    addition per array operation.  `chunk` is the contract's 8; the CPU test passes other values to build accumulators that must differ."""
    n_pixels, n_samples, _ = m.shape
    out = np.array(fb, np.float32, copy=True).reshape(n_pixels, 3)
    assert not (np.signbit(out) & (out == 0)).any(), "precondition: no -0 in the framebuffer"
    with np.errstate(all="ignore"):
        for c0 in range(0, n_samples, chunk):
            s = np.zeros((n_pixels, 3), np.float32)
            for k in range(c0, min(c0 + chunk, n_samples)):
                s = s + m[:, k, :]
            out = out + s
    assert out.dtype == np.float32
    return out


def accumulate(fb, n_pixels: int, n_samples: int, q, rgb) -> np.ndarray:
    """The contract: fb (n_pixels, 3) after one launch over n_samples samples with the records (q[i], rgb[i])."""
    return accumulate_dense(fb, dense(n_pixels, n_samples, q, rgb))


def accumulate_naive(fb, n_pixels: int, n_samples: int, q, rgb) -> np.ndarray:
    """The same sentence as a per-pixel Python loop over np.float32 scalars (small cases only)."""
    m = {int(k): np.asarray(v, np.float32) for k, v in zip(np.asarray(q).reshape(-1), np.asarray(rgb, np.float32).reshape(-1, 3)) if k != MARKER}
    out = np.array(fb, np.float32, copy=True).reshape(n_pixels, 3)
    zero = np.float32(0.0)
    with np.errstate(all="ignore"):
        for p in range(n_pixels):
            for c in range(3):
                v = out[p, c]
                for c0 in range(0, n_samples, ACCUM_CHUNK):
                    s = zero
                    for k in range(c0, min(c0 + ACCUM_CHUNK, n_samples)):
                        rec = m.get(p * n_samples + k)
                        s = np.float32(s + (rec[c] if rec is not None else zero))
                    v = np.float32(v + s)
                out[p, c] = v
    return out


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b) -> np.ndarray:
    """Per element: both NaN, or the same bits."""
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    return (np.isnan(a) & np.isnan(b)) | (bits(a) == bits(b))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------

def values(rng, n: int) -> np.ndarray:
    """+-10^U(-5, 5) per component: signed values over ten decades, so that the order and the grouping of the additions show in the sum."""
    mag = 10.0 ** rng.uniform(-5.0, 5.0, (n, 3))
    return (mag * rng.choice([-1.0, 1.0], (n, 3))).astype(np.float32)


def lit_paths(rng, n_pixels: int, n_samples: int, density: float, forced=()) -> np.ndarray:
    """Sorted path indices: every path with probability `density`, plus the `forced` ones."""
    n_paths = n_pixels * n_samples
    lit = np.ones(n_paths, bool) if density >= 1.0 else rng.random(n_paths) < density
    lit[np.asarray(forced, np.int64)] = True
    return np.flatnonzero(lit).astype(np.uint32)


TRIP_COUNTS = (64, 0, 1, 63, 40, 40, 64, 1, 17)     # emitting lanes of the first trips; then random counts in [0, 64]


def interleave(rng, q, rgb, counts=None):
    """The records in the given order spread over trips of 64 items with non-emitting lanes (q = MARKER, rgb = 1e30: it must never show) in between:
    trip t has counts[t] emitting lanes at random places -- TRIP_COUNTS first, then random counts -- until the records are used up."""
    q, rgb = np.asarray(q, np.uint32), np.asarray(rgb, np.float32).reshape(-1, 3)
    n = len(q)
    if counts is None:
        counts = list(TRIP_COUNTS)
        while sum(counts) < n:
            counts.extend(int(c) for c in rng.integers(0, 65, 64))
    counts = np.asarray(counts, np.int64)
    cum = np.cumsum(counts)
    last = int(np.searchsorted(cum, n))                # first trip at which the records run out
    counts = counts[: last + 1].copy()
    counts[last] = n - (cum[last - 1] if last else 0)
    lanes = np.argsort(rng.random((len(counts), 64)), axis=1) < counts[:, None]     # exactly counts[t] lanes of trip t
    emit = lanes.reshape(-1)
    out_q = np.full(emit.size, MARKER, np.uint32)
    out_rgb = np.full((emit.size, 3), 1e30, np.float32)
    out_q[emit], out_rgb[emit] = q, rgb
    return out_q, out_rgb, counts


def make_case(n_pixels: int, n_samples: int, density: float, seed: int, forced=(), only_pixels=None):
    """(q, rgb) of one launch, items shuffled and interleaved with non-emitting lanes.  only_pixels: every record lies in these pixels."""
    rng = np.random.default_rng(seed)
    lit = lit_paths(rng, n_pixels, n_samples, density, forced)
    if only_pixels is not None:
        lit = lit[np.isin(lit // n_samples, np.asarray(only_pixels))]
    rgb = values(rng, len(lit))
    order = rng.permutation(len(lit))
    q, rgb, _ = interleave(rng, lit[order], rgb[order])
    return q, rgb


# The table of the issue: name -> (n_pixels, n_samples, density).  The scan-carry rows and the row with untouched pixels are built by the GPU test.
DENSE_CASES = {
    "1x1": (1, 1, 1.0), "1x8": (1, 8, 1.0), "1x9": (1, 9, 1.0), "3x31": (3, 31, 1.0),
    "255x32": (255, 32, 1.0), "256x32": (256, 32, 1.0), "257x32": (257, 32, 1.0),
    "1000x33": (1000, 33, 0.3),
    "300x512": (300, 512, 1.0),
    "77x544": (77, 544, 0.5),
    "50x1056": (50, 1056, 0.5),
    "64x1024": (64, 1024, 1.0),
}
SPARSE_CASES = {"300x512 sparse": (300, 512, 0.05), "64x1024 sparse": (64, 1024, 0.002)}


def case_seed(name: str) -> int:
    return 1000 + sorted(list(DENSE_CASES) + list(SPARSE_CASES)).index(name)
