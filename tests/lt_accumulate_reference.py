"""amber_hip_lt_render_pass restated in numpy from the text of include/amber_hip.h (not from the device code).

Every operation is binary32 and rounded alone.  The records are ordered by (pass, path, bounce).  For each pass s ascending, P_s starts at +0
everywhere; each record of pass s, in that order, does P_s[pixel].c = P_s[pixel].c + rgb[c]; then fb[p].c = fb[p].c + P_s[p].c for every pixel
that received at least one record in pass s.  All other pixels are untouched.
"""
import numpy as np

SPLAT_DTYPE = np.dtype([("path", np.uint32), ("sample", np.uint32), ("bounce", np.uint32), ("pixel", np.uint32), ("rgb", np.float32, (3,)), ("pad", np.uint32)])


def records(path, sample, bounce, pixel, rgb) -> np.ndarray:
    """A record array of AmberSplat's layout from columns."""
    rec = np.zeros(len(pixel), SPLAT_DTYPE)
    rec["path"], rec["sample"], rec["bounce"], rec["pixel"], rec["rgb"] = path, sample, bounce, pixel, rgb
    return rec


def accumulate(rec: np.ndarray, width: int, height: int, fb=None) -> np.ndarray:
    """fb (height, width, 3) float32 -- zeros if None, never modified -- after the records; one np.float32 addition at a time."""
    out = np.zeros((height, width, 3), np.float32) if fb is None else np.array(fb, np.float32, copy=True).reshape(height, width, 3)
    flat = out.reshape(-1, 3)
    order = np.lexsort((rec["bounce"], rec["path"], rec["sample"]))     # last key is the primary one
    sample, pixel, rgb = rec["sample"][order], rec["pixel"][order], rec["rgb"][order]
    assert (pixel < width * height).all()
    zero = np.float32(0.0)
    k, n = 0, len(order)
    while k < n:
        s = sample[k]
        image = {}                                                     # P_s: pixel -> [r, g, b], created at +0 by the first record
        while k < n and sample[k] == s:
            p = image.setdefault(int(pixel[k]), [zero, zero, zero])
            for c in range(3):
                p[c] = np.float32(p[c] + rgb[k, c])
            k += 1
        for px, p in image.items():
            for c in range(3):
                flat[px, c] = np.float32(flat[px, c] + p[c])
    return out


def longest_run(rec: np.ndarray) -> int:
    """The largest number of records one pixel received in one pass."""
    if len(rec) == 0:
        return 0
    key = (rec["pixel"].astype(np.uint64) << np.uint64(32)) | rec["sample"].astype(np.uint64)
    return int(np.unique(key, return_counts=True)[1].max())


def one_pixel_fixture(width: int, height: int, n: int = 1 << 17, seed: int = 20250) -> np.ndarray:
    """n records on one pixel in one pass: magnitudes 1e-8 ... 1e8, mixed signs, so that the order of the additions shows in the sum; given in
    shuffled order (the path index says where each belongs)."""
    rng = np.random.default_rng(seed)
    mag = (10.0 ** rng.uniform(-8.0, 8.0, (n, 3))).astype(np.float32)
    rgb = (mag * rng.choice(np.float32([-1.0, 1.0]), (n, 3))).astype(np.float32)
    path = rng.permutation(n).astype(np.uint32)
    return records(path, np.full(n, 7, np.uint32), np.full(n, 1, np.uint32), np.full(n, (width * height) // 2, np.uint32), rgb)
