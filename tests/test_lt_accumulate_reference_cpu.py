"""tests/lt_accumulate_reference.py, the numpy restatement of amber_hip_lt_render_pass's definition, against a literal transcription of the loop at the
end of HipLightTracing::Render (no GPU): the GPU tests compare the device with the restatement, these hold the restatement itself."""
import numpy as np

import lt_accumulate_reference as R


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def adapter_loop(rec, width, height, first, n):
    """HipLightTracing::Render's loop over a list sorted (pass, path, bounce): a zeroed image per pass that has records, `image[pixel] += rgb` per
    record, `sum += image` over the whole image."""
    order = sorted(range(len(rec)), key=lambda i: (int(rec["sample"][i]), int(rec["path"][i]), int(rec["bounce"][i])))
    all_ = rec[order]
    total = np.zeros((height, width, 3), np.float32)
    k = 0
    for s in range(first, first + n):
        if k >= len(all_) or all_["sample"][k] != s:
            continue
        image = np.zeros((height, width, 3), np.float32)
        while k < len(all_) and all_["sample"][k] == s:
            px = int(all_["pixel"][k])
            image[px // width, px % width] += all_["rgb"][k]
            k += 1
        total += image
    assert k == len(all_)
    return total


def random_records(rng, n, width, height, first, n_passes):
    rgb = (10.0 ** rng.uniform(-6, 6, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))).astype(np.float32)
    rec = R.records(rng.integers(0, width * height, n), rng.integers(first, first + n_passes, n), rng.integers(1, 5, n),
                    rng.integers(0, width * height, n), rgb)
    key = np.stack([rec["sample"], rec["path"], rec["bounce"]], 1)
    return rec[np.unique(key, axis=0, return_index=True)[1]]          # a (pass, path, bounce) names one record, as in a real list


def test_the_restatement_is_the_adapters_loop():
    rng = np.random.default_rng(1)
    for width, height, n, first, n_passes in ((5, 3, 400, 0, 7), (16, 9, 3000, 11, 40), (1, 1, 200, 5, 3)):
        rec = random_records(rng, n, width, height, first, n_passes)
        assert R.longest_run(rec) >= 2 and len(np.unique(rec["sample"])) >= 2
        assert np.array_equal(bits(R.accumulate(rec, width, height)), bits(adapter_loop(rec, width, height, first, n_passes)))
    assert not R.accumulate(rec[:0], 4, 4).any() and R.longest_run(rec[:0]) == 0


def test_it_adds_to_what_the_framebuffer_holds_and_leaves_the_input_alone():
    rng = np.random.default_rng(2)
    rec = random_records(rng, 500, 6, 4, 0, 9)
    rec = rec[rec["pixel"] % 3 != 0]
    fb = rng.uniform(-3, 3, (4, 6, 3)).astype(np.float32)
    keep = fb.copy()
    got = R.accumulate(rec, 6, 4, fb)
    assert np.array_equal(fb, keep)
    touched = np.zeros(24, bool); touched[rec["pixel"]] = True
    assert np.array_equal(bits(got.reshape(-1, 3)[~touched]), bits(fb.reshape(-1, 3)[~touched])) and (~touched).any()
    a, b = rec[rec["sample"] < 4], rec[rec["sample"] >= 4]            # pass by pass: any split at a pass boundary gives the same bits
    assert np.array_equal(bits(R.accumulate(b, 6, 4, R.accumulate(a, 6, 4, fb))), bits(got))


def test_it_does_not_depend_on_the_order_of_its_input():
    rng = np.random.default_rng(3)
    rec = random_records(rng, 2000, 5, 3, 0, 30)
    want = bits(R.accumulate(rec, 5, 3))
    for _ in range(3):
        assert np.array_equal(bits(R.accumulate(rec[rng.permutation(len(rec))], 5, 3)), want)


def test_the_fixture_shows_a_wrong_order():
    """The one-pixel fixture of the GPU tests: summed in the reverse (path) order it gives other bits, so a device that adds in a wrong order fails."""
    rec = R.one_pixel_fixture(5, 3)
    assert len(rec) == 1 << 17 and len(np.unique(rec["pixel"])) == 1 and len(np.unique(rec["sample"])) == 1 and R.longest_run(rec) == 1 << 17
    assert not np.array_equal(rec["path"], np.sort(rec["path"]))       # given shuffled
    mag = np.abs(rec["rgb"])
    assert mag.min() < 1e-7 and mag.max() > 1e7 and (rec["rgb"] < 0).any() and (rec["rgb"] > 0).any()
    forward = R.accumulate(rec, 5, 3)
    backward = rec.copy()
    backward["path"] = np.uint32((1 << 17) - 1) - rec["path"]
    assert not np.array_equal(bits(forward), bits(R.accumulate(backward, 5, 3)))
    assert np.isfinite(forward).all() and np.count_nonzero(forward) == 3
