"""tests/temporal_reference.py, the numpy restatement of amber_hip_pt_temporal's contract (include/amber_hip.h), pinned by properties (no GPU).
tests/test_temporal.py holds the device to this restatement bit for bit; here the restatement itself is held to what the contract promises: a static
camera is a running mean, the cap turns it into an exponential blend, an empty history takes the frame as it is, eight frames of noise shrink the error
by sqrt(8), a panned camera finds a plane's colours again, and every one of the rejections resets.

The plane scene: a camera at the origin looking down -z (global_ = a rotation about y, sensor distance 0.05, a 64 x 48 sensor 0.036 wide) at the plane
z = -2; the depth of a pixel is the binary64 distance from the lens origin to the plane along the pixel's chief ray, narrowed to binary32."""
import numpy as np
import pytest

import temporal_reference as T

F32 = np.float32
W, H = 64, 48
SENSOR = (W, H, F32(0.036), F32(0.036 / W * H))
SD, DIST = 0.05, 2.0
PIXEL = float(np.arctan(0.036 / W / SD))                                        # the pan that moves the image centre by one pixel
U = 2.0 ** -24


def rot_y(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def lens(angle=0.0, origin=(0.0, 0.0, 0.0)):
    return T.make_lens(origin, rot_y(angle), SD)


def plane_points(L, dist=DIST):
    """binary64: the world point where every pixel's chief ray meets the plane z = -dist, and its distance from the lens origin"""
    y, x = np.mgrid[0:H, 0:W]
    s = np.stack([((x + 0.5) / W - 0.5) * float(SENSOR[2]), ((y + 0.5) / H - 0.5) * float(SENSOR[3]), np.full((H, W), float(L.sensor_distance))], -1)
    g = -(s @ L.global_.astype(np.float64).reshape(3, 3).T)
    g = g / np.linalg.norm(g, axis=-1, keepdims=True)
    o = L.origin.astype(np.float64)
    t = (-dist - o[2]) / g[..., 2]
    return o + t[..., None] * g, t


def aov_of(depth, albedo=(0.7, 0.7, 0.7), normal=(0.0, 0.0, 1.0), cov=None, count=2):
    cov = np.full((H, W), count, F32) if cov is None else cov.astype(F32)
    a = np.zeros((H, W, 8), F32)
    a[..., 0:3] = F32(albedo) * cov[..., None]
    a[..., 3] = np.asarray(depth, F32) * cov
    a[..., 4:7] = F32(normal) * cov[..., None]
    a[..., 7] = cov
    return a


def texture(P):
    return np.stack([0.5 + 0.3 * np.sin(2 * P[..., 0]) + 0.2 * np.cos(3 * P[..., 1])] * 3, -1)


def frame(L, dist=DIST, **kw):
    P, t = plane_points(L, dist)
    return texture(P).astype(F32), aov_of(t, **kw), P


def run(frames, **kw):
    """frames: (colour, aov, lens); levels = 0.  Returns the states and infos after every frame"""
    state, out = T.empty_state(H, W), []
    for c, aov, L in frames:
        _, state, info = T.temporal(state, c, aov, 1, L, SENSOR, levels=0, **kw)
        out.append((state, info))
    return out


# ---- a static camera ---------------------------------------------------------------------------------------------------------------------------
def test_an_unchanged_lens_is_a_running_mean():
    """Bound: one blend h + (x - h) * (1 / j) rounds four times; with every value within M its error is at most u * M * (1 + 6 / j) <= 7 u M
    (u = 2^-24: x - h is within 2 M, the reciprocal and the product add 2 u of 2 M / j each way, the sum u M), and an error already in h is carried
    on with the factor 1 - 1 / j <= 1: after k blends at most 7 k u M."""
    rng = np.random.default_rng(1)
    k, L = 8, lens()
    _, aov, _ = frame(L)
    cs = [rng.uniform(0, 2, (H, W, 3)).astype(F32) for _ in range(k)]
    res = run([(c, aov, L) for c in cs], max_history=k)
    for j, (state, info) in enumerate(res, 1):
        assert (state["hist"][..., 3] == j).all() and info["kept"].all() == (j > 1) and info["kept"].any() == (j > 1)
        mean = np.mean(np.stack(cs[:j]).astype(np.float64), axis=0)
        assert np.abs(state["hist"][..., :3] - mean).max() <= 7 * j * U * 2.0
        assert (state["hist"][..., 6:] == 0).all()
    y = [T.lum(c).astype(np.float64) for c in cs]
    assert np.abs(res[-1][0]["hist"][..., 4] - np.mean(y, axis=0)).max() <= 7 * k * U * 2.0
    assert np.abs(res[-1][0]["hist"][..., 5] - np.mean(np.square(y), axis=0)).max() <= 7 * k * U * 4.0 + 4 * U * 4.0      # (Y * Y rounds once more)


def test_the_cap_makes_the_blend_exponential():
    rng = np.random.default_rng(2)
    L = lens()
    _, aov, _ = frame(L)
    cs = [rng.uniform(0, 2, (H, W, 3)).astype(F32) for _ in range(7)]
    res = run([(c, aov, L) for c in cs], max_history=4)
    assert [float(s["hist"][0, 0, 3]) for s, _ in res] == [1, 2, 3, 4, 4, 4, 4]
    for j in range(4, 7):                                                        # from the fifth frame on alpha stays 1/4
        old, new = res[j - 1][0]["hist"], res[j][0]["hist"]
        assert (new[..., 3] == 4).all()
        want = old[..., :3] + (cs[j] - old[..., :3]) * F32(0.25)
        assert want.dtype == F32 and np.array_equal(new[..., :3].view(np.uint32), want.view(np.uint32))


def test_an_empty_and_a_reset_history_take_the_frame_as_it_is():
    rng = np.random.default_rng(3)
    L = lens()
    _, aov, _ = frame(L)
    fb = rng.uniform(0, 8, (H, W, 3)).astype(F32)
    c = fb / F32(4)
    Y = T.lum(c)
    out, state, info = T.temporal(T.empty_state(H, W), fb, aov, 4, L, SENSOR, levels=0)
    for s, o in ((state, out), ):
        assert np.array_equal(s["hist"][..., :3].view(np.uint32), c.view(np.uint32)) and np.array_equal(o.view(np.uint32), c.view(np.uint32))
        assert (s["hist"][..., 3] == 1).all() and np.array_equal(s["hist"][..., 4], Y) and np.array_equal(s["hist"][..., 5], Y * Y) and not info["kept"].any()
    _, state, _ = T.temporal(state, fb, aov, 4, L, SENSOR, levels=0)
    assert (state["hist"][..., 3] == 2).all()
    emptied = T.reset(state)
    assert not emptied["hist"].any() and emptied["empty"]
    other = rng.uniform(0, 8, (H, W, 3)).astype(F32)
    _, again, info = T.temporal(emptied, other, aov, 4, L, SENSOR, levels=0)
    _, first, _ = T.temporal(T.empty_state(H, W), other, aov, 4, L, SENSOR, levels=0)
    assert np.array_equal(again["hist"].view(np.uint32), first["hist"].view(np.uint32)) and (again["hist"][..., 3] == 1).all() and not info["kept"].any()


def test_eight_frames_of_noise_shrink_the_error_by_the_root_of_eight():
    """Independent noise of variance s^2: the mean of 8 frames has s^2 / 8, so the RMSE ratio is 0.354 in expectation.  Over 64 x 48 x 3 = 9216 values
    a sample RMSE has a relative spread of 1 / sqrt(2 * 9216) = 0.7 %, so the ratio of two of them stays within a few per cent of 0.354: < 0.45."""
    rng = np.random.default_rng(4)
    L = lens()
    _, aov, _ = frame(L)
    truth = F32([0.6, 0.4, 0.2])
    cs = [(truth + rng.normal(0, 0.2, (H, W, 3))).astype(F32) for _ in range(8)]
    res = run([(c, aov, L) for c in cs])
    rmse = lambda img: float(np.sqrt(np.mean((img.astype(np.float64) - truth) ** 2)))
    ratio = rmse(res[-1][0]["hist"][..., :3]) / rmse(cs[-1])
    assert 0.30 < ratio < 0.45, ratio


# ---- a moved camera ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pixels", [0.3, 1.0, 2.6])
def test_a_pan_finds_the_planes_colours_again(pixels):
    """The previous frame's colour is texture(world point).  With this frame black the blend is h + (0 - h) * (1 / 2) = h / 2 exactly, so twice the new
    history is the reprojected colour h.  Where all four taps were accepted h is a bilinear interpolation of the texture over one previous pixel, whose
    footprint on the plane is at most 1.3 * DIST * 0.036 / W / SD wide (1 / cos^2 of the corner's angle is 1.2, the pan adds a little): the error is
    at most footprint^2 / 8 * (|f_xx| + |f_yy|) = footprint^2 / 8 * (1.2 + 1.8), plus the texture's gradient (<= 0.85) times what a position error of
    1e-3 pixel -- far more than binary32 leaves of a coordinate below 64 -- moves the point."""
    A, B = lens(0.0), lens(pixels * PIXEL)
    cA, aovA, _ = frame(A)
    _, aovB, PB = frame(B)
    (_, _), (state, info) = run([(cA, aovA, A), (np.zeros((H, W, 3), F32), aovB, B)])
    assert info["moved"]
    full = info["taps"] == 4
    assert full.mean() > 0.85 and info["kept"].mean() > 0.9 and (state["hist"][..., 3][info["kept"]] == 2).all()
    if pixels != 1.0:
        assert info["fractional"].mean() > 0.85
    h = 2.0 * state["hist"][..., :3].astype(np.float64)
    footprint = 1.3 * DIST * 0.036 / W / SD
    tol = footprint ** 2 / 8 * 3.0 + 0.85 * 1e-3 * footprint
    assert np.abs(h - texture(PB))[full].max() <= tol
    lost = ~info["kept"]                                                        # from one pixel at the centre (more at the edge) the columns that came into view have nothing to reproject
    assert lost.any() == (pixels >= 1) and (state["hist"][..., 3][lost] == 1).all() and lost[:, W // 2].sum() == 0


def two_frames(second, same, first=None, **kw):
    A = lens(0.0)
    B = A if same else lens(0.4 * PIXEL)
    cA, aovA, _ = frame(A, **(first or {}))
    cB, aovB, _ = frame(B, **second)
    (_, _), (state, info) = run([(cA, aovA, A), (cB, aovB, B)], **kw)
    assert info["moved"] == (not same)
    return state, info


@pytest.mark.parametrize("same", [True, False], ids=["same lens", "pan"])
def test_rejections(same):
    inner = np.zeros((H, W), bool)
    inner[2:-2, 2:-2] = True
    state, info = two_frames({}, same)                                          # the control: nothing changed, (nearly) everything kept
    assert info["kept"][inner].all() and (state["hist"][..., 3][inner] == 2).all()
    state, info = two_frames(dict(dist=DIST * 1.05), same)                      # 5 % deeper: within 1 / k_depth = 10 %
    assert info["kept"][inner].all()
    for what, change in {"15 % deeper": dict(dist=DIST * 1.15), "15 % nearer": dict(dist=DIST * 0.85), "a turned normal": dict(normal=(0.6, 0.0, 0.8)),
                         "another albedo": dict(albedo=(0.5, 0.5, 0.5))}.items():
        state, info = two_frames(change, same)
        assert not info["kept"].any() and (state["hist"][..., 3] == 1).all(), what
    state, info = two_frames(dict(dist=DIST * 1.15), same, k_depth=5.0)          # the stop is this call's k_depth
    assert info["kept"][inner].all()
    state, info = two_frames(dict(normal=(0.6, 0.0, 0.8), albedo=(0.5, 0.5, 0.5)), same, k_normal=0.0, k_albedo=0.0)
    assert info["kept"][inner].all()


def test_a_camera_turned_away_resets():
    A, B = lens(0.0), lens(np.pi)
    cA, aovA, _ = frame(A)
    (_, _), (state, info) = run([(cA, aovA, A), (cA, aovA, B)])                  # the guides would all pass: dl.z >= 0 alone rejects
    assert info["moved"] and not info["kept"].any() and (state["hist"][..., 3] == 1).all()
    assert np.array_equal(state["hist"][..., :3].view(np.uint32), cA.view(np.uint32))


@pytest.mark.parametrize("same", [True, False], ids=["same lens", "pan"])
def test_a_nan_depth_resets_that_pixel(same):
    A = lens(0.0)
    B = A if same else lens(0.4 * PIXEL)
    cA, aovA, _ = frame(A)
    cB, aovB, _ = frame(B)
    bad = np.zeros((H, W), bool)
    bad[10:20, 30:40] = True
    aovB[bad, 3] = np.nan
    (_, _), (state, info) = run([(cA, aovA, A), (cB, aovB, B)])
    assert not info["kept"][bad].any() and (state["hist"][..., 3][bad] == 1).all() and np.isfinite(state["hist"]).all()
    assert info["kept"][~bad].mean() > 0.9
    # ... and a NaN depth in the previous guide (rz' = 0: no coverage) rejects every tap that reads it
    (_, _), (state, info) = run([(cA, aov_nan(A, bad), A), (cB, frame(B)[1], B)])
    assert not info["kept"][12:18, 32:38].any() and np.isfinite(state["hist"]).all() and info["kept"][~bad].mean() > 0.85


def aov_nan(L, bad):
    aov = frame(L)[1]
    aov[bad, 3] = np.nan
    return aov


def test_coverage_zero():
    """lens unchanged: a background pixel keeps its history iff it was background before; a pixel that is hit now and was background before starts again.
    lens changed: every background pixel starts again."""
    rng = np.random.default_rng(6)
    A = lens(0.0)
    before, now = np.ones((H, W)), np.ones((H, W))
    before[:, :24] = 0
    now[:, 16:40] = 0                                                          # background now: columns 16..39; background before: 0..23
    _, t = plane_points(A)
    c1, c2 = rng.uniform(0, 1, (H, W, 3)).astype(F32), rng.uniform(0, 1, (H, W, 3)).astype(F32)
    (_, _), (state, info) = run([(c1, aov_of(t, cov=before), A), (c2, aov_of(t, cov=now), A)])
    n = state["hist"][..., 3]
    assert (n[:, 16:24] == 2).all() and (n[:, 24:40] == 1).all()                # background twice / hit before
    assert (n[:, :16] == 1).all() and (n[:, 40:] == 2).all()                    # background before, hit now / hit twice
    assert np.array_equal(info["kept"], n == 2)
    B = lens(0.4 * PIXEL)
    (_, _), (state, info) = run([(c1, aov_of(t, cov=before), A), (c2, aov_of(plane_points(B)[1], cov=now), B)])
    n = state["hist"][..., 3]
    assert (n[:, 16:40] == 1).all() and (n[:, :16] == 1).all() and (n[2:-2, 42:-2] == 2).all()
