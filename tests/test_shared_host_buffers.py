"""What one pair of staging buffers and one index sort per handle could break: every call that takes host pointers through device memory (cast_rays,
occluded, trace_paths, lt_trace_photons, pm_build, pm_gather -- numpy modes throughout) and every call that sorts (lt_render_pass, lt_trace_photons,
pm_build) answers, interleaved with the others on ONE handle, the bytes it answers alone on a fresh handle.  The Cornell box at 32 x 32, seed fixed.
Also: a large call followed by a small one (a stale size or stride in the trip driver), pm_release (which frees the staging) followed by a query, and
the lab's three stage clocks switched on together on one handle, since they time stages that share the one sort."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F = np.float32
SIZE, SEED = 32, 77
INFO_KEYS = ("n_photons", "n_dropped", "dims", "n_doublings", "max_cell_count", "cell_size", "lo", "hi")     # (build_ms is a host clock)


def raw(x):
    """The bytes of an answer: arrays, scalars, dicts and tuples of them."""
    if isinstance(x, dict):
        return tuple((k, raw(v)) for k, v in sorted(x.items()))
    if isinstance(x, (tuple, list)):
        return tuple(raw(v) for v in x)
    return np.ascontiguousarray(x).tobytes() if isinstance(x, np.ndarray) else x


class Work:
    """The handle factory, the inputs and every call's stand-alone answer: made once, left unchanged."""

    def __init__(self, amber):
        self.amber, self.hs = amber, amber.HostScene.cornell_box()
        pt = self.fresh()
        i = np.arange(4097)
        eye = pt.kat_eye(i % (SIZE * SIZE), i // (SIZE * SIZE))              # the eye rays of the frame, four samples and one ray more
        self.o, self.d = eye[:, 0:3].copy(), eye[:, 3:6].copy()
        photons, _ = pt.lt_trace_photons(0, 1)
        pt.close()
        assert len(photons) > 1000
        extent = float((photons["pos"].max(axis=0) - photons["pos"].min(axis=0)).max())
        self.cell = extent / 16
        at = photons[:: len(photons) // 130][:130]                            # queries on the surfaces, where the photons are
        q = np.zeros(130, amber.api.GATHER_QUERY_DTYPE)
        q["pos"], q["normal"], q["object"], q["dir_out"], q["weight"] = at["pos"], at["normal"], at["object"], at["dir_out"], (1, 0.5, 0.25)
        q["radius"] = (extent * (0.05 + 0.15 * np.random.default_rng(3).random(130))).astype(F)
        self.q = q
        for self.lt_passes in (16, 64, 256, 1024, 4096):                      # the box splats rarely: enough passes in the one call for the sorts to have work
            pt = self.fresh()
            n_splats = len(pt.lt_trace(0, self.lt_passes)[0])
            pt.close()
            if n_splats >= 16:
                break
        for a in (self.o, self.d, self.q):
            a.setflags(write=False)
        self.ops = {
            "cast": lambda pt: pt.cast_rays(self.o[:257], self.d[:257]),
            "occluded": lambda pt: pt.occluded(self.o[:257], self.d[:257], 2.0),
            "paths": lambda pt: pt.trace_paths(self.o[:257], self.d[:257], n_samples=2),
            "photons": lambda pt: pt.lt_trace_photons(0, 1),
            "map": self.map_and_gathers,
            "lt": self.lt_pass,
            "cast_4097": lambda pt: pt.cast_rays(self.o, self.d),
            "cast_3": lambda pt: pt.cast_rays(self.o[:3], self.d[:3]),
            "gather_1": lambda pt: self.map_and_gathers(pt, n=1),
        }
        self.want = {}
        for name, op in self.ops.items():
            pt = self.fresh()
            self.want[name] = raw(op(pt))
            pt.close()

    def fresh(self):
        return self.amber.PathTracer(self.hs, self.amber.Sensor.default(SIZE, SIZE), seed=SEED)

    def map_and_gathers(self, pt, n=130):
        photons, _ = pt.lt_trace_photons(0, 1)
        info = pt.pm_build(photons, self.cell)
        return {k: info[k] for k in INFO_KEYS}, pt.pm_gather(self.q[:n], k=0), pt.pm_gather(self.q[:n], k=7)

    def lt_pass(self, pt):
        pt.clear()                                                            # the framebuffer and the ray counter as a fresh handle has them
        info = pt.lt_render_pass(0, self.lt_passes)
        return info, pt.download()

    def run(self, pt, names):
        for name in names:
            assert raw(self.ops[name](pt)) == self.want[name], name


_work = {}


@pytest.fixture(scope="module")
def W(amber):
    if "w" not in _work:
        _work["w"] = Work(amber)
    return _work["w"]


def test_the_stand_alone_answers_are_not_trivial(W):
    pt = W.fresh()
    obj, t, _, _ = W.ops["cast"](pt)
    assert (obj >= 0).sum() > 200 and np.isfinite(t[obj >= 0]).all()
    _, g0, g7 = W.map_and_gathers(pt)
    assert (g0["n_in_radius"] > 7).sum() > 30 and (g7["n_used"] == 7).sum() > 30 and (g0["n_in_radius"] <= 7).any() and (g0["rgb"] > 0).any()   # both paths of the gather
    info, (img, rays) = W.lt_pass(pt)
    assert info["n_splats"] >= 16 and rays == info["n_rays"] > 0 and img.any()
    pt.close()
    assert W.want["cast_3"] != W.want["cast"] and W.want["gather_1"] != W.want["map"]


@pytest.mark.parametrize("order", [("cast", "occluded", "paths", "photons", "map", "lt"), ("lt", "map", "paths", "photons", "occluded", "cast")],
                         ids=["queries_first", "sorts_first"])
def test_every_call_interleaved_on_one_handle_answers_as_alone(W, order):
    pt = W.fresh()
    W.run(pt, order + order)
    pt.close()


def test_a_small_call_after_a_large_one(W):
    pt = W.fresh()
    W.run(pt, ("cast_4097", "cast_3", "map", "gather_1", "cast_4097", "occluded"))
    pt.close()


def test_released_staging_regrows(W):
    pt = W.fresh()
    W.run(pt, ("cast", "map"))
    pt.pm_release()
    W.run(pt, ("cast", "paths", "map", "occluded"))
    pt.pm_release(); pt.pm_release()
    W.run(pt, ("cast_3", "cast_4097"))
    pt.close()


def test_the_three_stage_clocks_on_one_handle(W, amber):
    """What test_photon_map.py asserts for its hook, with all three clocks on: each reports positive times for its own stages, then zeros."""
    assert amber.is_lab()
    pt = W.fresh()
    assert pt.kat_lt_stage_ms() == (0.0, 0.0) and pt.kat_photon_stage_ms() == (0.0, 0.0, 0.0) and pt.kat_pm_stage_ms() == (0.0, 0.0)    # switched on
    W.run(pt, ("lt", "photons", "map", "lt"))                                 # (timed stages answer the same bytes)
    lt, photon, pm = pt.kat_lt_stage_ms(), pt.kat_photon_stage_ms(), pt.kat_pm_stage_ms()
    assert all(ms > 0 for ms in lt + photon + pm), (lt, photon, pm)
    assert pt.kat_lt_stage_ms() == (0.0, 0.0) and pt.kat_photon_stage_ms() == (0.0, 0.0, 0.0) and pt.kat_pm_stage_ms() == (0.0, 0.0)
    W.run(pt, ("photons",))                                                   # only the photon stages ran: the other clocks stay at zero
    assert all(ms > 0 for ms in pt.kat_photon_stage_ms()) and pt.kat_lt_stage_ms() == (0.0, 0.0) and pt.kat_pm_stage_ms() == (0.0, 0.0)
    pt.close()
