"""pt_megakernel reads its COLD kernel arguments from the kernarg segment next to their use (pt_args.h, ColdArgs): the queue, what places a
primary round's 64 paths in the frame (samples, seed, rows, stripes, sensor, lens, blades, pixel masks), the record buffers and the carried
measurements.  A field read at a wrong offset shows as a wrong pixel, a wrong seed or a lost record, so every case here compares image bits
and the ray count of the two-phase engine (and of engine LIST with the same handle parameters) with the oracle, at the smallest shapes that
exercise each group of fields:

  * the Cornell box, 40 x 48;
  * the row band 8..40, dealt as stripes of 8 rows with period 16 and as contiguous rows (row_begin, stripe_rows, stripe_period);
  * two launches of 37 and 27 samples: first_sample is non-zero, n_samples is no multiple of 64, so primary rounds straddle pixels;
  * the same through a pinhole lens (the Cornell box's objects behind HostScene.create with n_blades = 0);
  * a fuzz scene in which 15 % of the paths reach a light: a wave's 1024 claimed paths give some 150 records, more than two blocks of
    AMBER_REC_BLOCK = 64 slots (EmitRecords: records, flags, touched, rec_count, rec_capacity).
"""
import numpy as np
import pytest

import oracle_binding as O
from fuzz_scenes import scene_for_seed

pytestmark = pytest.mark.gpu

W, H, SEED = 40, 48, 4242


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cornell_kwargs(amber):
    """The Cornell box's objects, materials and camera as HostScene.create / oracle Scene.create take them (without the aperture blades)."""
    objs, mats, lens = amber.HostScene.cornell_box().flatten()
    n_params = {0: 9, 1: 4, 2: 7, 3: 8}
    objects = [(o.kind, o.material, [float(v) for v in o.p[:n_params[o.kind]]]) for o in list(objs)[lens.n_blades:]]
    materials = [(m.kind, tuple(float(x) for x in m.rho[:]), float(m.param)) for m in mats]
    g, o = np.array(lens.global_[:], np.float32).reshape(3, 3), np.array(lens.origin[:], np.float32)
    transform = [float(x) for r in range(3) for x in (*g[r], o[r])] + [0.0, 0.0, 0.0, 1.0]
    return dict(objects=objects, materials=materials, transform=transform, focal_length=0.05, focus_distance=float(lens.focus_distance), radius=0.05)


_scenes = {}


def _scene(amber, name):
    """(host scene, oracle scene with the List acceleration), made once per name."""
    if name not in _scenes:
        if name == "cornell":
            _scenes[name] = (amber.HostScene.cornell_box(), O.Scene.cornell(O.ACCEL_LIST))
        elif name == "pinhole":
            kw = dict(_cornell_kwargs(amber), n_blades=0)
            _scenes[name] = (amber.HostScene.create(**kw), O.Scene.create(**kw))
        else:
            kw, _ = scene_for_seed(FUZZ_SEED)
            assert len(kw["objects"]) + kw["n_blades"] <= 32                 # the 32-object two-phase engine
            _scenes[name] = (amber.HostScene.create(**kw), O.Scene.create(**kw))
    return _scenes[name]


def _check(amber, name, launches, rows=None, stripe=None):
    hs, osc = _scene(amber, name)
    got = {}
    for engine in (amber.ENGINE_TWO_PHASE, amber.ENGINE_LIST):
        pt = amber.PathTracer(hs, amber.Sensor.default(W, H), seed=SEED, rows=rows, stripe=stripe, engine=engine)
        for first, n in launches:
            pt.render_pass(first, n)
        img, rays = pt.download()
        index = pt.row_index
        pt.close()
        got[engine] = (bits(img).copy(), rays)
    full = np.zeros((H, W, 3), np.float32)
    casts = 0
    y = 0
    while y < len(index):                                                    # the oracle renders every contiguous run of the handle's rows
        z = y
        while z + 1 < len(index) and index[z + 1] == index[z] + 1:
            z += 1
        for first, n in launches:                                            # chunk sums added launch after launch, as the engine does
            _, cnt = osc.render_xorshift(W, H, SEED, first, n, rows=(int(index[y]), int(index[z]) + 1), out=full)
            casts += cnt.casts
        y = z + 1
    for engine, (img_bits, rays) in got.items():
        assert rays == casts, (name, engine, rays, casts)
        assert np.array_equal(img_bits, bits(full[index])), (name, engine)
    return full, casts


def test_cornell_40x48(amber):
    full, casts = _check(amber, "cornell", [(0, 64)])
    assert casts > W * H * 64 and (bits(full) != 0).any()                    # paths bounce, and some reach the light


@pytest.mark.parametrize("stripe", [(8, 16), None], ids=["stripes", "contiguous"])
def test_row_band(amber, stripe):
    """Rows 8..40: as stripes the handle owns rows 8..15 and 24..31, contiguous all 32."""
    _check(amber, "cornell", [(0, 32)], rows=(8, 40), stripe=stripe)


@pytest.mark.parametrize("scene", ["cornell", "pinhole"])
def test_two_launches_of_37_and_27_samples(amber, scene):
    _check(amber, scene, [(0, 37), (37, 27)])


FUZZ_SEED = 910_006


def test_many_records_per_wave(amber):
    """fuzz_scenes.scene_for_seed(910006): 26 objects and six blades.  The share of paths that end on a light is counted on the oracle's
    single-sample images first: with 1024 paths per claim it must fill more than two record blocks per wave."""
    _, osc = _scene(amber, "fuzz")
    lit = sum(int((bits(osc.render_xorshift(W, H, SEED, k, 1)[0]) != 0).any(axis=2).sum()) for k in range(4))
    assert lit / (4 * W * H) * 1024 > 2 * 64, lit
    _check(amber, "fuzz", [(0, 64)])
