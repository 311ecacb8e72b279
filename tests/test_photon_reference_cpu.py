"""tests/photon_reference.py is pinned to the pinned oracle (no GPU needed): the walker that restates amber_hip_lt_trace_photons from the oracle's
exported stages must reproduce oracle_render_lt_xorshift -- its Eye vertices, through oracle_lens_responses and weight * value / (W * H), are that
function's splat records bit for bit, in number and order, and its casts are that function's casts -- with the handle's default depth and with
max_depth = 3.  The scene must also give the GPU tests what they need: vertices of every material kind, and long paths."""
import numpy as np
import pytest

import photon_reference as P


@pytest.mark.parametrize("max_depth", [0, 3])
def test_the_walker_is_the_oracles_light_tracer(max_depth):
    walker, rec = P.reference(max_depth)
    got, n_eye = P.splats_of(walker, rec, P.W, P.H, P.SCALE)
    want, casts = P.oracle_splats(walker.osc, P.W, P.H, P.SCALE, P.SEED, 0, P.PASSES, max_depth)
    print(f"max_depth {max_depth}: {walker.casts} casts, {len(rec)} vertices, {len(got)} records from {n_eye} Eye vertices; the oracle: {casts} casts, {len(want)} records")
    assert walker.casts == casts
    assert got.shape == want.shape and np.array_equal(got, want)
    assert len(want) >= 1
    if max_depth:
        assert rec["bounce"].max() == max_depth


def test_the_scene_gives_the_vertices_the_cases_need():
    walker, rec = P.reference(0)
    kinds = walker.kinds(rec)
    counts = np.bincount(kinds, minlength=6)
    longest = np.bincount((rec["sample"].astype(np.uint64) * np.uint64(P.W * P.H) + rec["path"]).astype(np.int64)).max()
    print(f"vertices by kind (Lambertian, Phong, Specular, Refraction, Light, Eye): {counts.tolist()}; the longest path has {longest} vertices")
    assert (counts >= 20).all(), counts
    assert longest >= 8
    order = np.lexsort((rec["bounce"], rec["path"], rec["sample"]))
    assert np.array_equal(order, np.arange(len(rec)))
    # masks partition the list
    parts = [P.select_len(walker, rec, m) for m in (P.DIFFUSE, P.SPECULAR, P.LIGHT, P.EYE)]
    assert sum(parts) == len(rec) and parts == [counts[0] + counts[1], counts[2] + counts[3], counts[4], counts[5]]
