"""amber_hip_pt_trace_paths / amber_hip_sampler_state, the part that needs no GPU: the layout of the two structs, the export lists, and
amber_hip_sampler_state (host arithmetic only) against a literal Python restatement of DESIGN.md section 4 -- SplitMix64 of the seed, SplitMix64 of
that xor (pixel << 32 | sample), 0 replaced by the golden-ratio constant."""
import ctypes

import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def splitmix64(z):
    z = (z + GOLDEN) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sampler_state(seed, pixel, sample):
    s = splitmix64(splitmix64(seed) ^ ((pixel << 32) | sample))
    return s if s else GOLDEN


def test_struct_layouts(amber):
    assert ctypes.sizeof(amber.PathRay) == 64 and ctypes.sizeof(amber.PathResult) == 32
    assert amber.api._PATH_RAY.itemsize == 64 and amber.api._PATH_RESULT.itemsize == 32
    for name, off in (("origin", 0), ("dir", 16), ("weight", 32), ("rng_state", 48), ("pad3", 56)):
        assert getattr(amber.PathRay, name).offset == off == amber.api._PATH_RAY.fields[name][1], name
    for name, off in (("rgb", 0), ("casts", 12), ("rng_state", 16), ("pad", 24)):
        assert getattr(amber.PathResult, name).offset == off == amber.api._PATH_RESULT.fields[name][1], name


def test_symbols_are_product_abi(amber):
    from amber_amd.api import ABI_SYMBOLS, LAB_SYMBOLS
    lib = amber.load_library()
    for s in ("amber_hip_pt_trace_paths", "amber_hip_sampler_state"):
        assert s in ABI_SYMBOLS and s not in LAB_SYMBOLS and hasattr(lib, s), s
    assert lib.amber_hip_abi_version() == 3


def test_sampler_state_is_the_render_kernels_seed(amber):
    rng = np.random.default_rng(5)
    edge = [0, 1, 2, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff]
    seeds = [0, 1, 12345, M64, 1 << 63, GOLDEN, (-GOLDEN) & M64] + [int(x) for x in rng.integers(0, 1 << 63, 8)]
    triples = [(s, p, q) for s in seeds[:7] for p in edge for q in edge]
    triples += [(int(rng.choice(seeds)), int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))) for _ in range(300)]
    assert len(triples) > 500
    for seed, pixel, sample in triples:
        got = amber.sampler_state(seed, pixel, sample)
        assert got == sampler_state(seed, pixel, sample) and got != 0, (seed, pixel, sample, got)
    # the vectorised form trace_paths uses for its default states: the same numbers
    for seed in seeds:
        px, sm = np.array([t[1] for t in triples], np.uint32), np.array([t[2] for t in triples], np.uint32)
        want = np.array([sampler_state(seed, int(p), int(q)) for p, q in zip(px, sm)], np.uint64)
        assert np.array_equal(amber.sampler_states(seed, px, sm), want), seed
