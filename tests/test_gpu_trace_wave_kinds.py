"""The FUSED trace launch -- closest-hit rays and shadow rays in one index space, as every bounce after the first makes it -- against the oracle, ray for ray.

hipr_debug_trace_closest / _shadow reach only the launches of one kind; the fused kernel was covered by whole images alone. Its record block treats the two kinds of ray
in branches of their own (csrc/wide8_kernels.h: a record iteration whose lanes all hold one kind issues nothing of the other kind's code), so the cases below are
chosen by what the lanes of a wave hold: waves of one kind, one mixed wave, ragged waves, an empty queue, and launches long enough that waves outlive their shard and
take shadow rays while closest-hit rays are still in flight. Hits as uint32 words, transmittance bit for bit, and -- with instrumentation on, which runs the counting
instantiation of the same code -- the four node / triangle counters against the oracle's sums.
"""
import numpy as np
import pytest

from bifrost3d_amd import capi
from bifrost3d_amd.host import Scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from bifrost3d_amd.renderer import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle_q():
    from oracle_bindings import get_oracle
    return get_oracle(True)   # unorm16 tables, as uploaded to the device


@pytest.fixture(scope="module")
def atrium():
    return Scene("atrium", param0=20000, param1=3)


@pytest.fixture(scope="module")
def textured_atrium():
    """The small textured / cut-out atrium of test_textured_atrium_image_matches_oracle: 30 % of its triangles are not statically opaque -> the COVERAGE instantiation."""
    return Scene("atrium", param0=20000, param1=3, textured=True)


def random_rays(rng, n, lo, hi, tmax=np.inf):
    """tests/test_gpu_parity.py random_rays."""
    o = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = o
    rays[:, 3] = 0.0
    rays[:, 4:7] = d
    rays[:, 7] = tmax
    return rays


def fused_rays(scene, n_closest, n_shadow, with_skip):
    """The recipe of test_the_kernels_the_renderer_runs_return_the_instrumented_kernels_hits, for two queues."""
    # the lone pair of (1, 1) from the seed, of the first forty, whose closest-hit ray finds a surface and whose shadow ray is occluded: both reach records
    rng = np.random.default_rng(30 if (n_closest, n_shadow) == (1, 1) else 1000 * n_closest + n_shadow)
    closest = random_rays(rng, n_closest, -14.0, 14.0)
    closest[:, 1] = np.abs(closest[:, 1]) * 0.7
    skip = np.full(n_closest, 0xFFFFFFFF, np.uint32)
    if with_skip:
        skip[::5] = rng.integers(0, scene.desc.triangle_count, len(skip[::5]))
    shadow = random_rays(rng, n_shadow, -14.0, 14.0)
    shadow[:, 1] = np.abs(shadow[:, 1]) * 0.7
    shadow[:, 7] = rng.uniform(0.05, 30.0, n_shadow).astype(np.float32)
    return closest, skip, shadow


# (scene, closest-hit rays, shadow rays, a triangle to skip on every fifth closest-hit ray)
CASES = [
    ("atrium", 64, 64, False),          # two waves of one kind each
    ("atrium", 33, 31, False),          # one mixed wave
    ("atrium", 1, 1, False),
    ("atrium", 0, 65, False),           # an empty path queue, a ragged wave
    ("atrium", 65, 0, False),           # an empty shadow queue
    ("atrium", 777, 555, False),
    ("atrium", 4113, 4101, False),      # waves outlive their shard and cross from closest-hit to shadow shards with rays in flight
    ("textured", 777, 555, False),      # COVERAGE: shadow rays that meet a cut-out read u and v
    ("atrium", 777, 555, True),
]

_expected = {}      # per case, computed once by the oracle and shared by the runs with and without instrumentation


def expected(oracle_q, search, scene, case):
    if case not in _expected:
        _, n_closest, n_shadow, with_skip = case
        closest, skip, shadow = fused_rays(scene, n_closest, n_shadow, with_skip)
        hits, closest_counts = oracle_q.trace_closest(scene.desc, closest, skip, use_bvh=search, with_lights=True) if n_closest else (np.zeros((0, 4), np.float32), (0, 0))
        transmittance, shadow_counts = oracle_q.trace_shadow(scene.desc, shadow, use_bvh=search) if n_shadow else (np.zeros(0, np.float32), (0, 0))
        for array in (closest, skip, shadow, hits, transmittance):
            array.setflags(write=False)
        _expected[case] = (closest, skip, shadow, hits, transmittance, closest_counts, shadow_counts)
    return _expected[case]


@pytest.mark.parametrize("instrumented", [True, False], ids=["counting", "product"])
@pytest.mark.parametrize("case", CASES, ids=[f"{s}-{c}-{sh}{'-skip' if k else ''}" for s, c, sh, k in CASES])
def test_fused_launch_matches_oracle(ctx, oracle_q, atrium, textured_atrium, case, instrumented):
    scene = textured_atrium if case[0] == "textured" else atrium
    ctx.upload_scene(scene)
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    closest, skip, shadow, hits, transmittance, (nodes, tris), (shadow_nodes, shadow_tris) = expected(oracle_q, ctx.oracle_search(), scene, case)
    ctx.set_instrumentation(instrumented)
    try:
        gpu_hits, gpu_transmittance = ctx.debug_trace_fused(closest, skip, shadow)
        counters = ctx.counters()
    finally:
        ctx.set_instrumentation(False)
    assert np.array_equal(gpu_hits.view(np.uint32), hits.view(np.uint32)), "t, u, v and primitive id must match bit for bit"
    assert np.array_equal(gpu_transmittance.view(np.uint32), transmittance.view(np.uint32))
    if instrumented:
        assert (counters["closest_nodes"], counters["closest_triangles"]) == (nodes, tris)
        assert (counters["shadow_nodes"], counters["shadow_triangles"]) == (shadow_nodes, shadow_tris)
    # the rays exercise what they are meant to: both outcomes of a shadow ray, and closest-hit rays that find a surface (a share of a handful of rays says nothing)
    if len(shadow) >= 31:
        assert 0.05 < (transmittance == 0).mean() < 0.99
    if len(closest) >= 33:
        assert (hits[:, 3].view(np.uint32) != 0xFFFFFFFF).mean() > 0.2
    if len(closest) == 1:
        assert hits[0, 3].view(np.uint32) != 0xFFFFFFFF and transmittance[0] == 0
    if case[0] == "textured":      # the cut-outs are there: the same shadow rays go on through the banners' holes and test more triangles than in the plain atrium
        assert shadow_tris > expected(oracle_q, ctx.oracle_search(), atrium, ("atrium",) + case[1:])[6][1]
