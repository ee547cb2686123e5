"""The refill ROUND of the 8-wide trace kernel (csrc/wide8_kernels.h) and the bookkeeping around its two blocks, against the oracle bit for bit.

A round retires the wave's finished rays and hands its idle lanes new ones, and it issues every load of both before it waits for any: the radiance a retiring shadow
ray adds to, the queue entries of the new rays, the scene's one analytic light. What a lane does is carried in one word (a node's slot, a record's slot, finished,
idle) from which the wave takes its votes. Neither changes a ray's arithmetic or its order of items, so everything here is compared exactly -- hits as uint32 words,
transmittances bit for bit, the node / triangle counters of the counting instantiations against the oracle's sums, an exact-mode frame against the oracle's f64 mean:
  * ragged fused launches (lanes that retire a closest-hit ray and take a shadow ray, either queue empty, triangles to skip),
  * rays chosen for the bookkeeping (every octant, axis-parallel directions with components of either zero, rays that miss the root, shadow rays that end before the
    first box or on the first triangle they meet),
  * the light lists the retire step tells apart (none analytic, one, a sphere of radius 0 beside a live one, a spot light, two analytic lights: one more than it
    fetches ahead),
  * one small render whose shadow rays add to radiance slots while new rays are loaded.
"""
import ctypes as C

import numpy as np
import pytest

from bifrost3d_amd import capi
from bifrost3d_amd.host import Scene

pytestmark = pytest.mark.gpu

LIGHT_SPHERE, LIGHT_DIRECTIONAL, LIGHT_SPOT = 1, 2, 5      # include/hiprenderer_c.h HIPR_LIGHT_*
MISS = 0xFFFFFFFF
LIGHT_HIT = 0x80000000


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
    """The 20 k-triangle atrium of tests/test_gpu_parity.py: the 8-wide tree, a directional light and a sphere light."""
    return Scene("atrium", param0=20000, param1=3)


class Relit:
    """A scene with another list of lights: what Context.upload_scene and the oracle read of a Scene, over a copy of its description."""

    def __init__(self, scene, lights):
        self.scene = scene
        self.lights = (capi.HiprLight * max(len(lights), 1))(*lights)
        self._desc = capi.HiprSceneDesc.from_buffer_copy(scene.desc)
        self._desc.lights = C.cast(self.lights, C.POINTER(capi.HiprLight))
        self._desc.light_count = len(lights)

    @property
    def desc(self):
        return self._desc

    @property
    def state(self):
        return self.scene.state

    def camera(self, *args, **kwargs):
        return self.scene.camera(*args, **kwargs)


def light(kind, position=(0, 0, 0), radius=0.0, direction=(0, -1, 0), cos_angle=0.8):
    l = capi.HiprLight()
    l.data[0:3] = [10.0, 9.0, 8.0]
    if kind == LIGHT_DIRECTIONAL:
        l.data[3:6] = list(direction)
    else:
        l.data[3:6] = list(position)
        l.data[6] = radius
        l.data[7:10] = list(direction)
        l.data[10] = cos_angle
    l.flags = kind
    return l


def rays_of(origins, directions, tmin=0.0, tmax=np.inf):
    rays = np.zeros((len(origins), 8), np.float32)
    rays[:, 0:3] = origins
    rays[:, 3] = tmin
    rays[:, 4:7] = directions
    rays[:, 7] = tmax
    return rays


def random_rays(rng, n, lo, hi):
    """tests/test_gpu_parity.py random_rays, kept inside the atrium's hall."""
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    rays = rays_of(rng.uniform(lo, hi, size=(n, 3)).astype(np.float32), d)
    rays[:, 1] = np.abs(rays[:, 1]) * 0.7
    return rays


def resident(ctx, scene):
    """Uploads the scene unless it is the one the context holds already (the cases of this file share two contexts and mostly one scene)."""
    if getattr(ctx, "_scene", None) is not scene:
        ctx.upload_scene(scene)
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT


def fused(ctx, oracle_q, scene, closest, skip, shadow, instrumented, expected=None):
    """One fused launch, product or counting instantiation, against the oracle (or the oracle's results computed earlier). Returns those results."""
    search = ctx.oracle_search()
    if expected is None:
        hits, closest_counts = oracle_q.trace_closest(scene.desc, closest, skip, use_bvh=search, with_lights=True) if len(closest) else (np.zeros((0, 4), np.float32), (0, 0))
        transmittance, shadow_counts = oracle_q.trace_shadow(scene.desc, shadow, use_bvh=search) if len(shadow) else (np.zeros(0, np.float32), (0, 0))
        for array in (hits, transmittance):
            array.setflags(write=False)
        expected = (hits, transmittance, tuple(closest_counts), tuple(shadow_counts))
    hits, transmittance, closest_counts, shadow_counts = expected
    ctx.set_instrumentation(instrumented)
    try:
        ctx.reset_counters()
        gpu_hits, gpu_transmittance = ctx.debug_trace_fused(closest, skip, shadow)
        counters = ctx.counters()
    finally:
        ctx.set_instrumentation(False)
    assert np.array_equal(gpu_hits.view(np.uint32), hits.view(np.uint32)), "t, u, v and primitive id must match bit for bit"
    assert np.array_equal(gpu_transmittance.view(np.uint32), transmittance.view(np.uint32))
    if instrumented:
        assert (counters["closest_nodes"], counters["closest_triangles"]) == closest_counts
        assert (counters["shadow_nodes"], counters["shadow_triangles"]) == shadow_counts
    return expected


# ---- ragged fused launches ------------------------------------------------------------------------------------------------------------------------------------------

CLOSEST_COUNTS = [1, 63, 64, 65, 127, 4097]
SHADOW_COUNTS = [0, 1, 65, 4097]
# every closest count with every shadow count, and the launches without closest-hit rays
RAGGED = [(c, s) for c in CLOSEST_COUNTS for s in SHADOW_COUNTS] + [(0, s) for s in SHADOW_COUNTS if s]
_ragged = {}


def ragged_rays(scene, n_closest, n_shadow):
    rng = np.random.default_rng(7000 * n_closest + n_shadow)
    closest = random_rays(rng, n_closest, -14.0, 14.0)
    skip = np.full(n_closest, MISS, np.uint32)
    skip[::3] = rng.integers(0, scene.desc.triangle_count, len(skip[::3]))      # some triangles to skip
    shadow = random_rays(rng, n_shadow, -14.0, 14.0)
    shadow[:, 7] = rng.uniform(0.05, 30.0, n_shadow).astype(np.float32)
    for array in (closest, skip, shadow):
        array.setflags(write=False)
    return closest, skip, shadow


@pytest.mark.parametrize("instrumented", [True, False], ids=["counting", "product"])
@pytest.mark.parametrize("n_closest,n_shadow", RAGGED, ids=[f"{c}-{s}" for c, s in RAGGED])
def test_ragged_fused_launch_matches_oracle(ctx, oracle_q, atrium, n_closest, n_shadow, instrumented):
    """The shadow rays follow the closest-hit rays in the launch's index space, a launch is cut into 64 shards by index and a wave that drains its shard moves on to
    the next open one: in the launches with both kinds of ray the waves that start on closest-hit shards end on shadow shards, so their lanes retire a closest-hit
    ray and take a shadow ray in one round. Which lanes do is a matter of timing and is not asserted (the library returns no counter of it); every ray's result is."""
    resident(ctx, atrium)
    closest, skip, shadow = ragged_rays(atrium, n_closest, n_shadow)
    key = (n_closest, n_shadow)
    _ragged[key] = fused(ctx, oracle_q, atrium, closest, skip, shadow, instrumented, _ragged.get(key))
    hits, transmittance = _ragged[key][:2]
    if n_closest >= 63:
        assert (hits[:, 3].view(np.uint32) != MISS).mean() > 0.2
    if n_shadow >= 65:
        assert 0.05 < (transmittance == 0).mean() < 0.99


# ---- rays that stress the bookkeeping -------------------------------------------------------------------------------------------------------------------------------

def bookkeeping_rays(scene, oracle_q, search):
    rng = np.random.default_rng(20)
    closest = []
    # all eight octants, from points inside the hall
    for octant in range(8):
        d = np.abs(rng.normal(size=(40, 3))).astype(np.float32) + 0.05
        d *= np.array([-1.0 if octant & 1 else 1.0, -1.0 if octant & 2 else 1.0, -1.0 if octant & 4 else 1.0], np.float32)
        d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
        o = rng.uniform(-10.0, 10.0, size=(40, 3)).astype(np.float32)
        o[:, 1] = np.abs(o[:, 1]) * 0.7
        closest.append(rays_of(o, d))
    # axis-parallel directions, the other two components +0 or -0 (the 1e-20 substitution takes their sign)
    for axis in range(3):
        for sign in (1.0, -1.0):
            for zero_a in (0.0, -0.0):
                for zero_b in (0.0, -0.0):
                    d = np.zeros((12, 3), np.float32)
                    d[:, axis] = sign
                    d[:, (axis + 1) % 3] = zero_a
                    d[:, (axis + 2) % 3] = zero_b
                    o = rng.uniform(-10.0, 10.0, size=(12, 3)).astype(np.float32)
                    o[:, 1] = np.abs(o[:, 1]) * 0.7
                    closest.append(rays_of(o, d))
    # origins outside the scene's bounds, heading away: the root is missed and the ray is done on its first item
    away = rng.normal(size=(70, 3)).astype(np.float32)
    away /= np.linalg.norm(away, axis=1, keepdims=True).astype(np.float32)
    closest.append(rays_of(away * 500.0, away))
    closest = np.concatenate(closest)
    skip = np.full(len(closest), MISS, np.uint32)

    # shadow rays that end before the first box they would enter: from far outside towards the scene, with a short extent
    shadow = [rays_of(away * 500.0, -away, tmax=1.0)]
    # shadow rays fully occluded by the first triangle they test: aimed at what a closest-hit ray found, ending just behind it
    probes = random_rays(rng, 400, -10.0, 10.0)
    found, _ = oracle_q.trace_closest(scene.desc, probes, np.full(len(probes), MISS, np.uint32), use_bvh=search, with_lights=False)
    surface = (found[:, 3].view(np.uint32) != MISS) & np.isfinite(found[:, 0]) & (found[:, 0] > 1e-2)
    blocked = probes[surface].copy()
    blocked[:, 7] = found[surface, 0] * np.float32(1.001)
    shadow.append(blocked)
    shadow = np.concatenate(shadow)
    for array in (closest, skip, shadow):
        array.setflags(write=False)
    return closest, skip, shadow


_bookkeeping = {}


@pytest.mark.parametrize("instrumented", [True, False], ids=["counting", "product"])
def test_rays_that_stress_the_bookkeeping_match_oracle(ctx, oracle_q, atrium, instrumented):
    resident(ctx, atrium)
    if "rays" not in _bookkeeping:
        _bookkeeping["rays"] = bookkeeping_rays(atrium, oracle_q, ctx.oracle_search())
    closest, skip, shadow = _bookkeeping["rays"]
    _bookkeeping["expected"] = fused(ctx, oracle_q, atrium, closest, skip, shadow, instrumented, _bookkeeping.get("expected"))
    hits, transmittance = _bookkeeping["expected"][:2]
    # the rays do what they were made for
    assert (hits[:8 * 40, 3].view(np.uint32) != MISS).mean() > 0.2                     # the octant rays find surfaces
    assert (hits[-70:, 3].view(np.uint32) == MISS).all()                               # the rays heading away find nothing
    assert (transmittance[:70] != 0).all()                                             # too short to reach the scene: nothing occludes them
    assert (transmittance[70:] == 0).mean() > 0.9                                      # ended behind the surface they were aimed at
    # the same closest-hit rays alone, and the shadow rays alone: the kernels of one kind carry the same bookkeeping
    ctx.set_instrumentation(instrumented)
    try:
        assert np.array_equal(ctx.debug_trace_closest(closest, skip).view(np.uint32), hits.view(np.uint32))
        assert np.array_equal(ctx.debug_trace_shadow(shadow).view(np.uint32), transmittance.view(np.uint32))
    finally:
        ctx.set_instrumentation(False)


# ---- the light lists the retire step tells apart ---------------------------------------------------------------------------------------------------------------------

SUN = dict(kind=LIGHT_DIRECTIONAL, direction=(0.3, -0.9, 0.2))
LIGHT_LISTS = {
    "directional-only": [SUN],
    "one-sphere": [SUN, dict(kind=LIGHT_SPHERE, position=(1.0, 4.0, 0.5), radius=1.5)],
    "dead-sphere-beside-live": [dict(kind=LIGHT_SPHERE, position=(-3.0, 3.0, 1.0), radius=0.0), dict(kind=LIGHT_SPHERE, position=(1.0, 4.0, 0.5), radius=1.5)],
    "spot": [dict(kind=LIGHT_SPHERE, position=(0.0, 0.0, 0.0), radius=0.0), dict(kind=LIGHT_SPOT, position=(-2.0, 5.0, 1.0), radius=2.0, direction=(0.0, -1.0, 0.0))],
    "sphere-and-spot": [SUN, dict(kind=LIGHT_SPHERE, position=(1.0, 4.0, 0.5), radius=1.5), dict(kind=LIGHT_SPOT, position=(-2.0, 5.0, 1.0), radius=2.0, direction=(0.0, -1.0, 0.0))],
    "two-spheres-overlapping": [dict(kind=LIGHT_SPHERE, position=(1.0, 4.0, 0.5), radius=1.5), SUN, dict(kind=LIGHT_SPHERE, position=(1.5, 4.2, 0.5), radius=1.5)],
}


def light_rays(lights):
    """Rays towards the lights from all over the hall (their light hit lies in front of the walls for some, behind a pillar or a banner for others) among rays
    that are not aimed at anything."""
    rng = np.random.default_rng(31)
    rays = [random_rays(rng, 300, -12.0, 12.0)]
    for l in lights:
        if l["kind"] == LIGHT_DIRECTIONAL:
            continue
        aimed = random_rays(rng, 500, -12.0, 12.0)
        target = np.array(l["position"], np.float32) + rng.uniform(-1.2, 1.2, size=(500, 3)).astype(np.float32) * np.float32(l["radius"])      # some pass it by
        d = target - aimed[:, 0:3]
        aimed[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
        rays.append(aimed)
    rays = np.concatenate(rays)
    rays.setflags(write=False)
    return rays


def cornell_spot_lights():
    """The sphere and the spot light of test_spot_light_image_matches_oracle's scene (the Cornell box itself is searched exhaustively: its lights are moved into the
    atrium's hall, 2.5 above the floor, and keep everything else)."""
    cornell = Scene("cornell", spot=True)
    assert cornell.desc.light_count == 2
    lights = []
    for k in range(2):
        l = cornell.desc.lights[k]
        assert l.flags & 7 in (LIGHT_SPHERE, LIGHT_SPOT) and l.data[6] > 0.0
        lights.append(dict(kind=int(l.flags & 7), position=(float(l.data[3]) * 4.0, float(l.data[4]) + 2.5, float(l.data[5]) * 4.0), radius=float(l.data[6]),
                           direction=tuple(float(v) for v in l.data[7:10]), cos_angle=float(l.data[10])))
    assert {l["kind"] for l in lights} == {LIGHT_SPHERE, LIGHT_SPOT}
    return lights


@pytest.mark.parametrize("name", list(LIGHT_LISTS) + ["cornell-spot-lights"])
def test_light_lists_match_oracle(ctx, oracle_q, atrium, name):
    lights = LIGHT_LISTS[name] if name in LIGHT_LISTS else cornell_spot_lights()
    scene = Relit(atrium, [light(**l) for l in lights])
    resident(ctx, scene)
    rays = light_rays(lights)
    skip = np.full(len(rays), MISS, np.uint32)
    cpu, counts = oracle_q.trace_closest(scene.desc, rays, skip, use_bvh=ctx.oracle_search(), with_lights=True)
    unlit, _ = oracle_q.trace_closest(scene.desc, rays, skip, use_bvh=ctx.oracle_search(), with_lights=False)
    for instrumented in (True, False):
        ctx.set_instrumentation(instrumented)
        try:
            ctx.reset_counters()
            gpu = ctx.debug_trace_closest(rays, skip)
            counters = ctx.counters()
        finally:
            ctx.set_instrumentation(False)
        assert np.array_equal(gpu.view(np.uint32), cpu.view(np.uint32)), (name, instrumented)
        if instrumented:
            assert (counters["closest_nodes"], counters["closest_triangles"]) == tuple(counts)
    ids = cpu[:, 3].view(np.uint32)
    on_light = (ids != MISS) & ((ids & LIGHT_HIT) != 0)
    analytic = [k for k, l in enumerate(lights) if l["kind"] != LIGHT_DIRECTIONAL and l["radius"] > 0.0]
    if not analytic:
        assert not on_light.any()
        return
    for k in analytic:                                       # every live light is found by some rays, under its own index ...
        assert (ids[on_light] == (LIGHT_HIT | k)).sum() > 20, (name, k)
    assert set(np.unique(ids[on_light] & ~np.uint32(LIGHT_HIT))) <= set(analytic)      # ... and no dead one by any
    surface_first = (unlit[:, 3].view(np.uint32) != MISS)
    assert (on_light & surface_first).sum() > 10             # the light hit lies in front of a triangle the ray would have reached
    assert (~on_light & surface_first).sum() > 10            # a triangle first (or no light on the way)
    aimed_and_blocked = ~on_light[300:] & surface_first[300:]
    assert aimed_and_blocked.sum() > 5                       # aimed at a light and stopped by a triangle before it


# ---- one small exact-mode render --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wavefronts", [1, 2])
def test_small_exact_render_matches_oracle(verify_ctx, oracle_q, atrium, wavefronts):
    """37 x 23 pixels, 3 samples per pass (2553 paths: no multiple of the wave), two passes, four bounces: every shadow ray's radiance reaches its path's slot
    through the retire step's read, add and write, issued among the loads of the rays that follow it. The f64 running mean, bit for bit."""
    w, h, samples, passes, bounces = 37, 23, 3, 2, 4
    resident(verify_ctx, atrium)
    verify_ctx.set_wavefront_count(wavefronts)
    try:
        verify_ctx.set_frame(w, h, 0, 1, samples)
        for a in range(0, samples * passes, samples):
            verify_ctx.render_pass(atrium.camera(w, h, accumulations=a, max_bounce_count=bounces))
        verify_ctx.synchronize()
        ours = verify_ctx.read_accumulation()[..., :3]
    finally:
        verify_ctx.set_wavefront_count(0)
        verify_ctx.set_frame(w, h, 0, 1, 1)
    if "image" not in _exact:
        before = oracle_q.lib.oracle_set_f64_transcendentals(1)
        try:
            _exact["image"], _, _ = oracle_q.render(atrium.desc, atrium.state, atrium.camera(w, h, max_bounce_count=bounces), w, h, samples * passes, use_bvh=verify_ctx.oracle_search())
        finally:
            oracle_q.lib.oracle_set_f64_transcendentals(before)
        _exact["image"].setflags(write=False)
    theirs = _exact["image"][..., :3]
    assert np.isfinite(ours).all() and float(theirs.mean()) > 0.0
    assert np.array_equal(ours, theirs), f"{(ours != theirs).any(axis=-1).sum()} of {w * h} pixels differ"


_exact = {}
