"""The shade kernel fetches per ray what its kind of hit reads (csrc/shade_kernel.h shade_fetch_by_kind): a surface hit its direction, a light hit direction and
origin, a miss its direction under an environment map only -- and its path's radiance a batch ahead, which k_shade then adds to without reading it again -- a dead
slot nothing, the AOV entries both for every live entry. None of it may show in a frame:

  * the exact arithmetic mode still equals the oracle bit for bit, every pixel's f64 mean;
  * the fast mode's listed render equals the render with HIPR_SHADE_ORDERED=0 (the queue's own order: the same rule lane by lane) bit for bit, with equal counters;
  * the depth and denoiser-albedo AOV entries equal the oracle's (the comparison of tests/test_gpu_parity.py test_aov_entry_points_match_oracle);
  * one and two wavefronts give the same frame (the radiance a miss fetched ahead belongs to its own path, whichever wavefront co-runs).

Scenes: a small atrium (2 312 triangles; open to a constant sky, a sphere light: misses, light hits and surface hits in one chunk of the listing), the same under an
environment map (a miss reads direction and pdf), the same with a black sky (a miss adds nothing), and the Cornell box (the unlisted small-scene kernels; at
max_bounce_count 0 it is lit through shadow rays alone, most of them occluded or unoccluded in whole waves). Frames of 72 x 44: the 44 rows leave a partial tile row, so
dead slots; 4 samples per pass in two passes, or 48 samples in one pass = 152 k path slots, which two wavefronts share. The listing is forced on from the first
entry (HIPR_SHADE_ORDERED_FROM=1) the way tests/test_gpu_shade_listing.py does it. max_bounce_count 0, 1 and 4."""
import ctypes as C
import os

import numpy as np
import pytest

from bifrost3d_amd import capi
from bifrost3d_amd.host import Scene

pytestmark = pytest.mark.gpu

W, H = 72, 44
SCENES = ("atrium", "atrium_environment", "atrium_black_sky", "cornell")
BOUNCES = (0, 1, 4)
COUNTERS = ("closest_rays", "shadow_rays", "shaded_hits", "camera_rays")


class Staged:
    """A scene and the scene state it is rendered under (the black sky is a change of the state alone)."""
    def __init__(self, name):
        self.name = name
        if name == "cornell": self.scene = Scene("cornell")
        else: self.scene = Scene("atrium", param0=3000, param1=3, environment=name == "atrium_environment")
        self.state = self.scene.state
        if name == "atrium_black_sky": self.state.environment_tint[:] = (0.0, 0.0, 0.0)
        assert bool(self.scene.desc.environment) == (name == "atrium_environment")

    def upload(self, ctx):
        ctx.upload_scene(self.scene)
        ctx._check(ctx.lib.hipr_set_scene_state(ctx.handle, C.byref(self.state)), "hipr_set_scene_state")


@pytest.fixture(scope="module")
def staged():
    return {name: Staged(name) for name in SCENES}


def context_with(settings, arithmetic=None):
    from bifrost3d_amd.renderer import Context
    names = ("HIPR_SHADE_ORDERED_FROM", "HIPR_SHADE_CLASSES", "HIPR_SHADE_ORDERED")
    saved = {k: os.environ.get(k) for k in names}
    for k in names:
        os.environ.pop(k, None)
    os.environ.update(settings)
    try:
        return Context(0, arithmetic=arithmetic)      # the switches are read when the context is created
    finally:
        for k, v in saved.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


@pytest.fixture(scope="module")
def listed():
    c = context_with(dict(HIPR_SHADE_ORDERED_FROM="1"))
    yield c
    c.close()


@pytest.fixture(scope="module")
def unlisted():
    c = context_with(dict(HIPR_SHADE_ORDERED="0"))
    yield c
    c.close()


@pytest.fixture(scope="module")
def exact():
    c = context_with(dict(HIPR_SHADE_ORDERED_FROM="1"), arithmetic="exact")
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle_q():
    from oracle_bindings import get_oracle
    return get_oracle(True)


def render(ctx, staged_scene, batch, passes, bounces, wavefronts=0, entry=None):
    staged_scene.upload(ctx)
    if entry is not None: ctx.set_entry_point(entry)
    try:
        ctx.set_wavefront_count(wavefronts)
        ctx.set_frame(W, H, 0, 1, batch)
        ctx.reset_counters()
        for p in range(passes):
            ctx.render_pass(staged_scene.scene.camera(W, H, accumulations=p * batch, max_bounce_count=bounces))
        ctx.synchronize()
        return ctx.read_accumulation(), ctx.counters()
    finally:
        ctx.set_wavefront_count(0)
        if entry is not None: ctx.set_entry_point(capi.ENTRY_PATH_TRACING)


@pytest.mark.parametrize("bounces", BOUNCES)
@pytest.mark.parametrize("name", SCENES)
def test_the_exact_mode_equals_the_oracle_bit_for_bit(exact, oracle_q, staged, name, bounces):
    s = staged[name]
    ours, counters = render(exact, s, 4, 2, bounces)
    ours = ours[..., :3]
    before = oracle_q.lib.oracle_set_f64_transcendentals(1)
    try:
        theirs, oracle_counters, _ = oracle_q.render(s.scene.desc, s.state, s.scene.camera(W, H, max_bounce_count=bounces), W, H, 8, use_bvh=exact.oracle_search())
    finally:
        oracle_q.lib.oracle_set_f64_transcendentals(before)
    theirs = theirs[..., :3]
    assert np.isfinite(ours).all() and counters["shaded_hits"] > 0
    assert ours.dtype == theirs.dtype == np.float64
    assert (ours == theirs).all(), float((ours == theirs).all(axis=-1).mean())
    if name == "atrium_black_sky" and bounces == 0:
        assert float(ours.sum()) > 0      # ... and the frame is not black with the sky: light hits and lit surfaces remain


@pytest.mark.parametrize("bounces", BOUNCES)
@pytest.mark.parametrize("name", SCENES)
def test_the_listed_render_equals_the_unlisted_one(listed, unlisted, staged, name, bounces):
    s = staged[name]
    a, counters_a = render(listed, s, 4, 2, bounces)
    b, counters_b = render(unlisted, s, 4, 2, bounces)
    if name != "cornell": assert listed.trace_variant() == capi.TRACE_WIDE8_PERSISTENT      # the scenes of the persistent kernels are the ones that list
    assert np.isfinite(b).all() and float(b[..., :3].mean()) > 0
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    for key in COUNTERS:
        assert counters_a[key] == counters_b[key] and (counters_b[key] > 0 or key == "shadow_rays"), key


@pytest.mark.parametrize("entry_name,entry", [("depth", capi.ENTRY_DEPTH), ("denoiser_albedo", capi.ENTRY_DENOISER_ALBEDO)])
@pytest.mark.parametrize("name", ["cornell", "atrium", "atrium_environment"])
def test_the_aov_entries_that_read_origin_and_direction_match_the_oracle(listed, oracle_q, staged, name, entry_name, entry):
    s = staged[name]
    gpu, _ = render(listed, s, 1, 2, 4, entry=entry)
    # the oracle with the search the device runs: on the small atrium the oracle's own BVH2 and 8-wide searches give first hits that differ in more than a quarter of
    # this frame (0.716 of the denoiser albedo's pixels agree between the two), and its BVH2 and exhaustive searches differ in four pixels of the Cornell box
    cpu, _, _ = oracle_q.render(s.scene.desc, s.state, s.scene.camera(W, H, max_bounce_count=4), W, H, 2, use_bvh=listed.oracle_search(), entry=entry)
    tol = 2e-3 if "albedo" in entry_name else 1e-5
    if entry_name == "depth":   # world units, scaled by the scene size on both sides
        tol = 1e-5 * max(1.0, float(np.nanmax(np.where(np.isfinite(cpu[..., 0]), cpu[..., 0], 0.0))))
    g, c = gpu[..., :3], cpu[..., :3]
    if entry_name == "depth":
        # a miss adds |origin - 1e30 * direction| = +inf, and the running mean of inf is NaN from the second accumulation on: the same pixels on both sides
        assert np.array_equal(np.isfinite(g), np.isfinite(c))
        assert 0.05 < np.isfinite(c).mean()
        g, c = np.where(np.isfinite(g), g, 0.0), np.where(np.isfinite(c), c, 0.0)
    err = np.abs(g - c).max(axis=-1)
    assert (err <= tol).mean() >= 0.999, (entry_name, float(err.max()), float((err <= tol).mean()))
    assert np.isfinite(g).all()


@pytest.mark.parametrize("name", ["atrium", "atrium_environment", "atrium_black_sky"])
def test_one_and_two_wavefronts_give_the_same_frame(listed, staged, name):
    s = staged[name]
    one, counters_one = render(listed, s, 48, 1, 4, wavefronts=1)
    two, counters_two = render(listed, s, 48, 1, 4, wavefronts=2)
    assert np.isfinite(one).all() and float(one[..., :3].mean()) > 0
    assert np.array_equal(one.view(np.uint64), two.view(np.uint64))
    for key in COUNTERS:
        assert counters_one[key] == counters_two[key] > 0, key
