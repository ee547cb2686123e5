"""The shade stage's listing pass and what follows from it (csrc/kernels.h k_classify_hits, csrc/shade_schedule.h, csrc/shade_kernel.h):

  * the listing itself, through hipr_debug_classify_hits: `order` is a permutation of the queue; every chunk of 4096 places holds exactly that chunk's entries as
    [plain surface hits | coated surface hits | everything else], each class in rising (queue) order; two runs give the same listing;
  * frames do not depend on it: a small atrium rendered with the listing forced on equals, bit for bit, the render with HIPR_SHADE_ORDERED=0 (k_shade then takes the
    queue's own order with the plain grid stride instead of the chunks through shade_schedule.h);
  * the last bounce without its BSDF sample: the exact arithmetic mode still equals the oracle bit for bit at max_bounce_count 0, 1 and 4.
"""
import os

import numpy as np
import pytest

from bifrost3d_amd import capi
from bifrost3d_amd.host import Scene

pytestmark = pytest.mark.gpu

CHUNK = 4096
MISS, LIGHT = 0xFFFFFFFF, 0x80000000
SIZES = (1, 63, 64, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 1000)
SURFACE_SHARES = (0.0, 0.4, 1.0)


@pytest.fixture(scope="module")
def coated():
    """A small scene with coated materials (the atrium of 2 312 triangles: 214 of them carry a coat), uploaded, and the class byte of each of its triangles as the device holds them."""
    from bifrost3d_amd.renderer import Context
    scene = Scene("atrium", param0=3000, param1=3)
    c = Context(0)
    c.upload_scene(scene)
    classes = c.read_scene_buffer(capi.SCENE_BUFFER_TRIANGLE_CLASS) & 1
    assert 0 < int(classes.sum()) < len(classes)      # coated and plain triangles both
    yield c, classes
    c.close()


def make_hits(n, surface_share, classes, seed):
    """(n, 4) hits {t, u, v, bits(id)}: `surface_share` of them on triangles of the scene (half of those on coated ones), the rest misses and light hits, interleaved at random."""
    rng = np.random.default_rng(seed)
    ids = np.where(rng.random(n) < 0.5, MISS, LIGHT | rng.integers(0, 3, n)).astype(np.uint32)
    surface = rng.random(n) < surface_share if 0.0 < surface_share < 1.0 else np.full(n, surface_share == 1.0)
    coated_triangles, plain_triangles = np.nonzero(classes)[0], np.nonzero(classes == 0)[0]
    on_coat = rng.random(n) < 0.5
    triangle = np.where(on_coat, coated_triangles[rng.integers(0, len(coated_triangles), n)], plain_triangles[rng.integers(0, len(plain_triangles), n)])
    ids[surface] = triangle[surface].astype(np.uint32)
    hits = rng.random((n, 4), dtype=np.float32)
    hits[:, 3] = ids.view(np.float32)
    return hits, ids


def expected_listing(ids, classes, coat_classes):
    """The listing as kernels.h states it: per chunk [plain surface hits | coated surface hits | everything else], each in queue order."""
    surface = (ids != MISS) & ((ids & LIGHT) == 0)
    kind = np.full(len(ids), 2)
    kind[surface] = classes[ids[surface]] if coat_classes else 0      # without the classes a coated hit is a plain one
    out = []
    for begin in range(0, len(ids), CHUNK):
        k = kind[begin:begin + CHUNK]
        out.append(begin + np.argsort(k, kind="stable"))
    return np.concatenate(out).astype(np.uint32), kind


@pytest.mark.parametrize("coat_classes", [False, True])
@pytest.mark.parametrize("share", SURFACE_SHARES)
def test_the_listing_holds_every_chunk_by_class_in_queue_order(coated, share, coat_classes):
    ctx, classes = coated
    for n in SIZES:
        hits, ids = make_hits(n, share, classes, seed=1000 * n + int(10 * share))
        order = ctx.debug_classify_hits(hits, coat_classes=coat_classes)
        again = ctx.debug_classify_hits(hits, coat_classes=coat_classes)
        assert np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32)), n                    # a permutation of range(n)
        expected, kind = expected_listing(ids, classes, coat_classes)
        for begin in range(0, n, CHUNK):
            part = order[begin:begin + CHUNK].astype(np.int64)
            assert part.min() >= begin and part.max() < min(begin + CHUNK, n), (n, begin)          # exactly that chunk's indices (with the permutation above)
            kinds = kind[part]
            assert (np.diff(kinds) >= 0).all(), (n, begin)                                         # plain, then coated, then everything else
            for k in range(3):
                assert (np.diff(part[kinds == k]) > 0).all(), (n, begin, k)                        # inside a class the indices rise
        assert np.array_equal(order, expected), n
        assert np.array_equal(order, again), n                                                     # equal across two runs


def test_a_block_that_lists_several_chunks_lists_each_in_place(coated):
    """The launch of a pass gives every chunk its own block up to eight blocks per CU; with fewer blocks than chunks a block goes on to the chunk a grid further."""
    ctx, classes = coated
    n = 3 * CHUNK + 1000
    hits, ids = make_hits(n, 0.4, classes, seed=7)
    expected, _ = expected_listing(ids, classes, True)
    for grid in (1, 2, 3):
        assert np.array_equal(ctx.debug_classify_hits(hits, coat_classes=True, grid=grid), expected), grid


def test_the_listing_entry_refuses_a_triangle_the_scene_does_not_hold(coated):
    ctx, classes = coated
    hits = np.zeros((4, 4), np.float32)
    hits[:, 3] = np.array([0, len(classes), MISS, LIGHT], np.uint32).view(np.float32)
    with pytest.raises(capi.HiprError):
        ctx.debug_classify_hits(hits, coat_classes=True)
    assert np.array_equal(ctx.debug_classify_hits(hits, coat_classes=False), np.array([0, 1, 2, 3], np.uint32))      # no class byte is read: ids are not looked up


def render_with(settings, scene, w, h, batch, passes, bounces):
    from bifrost3d_amd.renderer import Context
    names = ("HIPR_SHADE_ORDERED_FROM", "HIPR_SHADE_CLASSES", "HIPR_SHADE_ORDERED")
    saved = {k: os.environ.get(k) for k in names}
    for k in names:
        os.environ.pop(k, None)
    os.environ.update(settings)
    try:
        c = Context(0)       # the switches are read when the context is created
    finally:
        for k, v in saved.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
    try:
        c.upload_scene(scene)
        assert c.trace_variant() == capi.TRACE_WIDE8_PERSISTENT      # the scenes of the persistent kernels are the ones that list
        c.set_frame(w, h, 0, 1, batch)
        c.reset_counters()
        for p in range(passes):
            c.render_pass(scene.camera(w, h, accumulations=p * batch, max_bounce_count=bounces))
        c.synchronize()
        return c.read_accumulation(), c.counters()
    finally:
        c.close()


def test_frames_and_counters_equal_those_of_the_unlisted_render():
    """64 x 36 x 8 accumulations per pass = 18 432 camera rays; these are not listed (k_shade takes their queue with the plain stride). Bounces 1 to 4 are, with up to
    4.5 chunks of the listing and 72 shade batches each. The host sizes every shade launch to a multiple of 8 blocks, 8 at the least (hiprenderer.hip grid_for rounds
    up), whatever bound it holds for the bounce and however the pass is split into wavefronts -- so every listed bounce goes through shade_batch's schedule by XCD,
    never through its strided fall-back, here with nine blocks per XCD or fewer: chunks over several rounds, a partial last chunk, rounds without a batch, XCDs without a chunk. HIPR_SHADE_ORDERED_FROM brings the listing down to that size."""
    scene = Scene("atrium", param0=3000, param1=3)
    w, h, batch, passes, bounces = 64, 36, 8, 2, 4
    listed, c_listed = render_with(dict(HIPR_SHADE_ORDERED_FROM="1"), scene, w, h, batch, passes, bounces)
    classes, c_classes = render_with(dict(HIPR_SHADE_ORDERED_FROM="1", HIPR_SHADE_CLASSES="1"), scene, w, h, batch, passes, bounces)
    plain, c_plain = render_with(dict(HIPR_SHADE_ORDERED="0"), scene, w, h, batch, passes, bounces)
    assert np.isfinite(plain).all() and float(plain[..., :3].mean()) > 0
    assert np.array_equal(listed.view(np.uint64), plain.view(np.uint64)) and np.array_equal(classes.view(np.uint64), plain.view(np.uint64))
    for key in ("closest_rays", "shadow_rays", "shaded_hits", "camera_rays"):
        assert c_listed[key] == c_classes[key] == c_plain[key] and (c_plain[key] > 0 or key == "shadow_rays" and not scene.desc.light_count), key


@pytest.fixture(scope="module")
def exact():
    from bifrost3d_amd.renderer import Context
    c = Context(0, arithmetic="exact")
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle_q():
    from oracle_bindings import get_oracle
    return get_oracle(True)


@pytest.mark.parametrize("bounces", [0, 1, 4])
@pytest.mark.parametrize("name", ["cornell", "atrium"])
def test_the_exact_mode_equals_the_oracle_whatever_the_last_bounce(exact, oracle_q, name, bounces):
    """A hit at the last bounce queues its shadow ray and ends: the BSDF sample it would draw is used by nothing (shade_kernel.h shade_path). Every pixel's f64 running
    mean is the oracle's bit for bit, where the last bounce is the camera ray's hit (0), the one after (1) and the fourth."""
    scene = Scene("cornell") if name == "cornell" else Scene("atrium", param0=3000, param1=3)
    w, h, spp = 32, 18, 4
    exact.upload_scene(scene)
    exact.set_frame(w, h)
    for a in range(spp):
        exact.render_pass(scene.camera(w, h, accumulations=a, max_bounce_count=bounces), synchronize=True)
    ours = exact.read_accumulation()[..., :3]
    before = oracle_q.lib.oracle_set_f64_transcendentals(1)
    try:
        theirs, counters, _ = oracle_q.render(scene.desc, scene.state, scene.camera(w, h, max_bounce_count=bounces), w, h, spp, use_bvh=exact.oracle_search())
    finally:
        oracle_q.lib.oracle_set_f64_transcendentals(before)
    theirs = theirs[..., :3]
    assert np.isfinite(ours).all() and counters["shaded_hits"] > 0
    assert ours.dtype == theirs.dtype == np.float64
    assert (ours == theirs).all(), float((ours == theirs).all(axis=-1).mean())      # finite values of equal value: the comparison of tests/test_gpu_verify_build.py, here for every pixel
