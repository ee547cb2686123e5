"""The hints of k_trace_wide8 (csrc/wide8_kernels.h): a ray may look at ONE record before it starts on the root -- the record its pixel's camera rays hit in the last
pass, or the record that stopped its pixel's last shadow ray. A hint chooses where a ray looks first and nothing else: every hit, every transmittance and every frame
is bit for bit what it is without hints, whatever the table holds.

  * closest-only, shadow-only and fused launches of 50 000, 777, 64, 33 and 1 rays of each kind through hipr_debug_trace_hinted, with the table empty, warmed by the
    same launch, filled with random record slots, filled with the one record most rays hit, and tagged with another generation: all equal the oracle;
  * exact-mode frames, 64 x 36, max_bounce_count 0, 1 and 4, 1, 3 and 64 samples per pass, one wavefront and two: after the cold pass and after two warm ones the
    accumulation equals the oracle's f64 mean, and the ray counters are the oracle's;
  * a frame of the counting instantiations (which have no code for hints) equals the product's after warm passes, with the oracle's node and triangle counters;
  * a device rebuild, an instance removal and a refit between two warm passes: the next frames equal a fresh context's;
  * a scene of single-triangle records; a sphere and a spot light that rays hit (the hint and the light test of the retire); the textured atrium, where the shadow
    rays run the coverage code and have no hints while the camera rays do.

tests/test_trace_hint_start_cpu.py holds what the start state rests on (the next-item step yields the root, then the unhinted sequence) on a host build.
"""
import numpy as np
import pytest

from bifrost3d_amd import capi
from bifrost3d_amd.host import Scene
from device_refit_bindings import decode_tree
from test_gpu_trace_refill_round import LIGHT_HIT, MISS, Relit, light
from test_gpu_trace_lean_records import LIGHT_LISTS, SUN, all_opaque, rays_around, two_kinds, write_loose_triangles_obj

pytestmark = pytest.mark.gpu

COUNTS = [50000, 777, 64, 33, 1]
CLOSEST, SHADOW, FUSED = 0, 1, 2
STATES = ["empty", "warmed", "random", "one-record", "stale"]


@pytest.fixture(scope="module")
def ctx():
    from bifrost3d_amd.renderer import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle_q():
    from oracle_bindings import get_oracle
    return get_oracle(True)


@pytest.fixture(scope="module")
def atrium():
    scene = Scene("atrium", param0=20000, param1=3)
    assert all_opaque(scene)
    return scene


def record_slots(scene):
    is_node, _ = decode_tree(scene.wide8_slots())
    return np.nonzero(~is_node)[0].astype(np.uint32)


def words_for(n):
    return (n + 63) // 64


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Reference:
    """The oracle's hits and transmittance of a set of rays, computed once and left unchanged."""
    def __init__(self, ctx, oracle_q, scene, closest, skip, shadow):
        search = ctx.oracle_search()
        self.closest, self.skip, self.shadow = closest, skip, shadow
        self.hits, _ = oracle_q.trace_closest(scene.desc, closest, skip, use_bvh=search, with_lights=True)
        self.transmittance, _ = oracle_q.trace_shadow(scene.desc, shadow, use_bvh=search)
        self.hits.setflags(write=False)
        self.transmittance.setflags(write=False)

    def launch(self, ctx, mode, table):
        """One hinted launch; asserts its results and returns (table as left, tag)."""
        none = np.zeros((0, 8), np.float32)
        closest, skip = (self.closest, self.skip) if mode != SHADOW else (none, None)
        shadow = self.shadow if mode != CLOSEST else none
        hits, transmittance, table, tag = ctx.debug_trace_hinted(mode, closest, skip, shadow, table)
        if mode != SHADOW:
            assert np.array_equal(bits(hits), bits(self.hits)), "t, u, v and primitive id must match bit for bit"
        if mode != CLOSEST:
            assert np.array_equal(bits(transmittance), bits(self.transmittance))
        return table, tag


def tables_in_every_state(ctx, reference, mode, n, records, rng):
    """The launch of `mode` with the table in each of STATES, in their order; returns the warmed table."""
    words = words_for(n)
    warmed, tag = reference.launch(ctx, mode, np.zeros(words, np.uint32))                      # empty
    assert tag != 0 and tag & 0xFFFFFF == 0
    written = warmed[warmed != 0]
    assert (written >> 24 == tag >> 24).all() and np.isin(written & 0xFFFFFF, records).all()      # what a launch writes names a record of this tree
    again, _ = reference.launch(ctx, mode, warmed)                                           # warmed by the same launch
    assert (again != 0).sum() >= (warmed != 0).sum()
    reference.launch(ctx, mode, tag | rng.choice(records, words))                              # random valid record slots
    slots = written & 0xFFFFFF
    common = np.bincount(slots).argmax() if len(slots) else records[0]
    reference.launch(ctx, mode, np.full(words, tag | common, np.uint32))                     # one record that many rays hit
    stale = ((tag >> 24) % 255 + 1) << 24                                                    # another generation, never 0
    left, _ = reference.launch(ctx, mode, np.uint32(stale) | rng.integers(0, 1 << 24, words, dtype=np.uint32))      # slots of a stale tag are never read: any will do
    return warmed


@pytest.mark.parametrize("count", COUNTS)
def test_launches_with_the_table_in_every_state_match_oracle(ctx, oracle_q, atrium, count):
    ctx.upload_scene(atrium)
    ctx.set_instrumentation(False)
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    rng = np.random.default_rng(7000 + count)
    closest, skip, shadow = two_kinds(rng, count, -14.0, 14.0, atrium.desc.triangle_count)
    # groups of 64 rays that share a table word are one pixel's samples in a pass: half of the groups here are such bundles (one origin, directions a degree apart),
    # so that a hint is often the record the next ray hits; the others stay unrelated rays, for which a hint is nearly always a wasted visit
    for rays in (closest, shadow):
        for g in range(0, count, 128):
            rays[g:g + 64, 0:3] = rays[g, 0:3]
            d = rays[g, 4:7] + rng.normal(0.0, 0.01, (len(rays[g:g + 64]), 3)).astype(np.float32)
            rays[g:g + 64, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    reference = Reference(ctx, oracle_q, atrium, closest, skip, shadow)
    records = record_slots(atrium)
    for mode in (CLOSEST, SHADOW, FUSED):
        warmed = tables_in_every_state(ctx, reference, mode, count, records, rng)
        if count >= 777:
            assert (warmed != 0).mean() > 0.5, mode      # most groups had a ray that hit (closest) or was stopped (shadow)
    if count >= 777:
        assert 0.2 < (reference.hits[:, 3].view(np.uint32) != MISS).mean() < 0.999
        assert 0.05 < (reference.transmittance == 0).mean() < 0.99


def test_an_entry_that_names_a_node_is_refused(ctx, atrium):
    ctx.upload_scene(atrium)
    rays = np.zeros((1, 8), np.float32)
    rays[0, 4] = 1.0
    _, _, _, tag = ctx.debug_trace_hinted(CLOSEST, rays, None, np.zeros((0, 8), np.float32), np.zeros(1, np.uint32))
    with pytest.raises(capi.HiprError):
        ctx.debug_trace_hinted(CLOSEST, rays, None, np.zeros((0, 8), np.float32), np.array([tag | 0], np.uint32))      # slot 0 is the root


def test_a_scene_of_single_triangle_records_matches_oracle(ctx, oracle_q, tmp_path):
    side = 24
    scene = Scene("file:" + write_loose_triangles_obj(tmp_path / "loose.obj", side))
    assert all_opaque(scene)
    ctx.upload_scene(scene)
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    rng = np.random.default_rng(29)
    n = 6000
    closest, skip, shadow = two_kinds(rng, n, 0.0, float(side), scene.desc.triangle_count)
    for rays in (closest, shadow):
        rays[:, 1] = rng.uniform(-1.0, 5.0, n).astype(np.float32)
    reference = Reference(ctx, oracle_q, scene, closest, skip, shadow)
    records = record_slots(scene)
    for mode in (CLOSEST, SHADOW, FUSED):
        tables_in_every_state(ctx, reference, mode, n, records, rng)
    assert 0.1 < (reference.hits[:, 3].view(np.uint32) != MISS).mean() < 0.95


@pytest.mark.parametrize("name", list(LIGHT_LISTS))
def test_hinted_rays_that_hit_a_light_match_oracle(ctx, oracle_q, atrium, name):
    """The record of the hint seeds tmax, the light test of the retire then finds the light in front of it or behind it."""
    lights = LIGHT_LISTS[name]
    scene = Relit(atrium, [light(**l) for l in lights])
    ctx.upload_scene(scene)
    rng = np.random.default_rng(43)
    n = 400
    analytic = [k for k, l in enumerate(lights) if l is not SUN]
    closest = np.concatenate([rays for k in analytic for rays in rays_around(rng, lights[k], n)])
    skip = np.full(len(closest), MISS, np.uint32)
    shadow = closest.copy()
    shadow[:, 7] = rng.uniform(0.05, 30.0, len(shadow)).astype(np.float32)
    reference = Reference(ctx, oracle_q, scene, closest, skip, shadow)
    records = record_slots(atrium)      # the lights are not in the tree
    for mode in (CLOSEST, FUSED):
        tables_in_every_state(ctx, reference, mode, len(closest), records, rng)
    ids = reference.hits[:, 3].view(np.uint32)
    assert ((ids != MISS) & ((ids & LIGHT_HIT) != 0)).sum() > 20


def test_the_textured_atrium_matches_oracle(ctx, oracle_q):
    """Shadow rays run the coverage code there and have no hints (their table comes back as given); camera rays have them."""
    scene = Scene("atrium", param0=20000, param1=3, textured=True)
    assert not all_opaque(scene)
    ctx.upload_scene(scene)
    rng = np.random.default_rng(53)
    closest, skip, shadow = two_kinds(rng, 777, -14.0, 14.0, scene.desc.triangle_count)
    reference = Reference(ctx, oracle_q, scene, closest, skip, shadow)
    warmed = tables_in_every_state(ctx, reference, CLOSEST, 777, record_slots(scene), rng)
    assert (warmed != 0).any()
    for mode in (SHADOW, FUSED):
        given = np.zeros(words_for(777), np.uint32)
        left, _ = reference.launch(ctx, mode, given)
        assert np.array_equal(left, given)
    assert 0.05 < (reference.transmittance == 0).mean() < 0.99


W, H, PASSES = 64, 36, 3
_oracle_passes = {}


def oracle_passes(oracle_q, scene, search, bounces, spp):
    """The oracle's accumulation and summed ray counters after each of PASSES passes of spp samples, computed once per (bounces, spp)."""
    key = (bounces, spp)
    if key not in _oracle_passes:
        frames, counters, accum = [], [], None
        total = {}
        before = oracle_q.lib.oracle_set_f64_transcendentals(1)
        try:
            for p in range(PASSES):
                accum, c, _ = oracle_q.render(scene.desc, scene.state, scene.camera(W, H, accumulations=p * spp, max_bounce_count=bounces), W, H, spp, use_bvh=search, accum=accum)
                for k, v in c.items():
                    total[k] = total.get(k, 0) + v
                frame = accum.copy()
                frame.setflags(write=False)
                frames.append(frame)
                counters.append(dict(total))
        finally:
            oracle_q.lib.oracle_set_f64_transcendentals(before)
        _oracle_passes[key] = (frames, counters)
    return _oracle_passes[key]


def begin_frames(context, scene, spp, wavefronts, instrumented=False, upload=True):
    if upload:
        context.upload_scene(scene)
    context.set_instrumentation(instrumented)
    context.set_wavefront_count(wavefronts)
    context.set_frame(W, H, 0, 1, spp)
    context.reset_counters()


def end_frames(context):
    context.set_wavefront_count(0)
    context.set_instrumentation(False)
    context.set_frame(W, H, 0, 1, 1)


def one_pass(context, scene, p, spp, bounces):
    context.render_pass(scene.camera(W, H, accumulations=p * spp, max_bounce_count=bounces))
    context.synchronize()
    return context.read_accumulation(), context.counters()


@pytest.mark.parametrize("wavefronts", [1, 2])
@pytest.mark.parametrize("spp", [1, 3, 64])
@pytest.mark.parametrize("bounces", [0, 1, 4])
def test_cold_and_warm_exact_frames_equal_the_oracle_bit_for_bit(verify_ctx, oracle_q, atrium, bounces, spp, wavefronts):
    begin_frames(verify_ctx, atrium, spp, wavefronts)
    try:
        frames, oracle_counters = oracle_passes(oracle_q, atrium, verify_ctx.oracle_search(), bounces, spp)
        for p in range(PASSES):      # pass 0 meets empty tables, the others what the pass before left
            ours, counters = one_pass(verify_ctx, atrium, p, spp, bounces)
            ours, theirs = ours[..., :3], frames[p][..., :3]
            assert np.isfinite(ours).all() and float(theirs.mean()) > 0.0
            assert np.array_equal(ours, theirs), f"pass {p}: {(ours != theirs).any(axis=-1).sum()} of {W * H} pixels differ"
            for key in ("camera_rays", "closest_rays", "shadow_rays"):
                assert counters[key] == oracle_counters[p][key] > 0, (p, key)
    finally:
        end_frames(verify_ctx)


def test_the_counting_kernels_frame_and_counters_after_warm_passes(verify_ctx, oracle_q, atrium):
    """The counting instantiations have no code for hints: their node and triangle counters are the oracle's, and their frame is the product's, whose passes ran hinted.
    In the exact arithmetic mode, whose paths are the oracle's."""
    ctx = verify_ctx
    spp, bounces = 4, 4
    results = {}
    for instrumented in (False, True):
        begin_frames(ctx, atrium, spp, 1, instrumented)
        try:
            for p in range(PASSES):
                results[instrumented] = one_pass(ctx, atrium, p, spp, bounces)
        finally:
            end_frames(ctx)
    (product, product_counters), (counting, counting_counters) = results[False], results[True]
    assert np.isfinite(product).all() and float(product[..., :3].mean()) > 0
    assert np.array_equal(product.view(np.uint64), counting.view(np.uint64))
    _, oracle_counters = oracle_passes(oracle_q, atrium, ctx.oracle_search(), bounces, spp)
    for key in ("closest_rays", "shadow_rays", "camera_rays"):
        assert product_counters[key] == counting_counters[key] == oracle_counters[-1][key] > 0, key
    for key in ("closest_nodes", "closest_triangles", "shadow_nodes", "shadow_triangles"):
        assert counting_counters[key] == oracle_counters[-1][key] > 0, key


def passes_around(context, scene, edits, instrumented, warm):
    """`warm`: two passes before every edit, so that the tables hold the old tree's records when it is made. After each edit the accumulation starts again: the frames
    of its two passes."""
    spp, bounces = 8, 4
    frames = []
    begin_frames(context, scene, spp, 1, instrumented)
    try:
        for edit in edits:
            if warm:
                for p in range(2):
                    one_pass(context, scene, p, spp, bounces)
            edit(context, scene)
            context.set_instrumentation(instrumented)
            frames += [one_pass(context, scene, p, spp, bounces)[0].copy() for p in range(2)]
    finally:
        end_frames(context)
    return frames


def rebuild_on_the_device(context, scene):
    assert context.rebuild_scene_trees(read_back=False)["status"] == capi.HIPR_OK, context.lib.hipr_last_error()


def remove_a_model(context, scene):
    import instance_edit_bindings as ie
    ie.apply(scene, [("remove", 12)])
    assert context.edit_scene_instances(scene.staged_instance_edits(), read_back=False)["status"] == capi.HIPR_OK, context.lib.hipr_last_error()


def refit_a_model(context, scene):
    from device_rebuild_bindings import POSE
    before = context.read_scene_buffer(capi.SCENE_BUFFER_WIDE8_SLOTS)
    assert not context.refit_scene_transforms(scene.model_pose(10, **POSE))["needs_rebuild"]      # the model tests/test_gpu_device_refit.py moves in this atrium
    assert not np.array_equal(before, context.read_scene_buffer(capi.SCENE_BUFFER_WIDE8_SLOTS))      # boxes and records did move, slot for slot in place


@pytest.mark.parametrize("name", ["rebuild-then-removal", "refit"])
def test_frames_after_an_edit_between_warm_passes_equal_a_fresh_contexts(ctx, name):
    """The resident tree is replaced (its generation moves on: the old entries name no record of the new tree) or refitted (the entries stay usable: stale records,
    valid slots) under warm tables. The yardstick is a fresh context that makes the same edits with no pass before them and renders with the counting
    instantiations, which have no code for hints."""
    from bifrost3d_amd.renderer import Context
    edits = [rebuild_on_the_device, remove_a_model] if name == "rebuild-then-removal" else [refit_a_model]
    arguments = dict(param0=20000, param1=3)
    ours = passes_around(ctx, Scene("atrium", **arguments), edits, instrumented=False, warm=True)
    fresh = Context(0)
    try:
        theirs = passes_around(fresh, Scene("atrium", **arguments), edits, instrumented=True, warm=False)
    finally:
        fresh.close()
    assert len(ours) == len(theirs) == 2 * len(edits)
    for k, (a, b) in enumerate(zip(ours, theirs)):
        assert np.isfinite(a).all() and float(a[..., :3].mean()) > 0
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"frame {k}: {(a != b).any(axis=-1).sum()} of {W * H} pixels differ"
