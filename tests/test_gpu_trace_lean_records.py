"""The lean record block and the lean retire of k_trace_wide8 (csrc/wide8_kernels.h), against the oracle bit for bit.

In a scene whose triangles are all statically opaque the product's fused and shadow launches run the instantiations without coverage code and without counters. There
a shadow lane never loads a record's fourth quad (triangle ids, flags, facing margin) and takes "is there a second triangle" from e3; in a fused launch the load sits
behind the lane's kind, so that a wave whose record lanes all hold shadow rays issues three loads per record. And every uninstrumented closest-hit retire takes the
analytic light test in two steps: the cheap decision for every lane, the square root and the compare with the ray's bounds only where some lane of the wave can hit.
Neither may change a bit of a result:

  * fused launches of n closest-hit + n shadow rays, and the launches of one kind, for n = 50 000, 777, 64, 33 and 1 on the 20 k-triangle atrium: the chunk that
    straddles the two kinds, ragged waves, a launch of one ray of each kind;
  * a scene whose leaves are records of ONE triangle only (no two triangles of it share a corner): every record takes the e3 path;
  * a sphere light, a spot light of radius > 0, and both (the list walk), with rays that hit the light, graze it and pass it by;
  * the textured atrium once: the coverage instantiation, whose code is the parent's;
  * exact-mode frames of the atrium at max_bounce_count 0, 1 and 4, with one wavefront and with two, against the oracle's f64 mean;
  * a frame rendered by the counting instantiations equals the frame of the product's, with equal ray counters.

tests/test_record_without_second_triangle_cpu.py holds the claim the record block rests on (e3 == 0 refuses every ray) on the host build of the routines.
"""
import numpy as np
import pytest

from bifrost3d_amd import capi
from bifrost3d_amd.host import Scene
from device_refit_bindings import decode_tree
from test_gpu_trace_refill_round import LIGHT_SPHERE, LIGHT_SPOT, LIGHT_HIT, MISS, SUN, Relit, light, random_rays

pytestmark = pytest.mark.gpu

COUNTS = [50000, 777, 64, 33, 1]


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
    """The 20 k-triangle atrium of tests/test_gpu_parity.py: all opaque, so the lean instantiations."""
    scene = Scene("atrium", param0=20000, param1=3)
    assert all_opaque(scene)
    return scene


def all_opaque(scene):
    return bool((scene.triangles()[:, 11] & 1).all())      # HiprTriangle::flags, HIPR_TRIANGLE_OPAQUE


def two_kinds(rng, n, lo, hi, triangle_count):
    closest = random_rays(rng, n, lo, hi)
    skip = np.full(n, MISS, np.uint32)
    skip[::5] = rng.integers(0, triangle_count, len(skip[::5]))
    shadow = random_rays(rng, n, lo, hi)
    shadow[:, 7] = rng.uniform(0.05, 30.0, n).astype(np.float32)
    return closest, skip, shadow


def product_launches_equal_the_oracle(ctx, oracle_q, scene, closest, skip, shadow):
    """The fused launch and the two launches of one kind, uninstrumented, against the oracle. Returns the oracle's (hits, transmittance)."""
    search = ctx.oracle_search()
    hits, _ = oracle_q.trace_closest(scene.desc, closest, skip, use_bvh=search, with_lights=True)
    transmittance, _ = oracle_q.trace_shadow(scene.desc, shadow, use_bvh=search)
    ctx.set_instrumentation(False)
    fused_hits, fused_transmittance = ctx.debug_trace_fused(closest, skip, shadow)
    assert np.array_equal(fused_hits.view(np.uint32), hits.view(np.uint32)), "t, u, v and primitive id must match bit for bit"
    assert np.array_equal(fused_transmittance.view(np.uint32), transmittance.view(np.uint32))
    assert np.array_equal(ctx.debug_trace_shadow(shadow).view(np.uint32), transmittance.view(np.uint32))
    assert np.array_equal(ctx.debug_trace_closest(closest, skip).view(np.uint32), hits.view(np.uint32))
    return hits, transmittance


@pytest.mark.parametrize("count", COUNTS)
def test_product_launches_on_the_opaque_atrium_match_oracle(ctx, oracle_q, atrium, count):
    ctx.upload_scene(atrium)
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    closest, skip, shadow = two_kinds(np.random.default_rng(9000 + count), count, -14.0, 14.0, atrium.desc.triangle_count)
    hits, transmittance = product_launches_equal_the_oracle(ctx, oracle_q, atrium, closest, skip, shadow)
    if count >= 777:
        assert 0.2 < (hits[:, 3].view(np.uint32) != MISS).mean() < 0.999
        assert 0.05 < (transmittance == 0).mean() < 0.99


def write_loose_triangles_obj(path, side=24):
    """side^2 triangles on a grid, three floors of them, no two sharing a corner: the builder can pair none of them. One opaque material (a file without one
    gets the loader's empty material, whose coverage is 0: not statically opaque)."""
    path.with_suffix(".mtl").write_text("newmtl solid\nKd 0.7 0.7 0.7\nd 1\n")
    lines, v = ["mtllib " + path.with_suffix(".mtl").name, "usemtl solid"], 0
    rng = np.random.default_rng(17)
    for floor in range(3):
        for i in range(side):
            for j in range(side):
                x, y, z = float(i), 1.5 * floor + float(rng.uniform(0.0, 0.4)), float(j)
                a, b = rng.uniform(0.5, 0.95, 2)
                lines += ["v %.9g %.9g %.9g" % (x, y, z), "v %.9g %.9g %.9g" % (x + a, y, z + 0.05), "v %.9g %.9g %.9g" % (x + 0.05, y + 0.2, z + b), "f %d %d %d" % (v + 1, v + 2, v + 3)]
                v += 3
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def test_a_scene_of_single_triangle_records_matches_oracle(ctx, oracle_q, tmp_path):
    side = 24
    scene = Scene("file:" + write_loose_triangles_obj(tmp_path / "loose.obj", side))
    slots = scene.wide8_slots()
    is_node, _ = decode_tree(slots)
    assert (~is_node).sum() == scene.desc.triangle_count == 3 * side * side and (slots[~is_node, 13] == MISS).all()      # one record per triangle, none with a B
    assert all_opaque(scene)
    ctx.upload_scene(scene)
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    rng = np.random.default_rng(23)
    n = 6000
    closest, skip, shadow = two_kinds(rng, n, 0.0, float(side), scene.desc.triangle_count)
    for rays in (closest, shadow):
        rays[:, 1] = rng.uniform(-1.0, 5.0, n).astype(np.float32)      # between, below and above the floors
    hits, transmittance = product_launches_equal_the_oracle(ctx, oracle_q, scene, closest, skip, shadow)
    assert 0.1 < (hits[:, 3].view(np.uint32) != MISS).mean() < 0.95
    assert 0.05 < (transmittance == 0).mean() < 0.95


SPHERE = dict(kind=LIGHT_SPHERE, position=(1.0, 4.0, 0.5), radius=1.5)
SPOT = dict(kind=LIGHT_SPOT, position=(-2.0, 5.0, 1.0), radius=2.0, direction=(0.0, -1.0, 0.0))
LIGHT_LISTS = {"sphere": [SUN, SPHERE], "spot": [SUN, SPOT], "sphere-and-spot": [SPHERE, SUN, SPOT]}


def rays_around(rng, l, n):
    """n rays aimed at the light's surface and a little past it, n that graze it (the sphere's tangent cone, the disk's rim; a millionth inside, on it, a millionth
    outside), n aimed at nothing."""
    centre, radius = np.array(l["position"], np.float64), l["radius"]
    aimed, grazing, loose = (random_rays(rng, n, -12.0, 12.0) for _ in range(3))
    target = centre + rng.uniform(-1.2, 1.2, size=(n, 3)) * radius
    d = target - aimed[:, 0:3]
    aimed[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    scale = rng.choice([1 - 1e-6, 1.0, 1 + 1e-6], (n, 1))
    if l["kind"] == LIGHT_SPHERE:
        to_centre = centre - grazing[:, 0:3]
        distance = np.linalg.norm(to_centre, axis=1, keepdims=True)
        along = to_centre / distance
        across = np.cross(along, rng.normal(size=(n, 3)))
        across /= np.linalg.norm(across, axis=1, keepdims=True)
        sine = np.minimum(1.0, radius * scale / distance)
        grazing[:, 4:7] = np.sqrt(1.0 - sine * sine) * along + sine * across
    else:
        rim = rng.normal(size=(n, 3))
        rim[:, 1] = 0.0                                       # the disk's normal is the y axis
        d = centre + radius * scale * rim / np.linalg.norm(rim, axis=1, keepdims=True) - grazing[:, 0:3]
        grazing[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    return [aimed, grazing, loose]


@pytest.mark.parametrize("name", list(LIGHT_LISTS))
def test_rays_that_hit_graze_and_miss_a_light_match_oracle(ctx, oracle_q, atrium, name):
    lights = LIGHT_LISTS[name]
    scene = Relit(atrium, [light(**l) for l in lights])
    ctx.upload_scene(scene)
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    rng = np.random.default_rng(41)
    n = 400
    analytic = [k for k, l in enumerate(lights) if l is not SUN]
    closest = np.concatenate([rays for k in analytic for rays in rays_around(rng, lights[k], n)])
    skip = np.full(len(closest), MISS, np.uint32)
    shadow = random_rays(rng, len(closest), -12.0, 12.0)
    shadow[:, 7] = rng.uniform(0.05, 30.0, len(shadow)).astype(np.float32)
    hits, _ = product_launches_equal_the_oracle(ctx, oracle_q, scene, closest, skip, shadow)
    ids = hits[:, 3].view(np.uint32)
    on_light = (ids != MISS) & ((ids & LIGHT_HIT) != 0)
    for i, k in enumerate(analytic):
        aimed, grazing, loose = (on_light[(3 * i + part) * n:(3 * i + part + 1) * n] & (ids[(3 * i + part) * n:(3 * i + part + 1) * n] == (LIGHT_HIT | k)) for part in range(3))
        assert 20 < aimed.sum() < n - 20, (name, k)          # some of the aimed rays reach the light, some are stopped or pass it by
        assert 5 < grazing.sum() < n - 5, (name, k)           # ... and of the grazing ones
        assert loose.mean() < 0.2, (name, k)                  # most rays meet no light: their waves branch over the second step


def test_the_textured_atrium_matches_oracle(ctx, oracle_q):
    """The coverage instantiation, whose statements are the parent's: a guard."""
    scene = Scene("atrium", param0=20000, param1=3, textured=True)
    assert not all_opaque(scene)
    ctx.upload_scene(scene)
    closest, skip, shadow = two_kinds(np.random.default_rng(51), 777, -14.0, 14.0, scene.desc.triangle_count)
    _, transmittance = product_launches_equal_the_oracle(ctx, oracle_q, scene, closest, skip, shadow)
    assert 0.05 < (transmittance == 0).mean() < 0.99


W, H, SPP = 48, 27, 4
_oracle_frames = {}


def render(context, scene, w, h, spp, bounces, wavefronts=0, instrumented=False):
    context.upload_scene(scene)
    context.set_instrumentation(instrumented)
    context.set_wavefront_count(wavefronts)
    try:
        context.set_frame(w, h, 0, 1, spp)
        context.reset_counters()
        context.render_pass(scene.camera(w, h, accumulations=0, max_bounce_count=bounces))
        context.synchronize()
        return context.read_accumulation(), context.counters()
    finally:
        context.set_wavefront_count(0)
        context.set_instrumentation(False)
        context.set_frame(w, h, 0, 1, 1)


@pytest.mark.parametrize("wavefronts", [1, 2])
@pytest.mark.parametrize("bounces", [0, 1, 4])
def test_exact_frames_equal_the_oracle_bit_for_bit(verify_ctx, oracle_q, atrium, bounces, wavefronts):
    ours, counters = render(verify_ctx, atrium, W, H, SPP, bounces, wavefronts)
    if bounces not in _oracle_frames:
        before = oracle_q.lib.oracle_set_f64_transcendentals(1)
        try:
            _oracle_frames[bounces], _, _ = oracle_q.render(atrium.desc, atrium.state, atrium.camera(W, H, max_bounce_count=bounces), W, H, SPP, use_bvh=verify_ctx.oracle_search())
        finally:
            oracle_q.lib.oracle_set_f64_transcendentals(before)
        _oracle_frames[bounces].setflags(write=False)
    theirs = _oracle_frames[bounces][..., :3]
    ours = ours[..., :3]
    assert np.isfinite(ours).all() and float(theirs.mean()) > 0.0 and counters["shadow_rays"] > 0
    assert np.array_equal(ours, theirs), f"{(ours != theirs).any(axis=-1).sum()} of {W * H} pixels differ"


def test_the_counting_kernels_frame_equals_the_products(ctx, atrium):
    """64 x 36, 4 samples, 4 bounces: the frame and the ray counters of the counting instantiations (the parent's record block and retire) and of the product's."""
    product, product_counters = render(ctx, atrium, 64, 36, 4, 4)
    counting, counting_counters = render(ctx, atrium, 64, 36, 4, 4, instrumented=True)
    assert np.isfinite(product).all() and float(product[..., :3].mean()) > 0
    assert np.array_equal(product.view(np.uint64), counting.view(np.uint64))
    for key in ("closest_rays", "shadow_rays", "shaded_hits", "camera_rays"):
        assert product_counters[key] == counting_counters[key] > 0, key
    assert counting_counters["closest_nodes"] > 0 and counting_counters["shadow_triangles"] > 0      # the counting kernels did count
