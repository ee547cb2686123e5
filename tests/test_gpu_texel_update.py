"""hipr_update_scene_texels on the GPU: a pixel edit of a resident image applied to the resident scene by kernels (csrc/texel_update.h over the flag rules of
csrc/material_rules.h) must leave, byte for byte, what a fresh hipr_upload_scene of the edited scene (Scene.update_texels, tests/test_texel_update_on_host_cpu.py) puts
there -- the texel pool, the triangles, the trace records, the leaf records, the search the context picks, the image -- and refuse what it cannot do before it touches
anything. Every refusal here is a check on the host that returns a status."""
import ctypes as C

import numpy as np
import pytest

import lighting_update_bindings as lu
import texel_update_bindings as tu
from bifrost3d_amd import capi
from bifrost3d_amd.host import Scene
from bifrost3d_amd.renderer import Context

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 36, 4
BUFFERS = capi.SCENE_BUFFERS + (capi.SCENE_BUFFER_TEXTURES, capi.SCENE_BUFFER_TEXELS)
LIGHTING = (capi.SCENE_BUFFER_LIGHTS, capi.SCENE_BUFFER_ENVIRONMENT_PDF, capi.SCENE_BUFFER_ENVIRONMENT_SAMPLES)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fresh():
    """The second context: takes a fresh upload of the edited scene."""
    c = Context(0)
    yield c
    c.close()


def render(ctx, scene, spp=SPP):
    ctx.set_frame(W, H)
    for a in range(spp):
        ctx.render_pass(scene.camera(W, H, accumulations=a, max_bounce_count=4), synchronize=True)
    return ctx.read_accumulation()


def buffers(ctx, which=BUFFERS):
    return {b: ctx.read_scene_buffer(b) for b in which}


def unequal(a, b):
    return [which for which in a if a[which].shape != b[which].shape or not np.array_equal(a[which], b[which])]


def status_of(ctx, edits, group=None, null_edits=False, null_out=False):
    """The raw status of hipr_update_scene_texels (the refusals), or of hipr_group_update_scene_texels on the HiprGroup handle `group`."""
    array, keep = capi.texel_edits(edits)
    result = capi.HiprTexelUpdateResult()
    call, handle = (ctx.lib.hipr_group_update_scene_texels, group) if group is not None else (ctx.lib.hipr_update_scene_texels, ctx.handle)
    return call(handle, None if null_edits else array, max(len(keep), int(null_edits)), None if null_out else C.byref(result))


def applied_on_both(ctx, fresh, scene, edits):
    """The edits on the device of `ctx`, in the builder of `scene`, and the edited scene uploaded to `fresh`; the device's answer."""
    answer = ctx.update_scene_texels(edits)
    assert answer["status"] == capi.HIPR_OK, ctx.lib.hipr_last_error()
    assert scene.update_texels(edits) is True
    fresh.upload_scene(scene)
    return answer


@pytest.mark.parametrize("name", tu.CASE_IDS)
def test_buffers_search_and_image_equal_a_fresh_uploads(ctx, fresh, name):
    _, v, steps = tu.case(name)
    scene, info = tu.make_scene(v)
    ctx.upload_scene(scene)
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    for edits, expectation in steps:
        before, flags_before, held_before = tu.opaque(scene, info), scene.triangles()[:, 11], buffers(ctx)
        answer = applied_on_both(ctx, fresh, scene, tu.coverage_edits(info, edits))
        after, flags_after = tu.opaque(scene, info), scene.triangles()[:, 11]
        tu.check_expectation(expectation, before, after)
        held = buffers(ctx)
        assert unequal(held, buffers(fresh)) == []
        assert np.array_equal(held[capi.SCENE_BUFFER_TRIANGLES], scene.triangles()) and np.array_equal(held[capi.SCENE_BUFFER_WIDE8_SLOTS], scene.wide8_slots())
        assert ctx.trace_variant() == fresh.trace_variant()
        # the answer against the builder's count, never the library's own
        assert answer["changed_triangles"] == int((flags_before != flags_after).sum()) and answer["candidate_triangles"] >= answer["changed_triangles"]
        assert answer["all_triangles_opaque"] == bool((flags_after & capi.TRIANGLE_OPAQUE != 0).all()) and not answer["environment_stale"]
        if expectation == "none":
            assert answer["changed_triangles"] == 0 and unequal(held, held_before) == [capi.SCENE_BUFFER_TEXELS]
    assert np.array_equal(render(ctx, scene).view(np.uint64), render(fresh, scene).view(np.uint64))


def test_the_filled_hole_gives_back_the_uploaded_bytes_and_the_search_without_coverage(ctx, fresh):
    _, v, steps = tu.case("hole_nearest_r8")
    scene, info = tu.make_scene(v)
    ctx.upload_scene(scene)
    uploaded, image = buffers(ctx), render(ctx, scene)
    punched = applied_on_both(ctx, fresh, scene, tu.coverage_edits(info, steps[0][0]))
    assert not punched["all_triangles_opaque"] and punched["changed_triangles"] == 8      # the four cells whose boxes [4 i - 1, 4 i + 5] hold texel 13
    with_hole = render(ctx, scene)
    assert np.array_equal(with_hole.view(np.uint64), render(fresh, scene).view(np.uint64))
    filled = applied_on_both(ctx, fresh, scene, tu.coverage_edits(info, steps[1][0]))
    assert filled["all_triangles_opaque"] and filled["changed_triangles"] == 8
    assert unequal(buffers(ctx), uploaded) == []
    assert np.array_equal(render(ctx, scene).view(np.uint64), image.view(np.uint64))
    print("times of the last update (ms):", ctx.texel_update_times())


@pytest.mark.parametrize("tint", [tu.R32F, tu.RGBA32F], ids=["r32f", "rgba32f"])
def test_a_float_tint_texture_lands_in_the_pool_and_shows_in_the_image(ctx, fresh, tint):
    v = tu.variant(tint=tint)
    scene, info = tu.make_scene(v)
    ctx.upload_scene(scene)
    held_before, image = buffers(ctx), render(ctx, scene)
    pixels = np.zeros((8, 8) if tint == tu.R32F else (8, 8, 4), np.float32)
    answer = applied_on_both(ctx, fresh, scene, [(info["textures"]["tint"], 0, 0, pixels)])
    assert (answer["candidate_triangles"], answer["changed_triangles"], answer["all_triangles_opaque"]) == (0, 0, True)
    held = buffers(ctx)
    assert unequal(held, buffers(fresh)) == [] and unequal(held, held_before) == [capi.SCENE_BUFFER_TEXELS]
    updated = render(ctx, scene)
    assert np.array_equal(updated.view(np.uint64), render(fresh, scene).view(np.uint64)) and not np.array_equal(updated, image)


def test_a_pitch_beyond_the_row_and_two_textures_in_one_call(ctx, fresh):
    _, v, _ = tu.case("hole_nearest_r8")
    scene, info = tu.make_scene(v)
    ctx.upload_scene(scene)
    wide = np.full((4, 11), 77, np.uint8)       # rows of 11 bytes of which 6 are the rectangle's
    wide[:, :6] = np.arange(24, dtype=np.uint8).reshape(4, 6)
    edits = [(info["textures"]["coverage"], 21, 2, 6, 4, wide, 11), (info["textures"]["unrelated"], 13, 14, np.full((2, 3, 4), 9, np.uint8))]
    answer = applied_on_both(ctx, fresh, scene, edits)
    assert answer["changed_triangles"] > 0
    held = buffers(ctx)
    assert unequal(held, buffers(fresh)) == [] and 77 not in held[capi.SCENE_BUFFER_TEXELS][scene.desc.textures[info["textures"]["coverage"]].texel_offset:][:32 * 32]


def test_an_edited_sky_is_reported_stale_and_rebuilt_by_the_lighting_update(ctx, fresh):
    sky = np.random.default_rng(4).integers(0, 256, (32, 64, 4), dtype=np.uint8)
    sky[..., 3] = 255
    keywords = dict(width=64, height=32, texel_format=tu.RGBA8, linear=(True, True), repeat=(True, False))
    scene = Scene("cornell", param0=4)
    index = scene.add_environment(sky, sample_count=1024, **keywords)
    scene.rebuild()
    ctx.upload_scene(scene)
    sun = np.full((5, 9, 4), 255, np.uint8)
    answer = ctx.update_scene_texels([(index, 30, 8, sun)])
    assert answer["status"] == capi.HIPR_OK and answer["environment_stale"] and answer["changed_triangles"] == 0
    assert scene.update_texels([(index, 30, 8, sun)]) is True and scene.environment_stale
    lights = lu.own_lights(scene)
    updated = ctx.update_scene_lighting(lights, capi.ENVIRONMENT_BUILD, scene.staged_environment_build(index, 1024))
    assert updated["status"] == capi.HIPR_OK and scene.adopt_lighting(lights, capi.ENVIRONMENT_BUILD, index, updated)
    anew = Scene("cornell", param0=4)
    assert anew.add_environment(tu.painted(sky, 30, 8, sun), sample_count=1024, **keywords) == index
    anew.rebuild()
    fresh.upload_scene(anew)
    assert unequal(buffers(ctx, BUFFERS + LIGHTING), buffers(fresh, BUFFERS + LIGHTING)) == []
    assert np.array_equal(render(ctx, scene).view(np.uint64), render(fresh, anew).view(np.uint64))


def test_refusals_leave_everything_as_it_was(ctx):
    lib = ctx.lib
    one = np.zeros((1, 1), np.uint8)
    # no scene uploaded
    empty = Context(0)
    try:
        assert status_of(empty, [(1, 0, 0, one)]) == capi.HIPR_ERROR_NOT_READY
    finally:
        empty.close()
    # a scene that carries the exhaustive search's items: its coverage texture is refused, its other textures are served
    small = Scene("cornell", param0=1)
    unrelated = small.add_texture(tu.UNRELATED, 16, 16, tu.RGBA8, is_sRGB=True)
    coverage = small.add_texture(np.full((8, 8), 255, np.uint8), 8, 8, tu.R8, linear=(False, False))
    small.insert_model(1000, small.add_mesh(**tu.tessellated_quad(1, tu.UNIT)), small.add_material(tu.pg.material(flags=capi.MATERIAL_THIN_WALLED | capi.MATERIAL_CUTOUT, coverage=0.5, coverage_texture=coverage)),
                       model_index=202, **tu.pg.BESIDE_IT)
    small.rebuild()
    assert small.desc.triangle_count == 36
    ctx.upload_scene(small)
    assert ctx.trace_variant() == capi.TRACE_EXHAUSTIVE
    image, held = render(ctx, small), buffers(ctx)
    assert status_of(ctx, [(unrelated, 0, 0, np.zeros((1, 1, 4), np.uint8)), (coverage, 3, 3, one)]) == capi.HIPR_ERROR_UNSUPPORTED
    assert b"upload" in lib.hipr_last_error()
    assert small.update_texels([(coverage, 3, 3, one)]) is False
    assert unequal(buffers(ctx), held) == [] and np.array_equal(render(ctx, small), image)
    served = ctx.update_scene_texels([(unrelated, 0, 0, np.zeros((1, 1, 4), np.uint8))])
    assert served["status"] == capi.HIPR_OK and unequal(buffers(ctx), held) == [capi.SCENE_BUFFER_TEXELS]

    _, v, _ = tu.case("hole_nearest_r8")
    scene, info = tu.make_scene(v)
    ctx.upload_scene(scene)
    image, held = render(ctx, scene), buffers(ctx)
    texture = info["textures"]["coverage"]
    good = (texture, 13, 13, one)
    refused = [
        status_of(ctx, [good], null_out=True),
        status_of(ctx, [good], null_edits=True),
        status_of(ctx, [good, (texture, 0, 0, 1, 1, None, 1)]),                            # null texels
        status_of(ctx, [good, (0, 0, 0, one)]),                                            # texture 0
        status_of(ctx, [good, (scene.desc.texture_count, 0, 0, one)]),                     # outside the resident pool
        status_of(ctx, [good, (texture, 0, 0, 0, 1, one, 1)]),                             # no width
        status_of(ctx, [good, (texture, 0, 0, 1, 0, one, 1)]),                             # no height
        status_of(ctx, [good, (texture, 32, 0, one)]),                                     # begins outside
        status_of(ctx, [good, (texture, 31, 0, np.zeros((1, 2), np.uint8))]),              # reaches outside
        status_of(ctx, [good, (texture, 0, 30, np.zeros((3, 1), np.uint8))]),
        status_of(ctx, [good, (texture, 0xFFFFFFFF, 0, 2, 1, np.zeros((1, 2), np.uint8), 2)]),      # x + width wraps around 32 bits
        status_of(ctx, [good, (texture, 0, 0, 4, 1, np.zeros((1, 4), np.uint8), 3)]),      # a pitch below the row's bytes
        status_of(ctx, [good, (info["textures"]["unrelated"], 0, 0, 4, 1, np.zeros((1, 4, 4), np.uint8), 15)]),
    ]
    assert refused == [capi.HIPR_ERROR_INVALID_ARGUMENT] * len(refused), refused
    assert unequal(buffers(ctx), held) == [] and np.array_equal(render(ctx, scene), image)
    # an empty list is served and changes nothing
    assert status_of(ctx, []) == capi.HIPR_OK and unequal(buffers(ctx), held) == []
    # nothing is stale after a texel update: the other searches may still be asked for
    assert status_of(ctx, [good]) == capi.HIPR_OK
    assert lib.hipr_set_trace_variant(ctx.handle, capi.TRACE_BVH2) == 0
    ctx.set_trace_variant(-1)


def test_a_group_of_one_device_updates_like_a_single_context(ctx, fresh):
    lib = ctx.lib
    _, v, steps = tu.case("hole_nearest_r8")
    scene, info = tu.make_scene(v)
    edits = tu.coverage_edits(info, steps[0][0])
    devices = (C.c_int * 1)(0)
    group = C.c_void_p()
    assert lib.hipr_group_create(devices, 1, C.byref(group)) == 0
    member = Context.__new__(Context)      # a handle on the group's member 0, for the read-backs; the group owns the context
    member.lib, member.handle, member._scene = lib, C.c_void_p(), scene
    try:
        tables = capi.load_tables()
        t = capi.HiprTables(*[a.ctypes.data_as(C.POINTER(C.c_float)) for a in tables])
        assert lib.hipr_group_upload_tables(group, C.byref(t)) == 0
        assert status_of(ctx, edits, group=group) == capi.HIPR_ERROR_NOT_READY
        assert lib.hipr_group_upload_scene(group, C.byref(scene.desc)) == 0
        member.handle = C.c_void_p(lib.hipr_group_context(group, 0))
        uploaded = buffers(member)
        assert status_of(ctx, edits + [(info["textures"]["coverage"], 32, 0, np.zeros((1, 1), np.uint8))], group=group) == capi.HIPR_ERROR_INVALID_ARGUMENT
        assert status_of(ctx, edits, group=group, null_out=True) == capi.HIPR_ERROR_INVALID_ARGUMENT
        assert unequal(buffers(member), uploaded) == []
        answer = ctx.update_scene_texels(edits, group=group)
        assert answer["status"] == capi.HIPR_OK and answer["changed_triangles"] == 8
        assert scene.update_texels(edits) is True
        fresh.upload_scene(scene)
        assert unequal(buffers(member), buffers(fresh)) == []
    finally:
        member.handle = C.c_void_p()      # nothing of the group's is closed through the borrowed handle
        lib.hipr_group_destroy(group)
