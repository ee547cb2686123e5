"""hipr_update_scene_lighting on the GPU (csrc/environment_build.h): the light list of the resident scene replaced -- any count, any types -- and its environment kept,
removed or rebuilt by kernels from the texture the resident texel pool holds must leave, byte for byte, what the host path leaves on a fresh context:
SceneBuilder::add_light, InfiniteAreaLight + presample_environment + set_environment, rebuild(), hipr_upload_scene. Every equality is of bytes: the light buffer, the
environment's PDF image and samples, the result, the switches, and the images of both arithmetic modes; every refusal is an argument error that leaves the resident
scene as the call found it."""
import ctypes as C

import numpy as np
import pytest

import device_rebuild_bindings as rb
import lighting_update_bindings as lu
from bifrost3d_amd import capi
from bifrost3d_amd.renderer import Context
from test_gpu_device_rebuild import H, SPP, W, buffers, not_ready, render, unequal
from test_gpu_pool_growth import pool_buffers, unequal_pools

pytestmark = pytest.mark.gpu

KEEP, REMOVE, BUILD = capi.ENVIRONMENT_KEEP, capi.ENVIRONMENT_REMOVE, capi.ENVIRONMENT_BUILD


@pytest.fixture(scope="module", params=["fast", "exact"])
def pair(request):
    """(the context the edits go to, the context of the host path: it only ever takes uploads), both in one arithmetic mode."""
    mine, fresh = Context(0, arithmetic=request.param), Context(0, arithmetic=request.param)
    yield mine, fresh
    mine.close()
    fresh.close()


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fresh():
    c = Context(0)
    yield c
    c.close()


def everything(context):
    return buffers(context), pool_buffers(context), lu.lighting_buffers(context)


def all_unequal(mine, theirs):
    """Every readable buffer of two contexts: the scene arrays, the pools, the three buffers the lighting update writes."""
    a, b = everything(mine), everything(theirs)
    return unequal(a[0], b[0]) + unequal_pools(a[1], b[1]) + lu.unequal_lighting(a[2], b[2])


def scene_with_textures(*names):
    """A built scene that holds the maps' textures and no environment: what is resident before a build."""
    scene, indices = rb.make_scene(lu.CORNELL), []
    for name in names:
        m = lu.MAPS[name]
        indices.append(scene.add_texture(m["pixels"], m["width"], m["height"], m["texel_format"], m.get("is_sRGB", False), repeat=m["repeat"], linear=m["linear"]))
    scene.rebuild()
    return scene, indices


def host_with(textures_before, environment, sample_count=1024):
    """The host path's scene: the textures before the environment's as plain textures, then the environment (None: none) through InfiniteAreaLight +
    presample_environment + set_environment, then rebuild()."""
    scene = rb.make_scene(lu.CORNELL)
    for name in textures_before:
        m = lu.MAPS[name]
        scene.add_texture(m["pixels"], m["width"], m["height"], m["texel_format"], m.get("is_sRGB", False), repeat=m["repeat"], linear=m["linear"])
    if environment is not None:
        scene.add_environment(sample_count=sample_count, **lu.MAPS[environment])
    scene.rebuild()
    return scene


def held_to(mine, fresh, updated, host, staged):
    """The device's outcome `updated` on `mine` against a fresh upload of the host path's `host`; `staged` draws the image on `mine` (the camera is the scene's)."""
    fresh.upload_scene(host)
    assert updated["status"] == capi.HIPR_OK, mine.lib.hipr_last_error()
    assert all_unequal(mine, fresh) == []
    d = host.desc
    e = lu.environment_of(d)
    assert (updated["pdf_width"], updated["pdf_height"], updated["sample_count"]) == (e["extent"] if e else (0, 0, 0))
    assert updated["light_count"] == d.light_count and updated["switches"] == lu.expected_switches(d)
    assert np.array_equal(render(mine, staged).view(np.uint64), render(fresh, host).view(np.uint64))


@pytest.mark.parametrize("name, sample_count", lu.BUILDS, ids=lu.BUILD_IDS)
def test_an_environment_built_on_the_device_is_the_host_paths(pair, name, sample_count):
    mine, fresh = pair
    staged, (index,) = scene_with_textures(name)
    host = host_with([], name, sample_count)
    mine.upload_scene(staged)
    assert mine.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    before = render(mine, staged)
    updated = mine.update_scene_lighting(lu.own_lights(staged), BUILD, staged.staged_environment_build(index, sample_count))
    held_to(mine, fresh, updated, host, staged)
    black = name == "32x16_all_black"
    assert updated["disabled"] == black and (updated["light_count"] == len(lu.own_lights(staged)) + (0 if black else 1))
    e = lu.environment_of(host.desc)
    assert np.array_equal(updated["per_pixel_PDF"].view(np.uint32), e["pdf"]) and np.array_equal(updated["samples"].view(np.uint32), e["samples"])
    after = render(mine, staged)
    print(f"{name}, {sample_count} samples: {int((after != before).any(axis=-1).sum())} of {W * H} pixels differ from the image before; times {mine.lighting_times()}")
    assert black or not np.array_equal(after, before)
    # the builder follows without a rebuild
    assert staged.adopt_lighting(lu.own_lights(staged), BUILD, index, updated)
    assert rb.differences(rb.description(host), rb.description(staged)) == []


@pytest.mark.parametrize("environment", [None, "64x32_float_linear"], ids=["no environment", "environment kept"])
@pytest.mark.parametrize("which", lu.LIST_IDS)
def test_a_light_list_replaced_on_the_device_is_a_fresh_upload_of_the_list(pair, which, environment):
    mine, fresh = pair
    scene = host_with([], environment)
    lights = lu.light_lists(scene)[which]
    mine.upload_scene(scene)
    before = render(mine, scene)
    updated = mine.update_scene_lighting(lights, KEEP)
    held_to(mine, fresh, updated, lu.with_lights(host_with([], environment), lights), scene)
    assert updated["light_count"] == len(lights) + (1 if environment else 0) and not updated["disabled"]
    assert not np.array_equal(render(mine, scene), before)


def test_a_light_added_is_add_light_and_a_rebuild(ctx, fresh):
    """The host path in full for the one edit it has a call for: SceneBuilder::add_light + rebuild()."""
    scene, host = rb.make_scene(lu.CORNELL), rb.make_scene(lu.CORNELL)
    lamp = lu.sphere_light((0.1, 0.25, -0.2))
    host.add_light(lamp)
    host.rebuild()
    ctx.upload_scene(scene)
    updated = ctx.update_scene_lighting(lu.own_lights(scene) + [lamp], KEEP)
    held_to(ctx, fresh, updated, host, scene)
    assert scene.adopt_lighting(lu.own_lights(scene) + [lamp], KEEP, updated=updated)
    assert rb.differences(rb.description(host), rb.description(scene)) == []


def test_an_environment_set_then_replaced_then_removed(pair):
    mine, fresh = pair
    first, second = "67x130_float_nearest", "65x128_srgb_one_white"
    staged, (a, b) = scene_with_textures(first, second)
    lights = lu.own_lights(staged)
    mine.upload_scene(staged)
    updated = mine.update_scene_lighting(lights, BUILD, staged.staged_environment_build(a, 1024))
    host = rb.make_scene(lu.CORNELL)      # the first map as the environment, the second as a plain texture behind it
    host.add_environment(sample_count=1024, **lu.MAPS[first])
    m = lu.MAPS[second]
    host.add_texture(m["pixels"], m["width"], m["height"], m["texel_format"], m.get("is_sRGB", False), repeat=m["repeat"], linear=m["linear"])
    host.rebuild()
    held_to(mine, fresh, updated, host, staged)
    # replaced, with a lamp more in the same call
    more = lights + [lu.sphere_light((0.1, 0.25, -0.2))]
    updated = mine.update_scene_lighting(more, BUILD, staged.staged_environment_build(b, 256))
    held_to(mine, fresh, updated, lu.with_lights(host_with([first], second, 256), more), staged)
    # removed: the constant tint again, the textures stay
    updated = mine.update_scene_lighting(lights, REMOVE)
    held_to(mine, fresh, updated, scene_with_textures(first, second)[0], staged)
    assert (updated["pdf_width"], updated["sample_count"], updated["light_count"]) == (0, 0, len(lights))
    assert all(len(b) == 0 for b in lu.lighting_buffers(mine)[1:])


def test_the_environments_texture_comes_by_a_pool_growth_first(ctx, fresh):
    name = "63x129_float_nearest"
    scene = rb.make_scene(lu.CORNELL)
    ctx.upload_scene(scene)
    m = lu.MAPS[name]
    index = scene.add_texture(m["pixels"], m["width"], m["height"], m["texel_format"], repeat=m["repeat"], linear=m["linear"])
    build = scene.staged_environment_build(index, 1024)
    # not resident yet: refused
    assert ctx.update_scene_lighting(lu.own_lights(scene), BUILD, build, read_back=False)["status"] == capi.HIPR_ERROR_INVALID_ARGUMENT
    growth, edits = scene.staged_scene_growth()
    assert ctx.append_scene_pools(growth) == capi.HIPR_OK, ctx.lib.hipr_last_error()
    updated = ctx.update_scene_lighting(lu.own_lights(scene), BUILD, build)
    held_to(ctx, fresh, updated, host_with([], name), scene)


def test_life_after_a_lighting_update(ctx, fresh):
    name = "64x32_float_linear"
    staged, (index,) = scene_with_textures(name)
    lights = lu.own_lights(staged) + [lu.sphere_light((0.1, 0.25, -0.2))]
    ctx.upload_scene(staged)
    updated = ctx.update_scene_lighting(lights, BUILD, staged.staged_environment_build(index, 1024))
    assert updated["status"] == capi.HIPR_OK and staged.adopt_lighting(lights, BUILD, index, updated)
    # a refit that moves a model and a lamp: the count is the new one, the environment's light included
    moved = [capi.HiprLight.from_buffer_copy(bytes(light)) for light in staged.lights()]
    moved[1].data[4] = 0.3
    pose = dict(translation=(0.05, 0.0, 0.02))
    refitted = ctx.refit_scene_transforms(staged.model_pose(6, **pose), lights=moved)
    assert not refitted["needs_rebuild"]
    assert staged.move_model(6, rebuild_threshold=1e30, **pose) is True and staged.set_lights(moved[:-1])
    assert np.array_equal(ctx.read_scene_buffer(capi.SCENE_BUFFER_LIGHTS), rb.description(staged)["lights"])
    # a material edit, then a geometry update with the adopted description
    materials = staged.materials()
    materials[2].roughness = 0.9
    ctx.update_scene_materials([(2, materials[2])])
    assert staged.update_materials([(2, materials[2])]) is True
    ctx.update_scene_geometry(staged)
    fresh.upload_scene(staged)
    assert all_unequal(ctx, fresh) == []
    assert np.array_equal(render(ctx, staged).view(np.uint64), render(fresh, staged).view(np.uint64))
    # an instance edit over the lit scene
    assert staged.remove_model(5)
    edited = ctx.edit_scene_instances(staged.staged_instance_edits())
    assert edited["status"] == capi.HIPR_OK, ctx.lib.hipr_last_error()
    assert staged.adopt_edited_trees(edited["nodes"], edited["order"], edited["deepest"], edited["slots"], edited["wide8"])
    assert lu.unequal_lighting(lu.lighting_buffers(ctx), lu.lighting_buffers(fresh)) == []
    # a second lighting update: the first list again, the environment removed
    updated = ctx.update_scene_lighting(lights[:1], REMOVE)
    assert updated["status"] == capi.HIPR_OK and staged.adopt_lighting(lights[:1], REMOVE, updated=updated)
    fresh.upload_scene(staged)
    mine, theirs = everything(ctx), everything(fresh)
    assert unequal(mine[0][:7], theirs[0][:7]) == [] and unequal_pools(mine[1], theirs[1]) == [] and lu.unequal_lighting(mine[2], theirs[2]) == []      # the BVH2 nodes are the ones the edit leaves
    assert np.array_equal(render(ctx, staged).view(np.uint64), render(fresh, staged).view(np.uint64))


def test_an_update_after_a_refit_that_awaits_a_rebuild_leaves_that_state(ctx, tmp_path):
    import device_refit_bindings as refit
    scene = refit.scene_with_a_parting_pair(tmp_path / "pair.obj")
    ctx.upload_scene(scene)
    assert ctx.refit_scene_transforms(scene.model_pose(1, **refit.LARGE_POSE))["needs_rebuild"]
    assert not_ready(ctx, scene)
    updated = ctx.update_scene_lighting([lu.sphere_light((0.0, 2.0, 0.0))], KEEP)
    assert updated["status"] == capi.HIPR_OK and updated["light_count"] == 1
    assert not_ready(ctx, scene)      # still awaiting the rebuild ...
    assert ctx.rebuild_scene_trees()["status"] == capi.HIPR_OK      # ... which the scene still takes
    assert not not_ready(ctx, scene)


def test_refusals_leave_the_buffers_and_a_render_as_before(ctx):
    INVALID, UNSUPPORTED = capi.HIPR_ERROR_INVALID_ARGUMENT, capi.HIPR_ERROR_UNSUPPORTED
    lib = ctx.lib
    scene, (linear, srgb) = scene_with_textures("67x130_float_nearest", "65x128_srgb_one_white")
    r8 = scene.add_texture(np.full((4, 4), 200, np.uint8), 4, 4, capi.TEXEL_R8, linear=(False, False))
    scene.rebuild()
    lights = lu.own_lights(scene)
    array = (capi.HiprLight * len(lights))(*lights)
    keep = []

    def floats(values):
        keep.append(np.ascontiguousarray(values, np.float32))
        return keep[-1].ctypes.data_as(C.POINTER(C.c_float))

    def owned(staged):
        """A copy of a staged description over arrays of its own: the builder's staging holds until the next one only."""
        b = capi.HiprEnvironmentBuild.from_buffer_copy(bytes(staged))
        b.row_sines = floats(np.ctypeslib.as_array(staged.row_sines, shape=(staged.pdf_height,)).copy())
        b.draw_points = floats(np.ctypeslib.as_array(staged.draw_points, shape=(2 * staged.sample_count,)).copy())
        if staged.srgb_decode:
            b.srgb_decode = floats(np.ctypeslib.as_array(staged.srgb_decode, shape=(256,)).copy())
        return b

    good, good_srgb = owned(scene.staged_environment_build(linear, 64)), owned(scene.staged_environment_build(srgb, 64))
    table = np.ctypeslib.as_array(good_srgb.srgb_decode, shape=(256,)).copy()
    sines = np.ctypeslib.as_array(good.row_sines, shape=(good.pdf_height,)).copy()
    points = np.ctypeslib.as_array(good.draw_points, shape=(128,)).copy()
    result = capi.HiprLightingResult()
    pdf, samples = np.zeros(67 * 130, np.float32), np.zeros((64, 8), np.float32)

    def call(lights=array, count=len(lights), action=BUILD, build=good, pdf_room=len(pdf), sample_room=len(samples), out=result, context=ctx):
        return lib.hipr_update_scene_lighting(context.handle, lights, count, action, C.byref(build) if build is not None else None, pdf.ctypes.data_as(C.POINTER(C.c_float)), pdf_room,
                                              C.cast(samples.ctypes.data, C.POINTER(capi.HiprLightSample)), sample_room, C.byref(out) if out is not None else None)

    def changed(base=good, **fields):
        b = capi.HiprEnvironmentBuild.from_buffer_copy(bytes(base))
        for field, value in fields.items():
            setattr(b, field, value)
        return b

    def with_value(array, at, value):
        copy = array.copy()
        copy[at] = value
        return floats(copy)

    # no scene: not ready, and still not ready afterwards
    empty = Context(0)
    try:
        assert call(context=empty, action=KEEP, build=None) == capi.HIPR_ERROR_NOT_READY
        assert not_ready(empty, scene)
    finally:
        empty.close()
    ctx.upload_scene(scene)
    kept, before = everything(ctx), render(ctx, scene)
    environment_light = capi.HiprLight()
    environment_light.flags = capi.LIGHT_PRESAMPLED_ENVIRONMENT
    refused = [
        ("a null result", dict(out=None), INVALID),
        ("a null array with a count", dict(lights=None, count=2), INVALID),
        ("the environment's light in the list", dict(lights=(capi.HiprLight * 2)(lights[0], environment_light), count=2), INVALID),
        ("an action outside the enum", dict(action=3, build=None), INVALID), ("a negative action", dict(action=-1, build=None), INVALID),
        ("a build without a description", dict(build=None), INVALID), ("a description with KEEP", dict(action=KEEP), INVALID), ("a description with REMOVE", dict(action=REMOVE), INVALID),
        ("texture 0", dict(build=changed(environment_map_ID=0)), INVALID), ("a negative texture", dict(build=changed(environment_map_ID=-1)), INVALID),
        ("a texture outside the resident pool", dict(build=changed(environment_map_ID=scene.desc.texture_count)), INVALID),
        ("another pdf_height", dict(build=changed(pdf_height=128)), INVALID), ("pdf_height below 128", dict(build=changed(good_srgb, pdf_height=127)), INVALID),
        ("null row_sines", dict(build=changed(row_sines=None)), INVALID), ("null draw_points", dict(build=changed(draw_points=None)), INVALID),
        ("no table for an sRGB texture", dict(build=changed(good_srgb, srgb_decode=None)), INVALID), ("a table for a linear texture", dict(build=changed(srgb_decode=good_srgb.srgb_decode)), INVALID),
        ("48 samples", dict(build=changed(sample_count=48)), INVALID), ("one sample", dict(build=changed(sample_count=1)), INVALID), ("no samples", dict(build=changed(sample_count=0)), INVALID),
        ("a draw point of 1", dict(build=changed(draw_points=with_value(points, 77, 1.0))), INVALID), ("a negative draw point", dict(build=changed(draw_points=with_value(points, 0, -1e-9))), INVALID),
        ("a draw point that is no number", dict(build=changed(draw_points=with_value(points, 127, np.nan))), INVALID),
        ("an infinite sine", dict(build=changed(row_sines=with_value(sines, 129, np.inf))), INVALID), ("a sine that is no number", dict(build=changed(row_sines=with_value(sines, 0, np.nan))), INVALID),
        ("a table entry that is no number", dict(build=changed(good_srgb, srgb_decode=with_value(table, 255, np.nan))), INVALID),
        ("too little room for the PDF image", dict(pdf_room=67 * 130 - 1), INVALID), ("too little room for the samples", dict(sample_room=63), INVALID),
        ("a single-channel texture", dict(build=changed(environment_map_ID=r8, pdf_height=128)), UNSUPPORTED),
    ]
    for what, arguments, status in refused:
        assert call(**arguments) == status, what
        assert lib.hipr_last_error()
        assert not not_ready(ctx, scene), what
    now = everything(ctx)
    assert unequal(kept[0], now[0]) == [] and unequal_pools(kept[1], now[1]) == [] and lu.unequal_lighting(kept[2], now[2]) == []
    assert np.array_equal(render(ctx, scene), before)
    assert not pdf.any() and not samples.any() and bytes(result) == bytes(capi.HiprLightingResult())
    # the sound calls are accepted after all of that
    assert call() == capi.HIPR_OK and call(build=good_srgb, pdf_room=65 * 128) == capi.HIPR_OK and result.pdf_width == 65


def test_a_group_of_one_member_updates_like_a_single_context(ctx):
    lib = ctx.lib
    name = "65x129_float_linear"
    scene, (index,) = scene_with_textures(name)
    lights = lu.own_lights(scene) + [lu.sphere_light((0.1, 0.25, -0.2))]
    ctx.upload_scene(scene)
    single = ctx.update_scene_lighting(lights, BUILD, scene.staged_environment_build(index, 1024))
    assert single["status"] == capi.HIPR_OK
    image = render(ctx, scene)
    devices = (C.c_int * 1)(0)
    group = C.c_void_p()
    assert lib.hipr_group_create(devices, 1, C.byref(group)) == 0
    try:
        tables = capi.load_tables()
        t = capi.HiprTables(*[a.ctypes.data_as(C.POINTER(C.c_float)) for a in tables])
        assert lib.hipr_group_upload_tables(group, C.byref(t)) == 0
        assert lib.hipr_group_upload_scene(group, C.byref(scene.desc)) == 0
        state = scene.state
        assert lib.hipr_group_set_scene_state(group, C.byref(state)) == 0
        assert lib.hipr_group_set_frame(group, W, H, 1) == 0
        # a call one member refuses leaves the group as it was ...
        bad = scene.staged_environment_build(index, 1024)
        bad.sample_count = 48
        assert ctx.update_scene_lighting(lights, BUILD, bad, group=group, capacities=(65 * 129, 1024))["status"] == capi.HIPR_ERROR_INVALID_ARGUMENT
        # ... and the sound one is applied on every member
        updated = ctx.update_scene_lighting(lights, BUILD, scene.staged_environment_build(index, 1024), group=group, capacities=(65 * 129, 1024))
        assert updated["status"] == capi.HIPR_OK, lib.hipr_last_error()
        assert bytes(updated["result"]) == bytes(single["result"]) and np.array_equal(updated["per_pixel_PDF"].view(np.uint32), single["per_pixel_PDF"].view(np.uint32))
        assert np.array_equal(updated["samples"].view(np.uint32), single["samples"].view(np.uint32))
        for a in range(SPP):
            cam = scene.camera(W, H, accumulations=a, max_bounce_count=4)
            assert lib.hipr_group_trace_pass(group, C.byref(cam)) == 0
            assert lib.hipr_group_accumulate_samples(group, 0, 1, a, None, 0, 1) == 0
        accumulation = np.zeros((H, W, 4), np.float64)
        assert lib.hipr_group_read_accumulation(group, accumulation.ctypes.data_as(C.POINTER(C.c_double)), W * H) == 0
    finally:
        lib.hipr_group_destroy(group)
    assert np.array_equal(accumulation.view(np.uint64), image.view(np.uint64))


def test_a_lamp_and_an_environment_through_the_renderer_class():
    """tests/native/LightingUpdateTest.cpp: with HIPR_DEVICE_LIGHTING=1 HIPRenderer::Renderer replaces the resident light list and builds the environment on the
    device, counts the tick, uploads nothing further and gives the frame of the host path bit for bit; with the variable unset the counter stays 0."""
    import subprocess
    from pathlib import Path
    binary = Path(__file__).resolve().parent / "native" / "renderer_test"
    assert binary.exists(), f"{binary} is missing: run __graft_entry__.build()"
    p = subprocess.run([str(binary), "--gpu", "LightingUpdateFixture"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    for case in ("a_lamp_created_replaces_the_resident_light_list", "an_environment_map_set_is_built_on_the_device", "a_lamp_and_an_environment_in_one_tick"):
        assert f"[       OK ] LightingUpdateFixture.{case}" in p.stdout, p.stdout[-4000:]
