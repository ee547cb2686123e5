"""hipr_refit_scene_transforms on the GPU: a transform-only scene change refitted by kernels over the resident arrays (csrc/wide8_refit.h) must leave, byte for
byte, what the host path leaves there -- SceneBuilder::update_model_transforms (Scene.move_model) followed by hipr_update_scene_geometry -- and refuse what it
cannot do before it touches anything."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import device_refit_bindings as refit
from bifrost3d_amd import capi
from bifrost3d_amd.host import Scene
from bifrost3d_amd.renderer import Context

pytestmark = pytest.mark.gpu

POSE = dict(translation=(0.05, -0.30, 0.10), rotation=(0.0, float(np.sin(0.4)), 0.0, float(np.cos(0.4))), scale=0.3)      # test_refitted_scene_on_the_device_bit_exact's
OTHER_POSE = dict(translation=(0.2, -0.35, -0.2), rotation=(0.0, float(np.sin(np.pi / 12)), 0.0, float(np.cos(np.pi / 12))), scale=0.3)
# (scene, param0, param1, model): the smallest Cornell box whose upload selects the 8-wide search (88 BVH2 nodes; param0 = 3 has 53) and the 20 000-triangle atrium
SCENES = [("cornell", 4, 0, 6), ("atrium", 20000, 3, 10)]
W, H, SPP = 64, 36, 4


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle_q():
    from oracle_bindings import get_oracle
    return get_oracle(True)


def render(ctx, scene, spp=SPP):
    ctx.set_frame(W, H)
    for a in range(spp):
        ctx.render_pass(scene.camera(W, H, accumulations=a, max_bounce_count=4), synchronize=True)
    return ctx.read_accumulation()


def status_of_refit(ctx, moved=(), lights=None, group=None, result=None):
    """The raw status of hipr_refit_scene_transforms (the refusals), or of hipr_group_refit_scene_transforms on the HiprGroup handle `group`."""
    moved = list(moved)
    array = (capi.HiprInstanceTransform * max(len(moved), 1))()
    for k, (index, matrix) in enumerate(moved):
        array[k].instance_index = index
        array[k].object_to_world[:] = [float(v) for v in np.asarray(matrix, np.float32).reshape(12)]
    light_array = (capi.HiprLight * max(len(lights), 1))(*lights) if lights is not None else None
    result = result if result is not None else capi.HiprRefitResult()
    call, handle = (ctx.lib.hipr_group_refit_scene_transforms, group) if group is not None else (ctx.lib.hipr_refit_scene_transforms, ctx.handle)
    return call(handle, array, len(moved), light_array, len(lights) if lights is not None else 0, C.byref(result))


def test_the_smallest_cornell_box_of_the_8_wide_search(ctx):
    ctx.upload_scene(Scene("cornell", param0=3))
    assert ctx.trace_variant() != capi.TRACE_WIDE8_PERSISTENT
    ctx.upload_scene(Scene("cornell", param0=4))
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT


@pytest.mark.parametrize("name, param0, param1, model", SCENES)
def test_slots_triangles_and_grid_byte_equal_to_the_host_refit(ctx, name, param0, param1, model):
    scene = Scene(name, param0=param0, param1=param1)
    ctx.upload_scene(scene)
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    assert np.array_equal(ctx.read_scene_buffer(capi.SCENE_BUFFER_WIDE8_SLOTS), scene.wide8_slots())      # the upload's pass over the tree (exact boxes, area) wrote nothing
    uploaded = scene.wide8_slots()
    result = ctx.refit_scene_transforms(scene.model_pose(model, **POSE))
    assert not result["needs_rebuild"]
    assert scene.move_model(model, rebuild_threshold=1e30, **POSE) is True
    slots, triangles = ctx.read_scene_buffer(capi.SCENE_BUFFER_WIDE8_SLOTS), ctx.read_scene_buffer(capi.SCENE_BUFFER_TRIANGLES)
    assert not np.array_equal(slots, uploaded)
    different = np.nonzero((slots != scene.wide8_slots()).any(axis=1))[0]
    assert len(different) == 0, (len(different), different[:8])
    assert np.array_equal(triangles, scene.triangles())
    desc = scene.desc
    assert np.array_equal(bits(result["grid_min"]), bits(desc.wide8_grid_min[:])) and np.array_equal(bits(result["grid_cell"]), bits(desc.wide8_grid_cell[:]))


def test_traced_hits_and_counters_equal_the_oracles_on_the_host_refitted_description(ctx, oracle_q):
    from test_coverage_cpu import cornell_box_rays
    scene = Scene("cornell", param0=4)
    ctx.upload_scene(scene)
    ctx.refit_scene_transforms(scene.model_pose(6, **POSE))
    assert scene.move_model(6, **POSE) is True      # the host's refit: the description the oracle walks
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    ctx.set_instrumentation(True)
    rays = cornell_box_rays(40000, 8)
    skip = np.full(len(rays), 0xFFFFFFFF, np.uint32)
    gpu = ctx.debug_trace_closest(rays, skip)
    counters = ctx.counters()
    cpu, (nodes, tris) = oracle_q.trace_closest(scene.desc, rays, skip, use_bvh=ctx.oracle_search(), with_lights=True)
    assert np.array_equal(gpu.view(np.uint32), cpu.view(np.uint32))
    assert counters["closest_nodes"] == nodes and counters["closest_triangles"] == tris
    rays[:, 7] = np.random.default_rng(3).uniform(0.05, 2.0, len(rays))
    gpu_s = ctx.debug_trace_shadow(rays)
    counters = ctx.counters()
    ctx.set_instrumentation(False)
    cpu_s, (nodes, tris) = oracle_q.trace_shadow(scene.desc, rays, use_bvh=ctx.oracle_search())
    assert np.array_equal(gpu_s, cpu_s) and counters["shadow_nodes"] == nodes and counters["shadow_triangles"] == tris


@pytest.mark.parametrize("arithmetic", ["fast", "exact"])
def test_images_equal_between_the_device_path_and_the_host_path(arithmetic):
    context = Context(0, arithmetic=arithmetic)
    try:
        scene = Scene("cornell", param0=4)
        context.upload_scene(scene)
        uploaded = context.read_scene_buffer(capi.SCENE_BUFFER_WIDE8_SLOTS)
        still = render(context, scene)
        original = [(index, np.array(scene.desc.instances[index].object_to_world[:], np.float32)) for index, _ in scene.model_pose(6, **POSE)]
        context.refit_scene_transforms(scene.model_pose(6, **POSE))
        on_the_device = render(context, scene)
        # there and back: the original slots byte for byte
        context.refit_scene_transforms(original)
        assert np.array_equal(context.read_scene_buffer(capi.SCENE_BUFFER_WIDE8_SLOTS), uploaded)
        assert np.array_equal(render(context, scene), still)
        # the host path to the same pose
        assert scene.move_model(6, **POSE) is True
        context.update_scene_geometry(scene)
        on_the_host = render(context, scene)
        assert not np.array_equal(on_the_device, still)
        assert np.array_equal(on_the_device.view(np.uint64), on_the_host.view(np.uint64))
    finally:
        context.close()


class DescriptionWithLights:
    """A scene's description with other lights (the same count): what the host path uploads after a light moved."""

    def __init__(self, scene, lights):
        self.scene = scene
        self.lights = (capi.HiprLight * len(lights))(*lights)
        self.desc = capi.HiprSceneDesc.from_buffer_copy(scene.desc)
        self.desc.lights = C.cast(self.lights, C.POINTER(capi.HiprLight))
        self.state = scene.state


def moved_lights(scene):
    d = scene.desc
    lights = []
    for l in range(d.light_count):
        light = capi.HiprLight.from_buffer_copy(d.lights[l])
        if (light.flags & 7) in (1, 5):      # sphere and spot lights: position in data[3..5]
            light.data[3] += 0.11
            light.data[4] -= 0.07
        lights.append(light)
    return lights


def test_two_models_in_one_call_and_a_call_that_moves_only_the_light(ctx):
    scene = Scene("cornell", param0=4)
    ctx.upload_scene(scene)
    ctx.refit_scene_transforms(scene.model_pose(6, **POSE) + scene.model_pose(7, **OTHER_POSE))
    assert scene.move_model(6, **POSE) is True and scene.move_model(7, rebuild_threshold=1e30, **OTHER_POSE) is True
    slots = ctx.read_scene_buffer(capi.SCENE_BUFFER_WIDE8_SLOTS)
    assert np.array_equal(slots, scene.wide8_slots()) and np.array_equal(ctx.read_scene_buffer(capi.SCENE_BUFFER_TRIANGLES), scene.triangles())
    two_moved = render(ctx, scene)
    # zero moved instances and new lights: only the light moves
    lights = moved_lights(scene)
    assert any((light.flags & 7) in (1, 5) for light in lights)
    result = ctx.refit_scene_transforms([], lights=lights)
    assert not result["needs_rebuild"]
    assert np.array_equal(ctx.read_scene_buffer(capi.SCENE_BUFFER_WIDE8_SLOTS), slots)
    light_moved = render(ctx, scene)
    assert not np.array_equal(light_moved, two_moved)
    ctx.update_scene_geometry(DescriptionWithLights(scene, lights))      # the host path: the same scene with the same lights
    assert np.array_equal(render(ctx, scene).view(np.uint64), light_moved.view(np.uint64))


def test_refusals_leave_everything_as_it_was(ctx):
    # a scene searched exhaustively: not this call's business, and the context still renders
    small = Scene("cornell")
    ctx.upload_scene(small)
    assert ctx.trace_variant() == capi.TRACE_EXHAUSTIVE
    before = render(ctx, small)
    assert status_of_refit(ctx, small.model_pose(6, **POSE)) == capi.HIPR_ERROR_UNSUPPORTED
    assert np.array_equal(render(ctx, small), before)

    scene = Scene("cornell", param0=4)
    ctx.upload_scene(scene)
    slots, triangles = ctx.read_scene_buffer(capi.SCENE_BUFFER_WIDE8_SLOTS), ctx.read_scene_buffer(capi.SCENE_BUFFER_TRIANGLES)
    index, matrix = scene.model_pose(6, **POSE)[0]
    mirrored = matrix.copy()
    mirrored[:, 0] = -mirrored[:, 0]
    assert status_of_refit(ctx, [(index, mirrored)]) == capi.HIPR_ERROR_INVALID_ARGUMENT
    assert status_of_refit(ctx, [(scene.desc.instance_count, matrix)]) == capi.HIPR_ERROR_INVALID_ARGUMENT
    lights = moved_lights(scene)
    lights[0].flags = (lights[0].flags & ~7) | (2 if (lights[0].flags & 7) != 2 else 1)      # a light that changes its type
    assert status_of_refit(ctx, [(index, matrix)], lights) == capi.HIPR_ERROR_INVALID_ARGUMENT
    assert status_of_refit(ctx, [(index, matrix)], moved_lights(scene) * 2) == capi.HIPR_ERROR_INVALID_ARGUMENT      # another light count
    assert np.array_equal(ctx.read_scene_buffer(capi.SCENE_BUFFER_WIDE8_SLOTS), slots) and np.array_equal(ctx.read_scene_buffer(capi.SCENE_BUFFER_TRIANGLES), triangles)
    # nothing is stale yet: the other searches may be asked for
    assert ctx.lib.hipr_set_trace_variant(ctx.handle, capi.TRACE_BVH2) == 0
    ctx.set_trace_variant(-1)
    # after a device refit the BVH2 and 4-wide arrays are stale, until the host path brings them along again
    ctx.refit_scene_transforms([(index, matrix)])
    assert ctx.lib.hipr_set_trace_variant(ctx.handle, capi.TRACE_BVH2) == capi.HIPR_ERROR_UNSUPPORTED
    assert ctx.lib.hipr_set_trace_variant(ctx.handle, capi.TRACE_WIDE_PERSISTENT) == capi.HIPR_ERROR_UNSUPPORTED
    assert b"stale" in ctx.lib.hipr_last_error()
    assert scene.move_model(6, **POSE) is True
    ctx.update_scene_geometry(scene)
    assert ctx.lib.hipr_set_trace_variant(ctx.handle, capi.TRACE_BVH2) == 0
    ctx.set_trace_variant(-1)


@pytest.mark.parametrize("which", ["constructed", "atrium"])
def test_a_pair_that_parts_asks_for_a_rebuild(ctx, tmp_path, which):
    """Two object-space vertices one ulp apart that round to one world position in the built pose -- the builder paired their triangles -- and part under the move:
    a constructed OBJ scene (device_refit_bindings.write_parting_pair_obj: numpy float32 search, built at scale 0.3, moved to scale 1) and model 6 of the small
    atrium, which holds such a pair by itself. The host's move_model rebuilds (False: the reference behaviour, checked first, on a scene of its own); the device
    reports needs_rebuild, a render returns not-ready, and an upload of the rebuilt scene recovers."""
    if which == "constructed":
        scene, reference = refit.scene_with_a_parting_pair(tmp_path / "pair.obj"), refit.scene_with_a_parting_pair(tmp_path / "reference.obj")
        model, pose = 1, refit.LARGE_POSE
    else:
        scene, reference = Scene("atrium", param0=20000, param1=3), Scene("atrium", param0=20000, param1=3)
        model, pose = 6, POSE
    assert reference.move_model(model, rebuild_threshold=1e30, **pose) is False
    ctx.upload_scene(scene)
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    result = ctx.refit_scene_transforms(scene.model_pose(model, **pose))
    assert result["needs_rebuild"]
    ctx.set_frame(W, H)
    assert ctx.lib.hipr_render_pass(ctx.handle, C.byref(scene.camera(W, H, max_bounce_count=4)), None, 0, 1) == capi.HIPR_ERROR_NOT_READY
    assert scene.move_model(model, rebuild_threshold=1e30, **pose) is False      # rebuilt
    ctx.upload_scene(scene)
    assert np.array_equal(ctx.read_scene_buffer(capi.SCENE_BUFFER_WIDE8_SLOTS), scene.wide8_slots())
    image = render(ctx, scene, spp=1)
    assert np.isfinite(image).all() and image[..., :3].max() > 0.0


@pytest.mark.parametrize("name, param0, param1, model", SCENES)
def test_area_sum(ctx, name, param0, param1, model):
    """child_half_area against a numpy f64 sum over the exact boxes of the read-back tree: 1e-11 relative is the bound of a binary64 sum of at most 1e5
    positive terms in any order (n * 2^-53). Equal run to run; the upload's figure is that of a refit that moves nothing."""
    scene = Scene(name, param0=param0, param1=param1)
    ctx.upload_scene(scene)
    unchanged = [(index, np.array(scene.desc.instances[index].object_to_world[:], np.float32)) for index, _ in scene.model_pose(model, **POSE)]
    same = ctx.refit_scene_transforms(unchanged)
    assert same["uploaded_half_area"] == same["child_half_area"] > 0.0
    assert np.array_equal(ctx.read_scene_buffer(capi.SCENE_BUFFER_WIDE8_SLOTS), scene.wide8_slots())
    first = ctx.refit_scene_transforms(scene.model_pose(model, **POSE))
    slots, triangles = ctx.read_scene_buffer(capi.SCENE_BUFFER_WIDE8_SLOTS), ctx.read_scene_buffer(capi.SCENE_BUFFER_TRIANGLES)
    assert len(slots) <= 100000
    expected = refit.half_area_sum(refit.exact_boxes(slots, triangles))
    print(f"child_half_area {first['child_half_area']!r}, numpy {expected!r}, uploaded {first['uploaded_half_area']!r}")
    assert abs(first["child_half_area"] - expected) <= 1e-11 * expected
    assert first["uploaded_half_area"] == same["uploaded_half_area"] and first["child_half_area"] != first["uploaded_half_area"]
    ctx.upload_scene(scene)
    again = ctx.refit_scene_transforms(scene.model_pose(model, **POSE))
    assert again["child_half_area"] == first["child_half_area"] and again["uploaded_half_area"] == first["uploaded_half_area"]


def test_a_group_of_three_members_refits_like_a_single_context(ctx):
    lib = ctx.lib
    scene = Scene("atrium", param0=20000, param1=3)
    ctx.upload_scene(scene)
    single_result = ctx.refit_scene_transforms(scene.model_pose(10, **POSE))
    single = render(ctx, scene)
    devices = (C.c_int * 3)(0, 0, 0)
    group = C.c_void_p()
    assert lib.hipr_group_create(devices, 3, C.byref(group)) == 0
    try:
        tables = capi.load_tables()
        t = capi.HiprTables(*[a.ctypes.data_as(C.POINTER(C.c_float)) for a in tables])
        assert lib.hipr_group_upload_tables(group, C.byref(t)) == 0
        assert lib.hipr_group_upload_scene(group, C.byref(scene.desc)) == 0
        state = scene.state
        assert lib.hipr_group_set_scene_state(group, C.byref(state)) == 0
        assert lib.hipr_group_set_frame(group, W, H, 1) == 0
        result = capi.HiprRefitResult()
        assert status_of_refit(ctx, scene.model_pose(10, **POSE), group=group, result=result) == 0
        assert not result.needs_rebuild and result.child_half_area == single_result["child_half_area"]
        assert np.array_equal(bits(result.grid_min[:]), bits(single_result["grid_min"])) and np.array_equal(bits(result.grid_cell[:]), bits(single_result["grid_cell"]))
        for a in range(SPP):
            cam = scene.camera(W, H, accumulations=a, max_bounce_count=4)
            assert lib.hipr_group_trace_pass(group, C.byref(cam)) == 0
            assert lib.hipr_group_accumulate_samples(group, 0, 1, a, None, 0, 1) == 0
        accumulation = np.zeros((H, W, 4), np.float64)
        assert lib.hipr_group_read_accumulation(group, accumulation.ctypes.data_as(C.POINTER(C.c_double)), W * H) == 0
    finally:
        lib.hipr_group_destroy(group)
    assert np.array_equal(accumulation.view(np.uint64), single.view(np.uint64))


def test_a_moved_node_through_the_renderer_class():
    """tests/native/DeviceRefitTest.cpp: HIPRenderer::Renderer gives the same accumulation bit for bit with the device path and with HIPR_DEVICE_REFIT=0."""
    binary = Path(__file__).resolve().parent / "native" / "renderer_test"
    assert binary.exists(), f"{binary} is missing: run __graft_entry__.build()"
    p = subprocess.run([str(binary), "--gpu", "DeviceRefitFixture"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert "[       OK ] DeviceRefitFixture.a_moved_node_gives_the_same_accumulation_on_the_device_and_on_the_host_path" in p.stdout, p.stdout[-4000:]
