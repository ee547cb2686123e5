"""hipr_rebuild_scene_trees on the GPU (csrc/scene_rebuild.h): after a device refit that asks for a rebuild -- the tree stretched past 1.5 x its uploaded half area, or
a pair parted -- the trees of the resident scene rebuilt by kernels from the triangles the device holds must leave, byte for byte, what the host path leaves:
SceneBuilder::rebuild() (Scene.move_model past the rule) followed by hipr_upload_scene on a fresh context. Every equality is of bytes; every refusal leaves the
resident scene as the call found it."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import device_rebuild_bindings as rb
import device_refit_bindings as refit
import material_update_bindings as mu
from bifrost3d_amd import capi
from bifrost3d_amd.host import Scene
from bifrost3d_amd.renderer import Context

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 36, 4
BUFFERS = capi.SCENE_BUFFERS + (capi.SCENE_BUFFER_NODES,)      # the eight readable buffers
NAMES = ("triangles", "slots", "trace triangles", "shade triangles", "classes", "materials", "instances", "nodes")


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fresh():
    """The context of the host path: it only ever takes uploads, each of which replaces everything an earlier one left."""
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle_q():
    from oracle_bindings import get_oracle
    return get_oracle(True)


def buffers(context):
    return [context.read_scene_buffer(which) for which in BUFFERS]


def unequal(a, b):
    return [name for name, x, y in zip(NAMES, a, b) if x.shape != y.shape or not np.array_equal(x, y)]


def render(context, scene, spp=SPP):
    context.set_frame(W, H)
    for a in range(spp):
        context.render_pass(scene.camera(W, H, accumulations=a, max_bounce_count=4), synchronize=True)
    return context.read_accumulation()


def not_ready(context, scene):
    context.set_frame(W, H)
    return context.lib.hipr_render_pass(context.handle, C.byref(scene.camera(W, H, max_bounce_count=4)), None, 0, 1) == capi.HIPR_ERROR_NOT_READY


def refit_then_rebuild(context, scene, model, pose):
    """The device's path for a model dragged far: the refit, which must ask for a rebuild, then the rebuild. Returns the rebuild's dict."""
    refitted = context.refit_scene_transforms(scene.model_pose(model, **pose))
    print(f"refit: needs_rebuild {refitted['needs_rebuild']}, half area {refitted['child_half_area']!r} / uploaded {refitted['uploaded_half_area']!r}")
    if refitted["needs_rebuild"]:
        assert not_ready(context, scene)
    else:
        assert refitted["child_half_area"] > 1.5 * refitted["uploaded_half_area"]
    rebuilt = context.rebuild_scene_trees()
    assert rebuilt["status"] == capi.HIPR_OK, context.lib.hipr_last_error()
    return rebuilt


def same_trees(rebuilt, host):
    """The rebuild's outputs against a host scene that moved and rebuilt."""
    d = host.desc
    assert np.array_equal(rebuilt["nodes"], host.nodes()) and np.array_equal(rebuilt["order"], host.order()) and np.array_equal(rebuilt["slots"], host.wide8_slots())
    assert (rebuilt["node_count"], rebuilt["deepest"] + 1) == (d.node_count, d.bvh_max_depth)
    w = rebuilt["wide8"]
    assert (w["slot_count"], w["height"]) == (d.wide8_slot_count, d.wide8_height)
    grid = np.concatenate([w["grid_min"], w["grid_cell"]]).view(np.uint32)
    assert np.array_equal(grid, np.array(list(d.wide8_grid_min[:]) + list(d.wide8_grid_cell[:]), np.float32).view(np.uint32))
    is_node, _ = refit.decode_tree(rebuilt["slots"])
    leaves = rebuilt["slots"][~is_node]
    assert (w["node_count"], w["leaf_count"], w["paired_leaves"]) == (int(is_node.sum()), len(leaves), int((leaves[:, 13] != 0xFFFFFFFF).sum()))


def adopt(scene, model, pose, rebuilt):
    assert scene.stage_model(model, **pose) is True
    assert scene.adopt_trees(rebuilt["nodes"], rebuilt["order"], rebuilt["deepest"], rebuilt["slots"], rebuilt["raw"].wide8) is True


@pytest.mark.parametrize("name, arguments, model, pose, uploaded, rebuilt_counts, kept_at_the_rule", rb.MOVES, ids=rb.MOVE_IDS)
def test_the_three_moves_leave_what_a_fresh_upload_of_the_hosts_rebuild_leaves(ctx, fresh, name, arguments, model, pose, uploaded, rebuilt_counts, kept_at_the_rule):
    scene, host = rb.make_scene(arguments), rb.make_scene(arguments)
    ctx.upload_scene(scene)
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    uploaded_slots = ctx.read_scene_buffer(capi.SCENE_BUFFER_WIDE8_SLOTS)
    rebuilt = refit_then_rebuild(ctx, scene, model, pose)
    assert host.move_model(model, **pose) is False      # the host's path: moved and rebuilt
    fresh.upload_scene(host)
    assert (rebuilt["node_count"], rebuilt["wide8"]["slot_count"]) == rebuilt_counts
    assert unequal(buffers(ctx), buffers(fresh)) == []
    same_trees(rebuilt, host)
    slots = ctx.read_scene_buffer(capi.SCENE_BUFFER_WIDE8_SLOTS)
    assert slots.shape != uploaded_slots.shape or not np.array_equal(slots, uploaded_slots)
    # the figure the next refit's ratio rule starts from is the one an upload takes
    unmoved = fresh.refit_scene_transforms([])
    assert rebuilt["half_area"] == unmoved["uploaded_half_area"] == ctx.refit_scene_transforms([])["uploaded_half_area"]
    # and the host's description is brought along without a flatten
    adopt(scene, model, pose, rebuilt)
    assert rb.differences(rb.description(host), rb.description(scene)) == []
    assert render(ctx, scene, spp=1).tobytes() == render(fresh, host, spp=1).tobytes()


@pytest.mark.parametrize("arithmetic", ["fast", "exact"])
def test_images_equal_the_fresh_uploads(arithmetic):
    name, arguments, model, pose = rb.MOVES[0][:4]
    context = Context(0, arithmetic=arithmetic)
    try:
        scene, host = rb.make_scene(arguments), rb.make_scene(arguments)
        context.upload_scene(scene)
        still = render(context, scene)
        refit_then_rebuild(context, scene, model, pose)
        on_the_device = render(context, scene)
        assert host.move_model(model, **pose) is False
        context.upload_scene(host)
        on_the_host = render(context, host)
        assert not np.array_equal(on_the_device, still)
        assert np.array_equal(on_the_device.view(np.uint64), on_the_host.view(np.uint64))
    finally:
        context.close()


def test_traced_hits_and_counters_equal_the_oracles_on_the_hosts_rebuilt_description(ctx, oracle_q):
    from test_coverage_cpu import cornell_box_rays
    name, arguments, model, pose = rb.MOVES[0][:4]
    scene, host = rb.make_scene(arguments), rb.make_scene(arguments)
    ctx.upload_scene(scene)
    refit_then_rebuild(ctx, scene, model, pose)
    assert host.move_model(model, **pose) is False      # the description the oracle walks
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    ctx.set_instrumentation(True)
    rays = cornell_box_rays(40000, 8)
    skip = np.full(len(rays), 0xFFFFFFFF, np.uint32)
    gpu = ctx.debug_trace_closest(rays, skip)
    counters = ctx.counters()
    cpu, (nodes, tris) = oracle_q.trace_closest(host.desc, rays, skip, use_bvh=ctx.oracle_search(), with_lights=True)
    assert np.array_equal(gpu.view(np.uint32), cpu.view(np.uint32))
    assert counters["closest_nodes"] == nodes and counters["closest_triangles"] == tris
    rays[:, 7] = np.random.default_rng(3).uniform(0.05, 2.0, len(rays))
    gpu_s = ctx.debug_trace_shadow(rays)
    counters = ctx.counters()
    ctx.set_instrumentation(False)
    cpu_s, (nodes, tris) = oracle_q.trace_shadow(host.desc, rays, use_bvh=ctx.oracle_search())
    assert np.array_equal(gpu_s, cpu_s) and counters["shadow_nodes"] == nodes and counters["shadow_triangles"] == tris


def test_a_constructed_parting_pair_recovers_to_ready(ctx, fresh, tmp_path):
    scene, host = refit.scene_with_a_parting_pair(tmp_path / "pair.obj"), refit.scene_with_a_parting_pair(tmp_path / "host.obj")
    ctx.upload_scene(scene)
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    assert ctx.refit_scene_transforms(scene.model_pose(1, **refit.LARGE_POSE))["needs_rebuild"]
    assert not_ready(ctx, scene)
    rebuilt = ctx.rebuild_scene_trees()
    assert rebuilt["status"] == capi.HIPR_OK, ctx.lib.hipr_last_error()
    assert host.move_model(1, rebuild_threshold=1e30, **refit.LARGE_POSE) is False
    fresh.upload_scene(host)
    assert unequal(buffers(ctx), buffers(fresh)) == []
    same_trees(rebuilt, host)
    assert render(ctx, scene, spp=1).tobytes() == render(fresh, host, spp=1).tobytes()      # ready again


def test_life_after_a_rebuild(ctx, fresh):
    name, arguments, model, pose = rb.MOVES[0][:4]
    scene = rb.make_scene(arguments)
    ctx.upload_scene(scene)
    first = refit_then_rebuild(ctx, scene, model, pose)
    after_first = buffers(ctx)
    # a rebuild with nothing moved since, and so two rebuilds of one scene: the same bytes
    second = ctx.rebuild_scene_trees()
    assert second["status"] == capi.HIPR_OK, ctx.lib.hipr_last_error()
    assert unequal(after_first, buffers(ctx)) == []
    assert all(np.array_equal(first[k], second[k]) for k in ("nodes", "order", "slots")) and bytes(first["raw"]) == bytes(second["raw"])
    adopt(scene, model, pose, first)
    # the other searches' arrays are stale, as after the refit
    assert ctx.lib.hipr_set_trace_variant(ctx.handle, capi.TRACE_BVH2) == capi.HIPR_ERROR_UNSUPPORTED
    # a device refit after the rebuild against the host path on the adopted scene
    ctx.refit_scene_transforms(scene.model_pose(model, **rb.POSE))
    assert scene.move_model(model, rebuild_threshold=1e30, **rb.POSE) is True
    assert np.array_equal(ctx.read_scene_buffer(capi.SCENE_BUFFER_WIDE8_SLOTS), scene.wide8_slots()) and np.array_equal(ctx.read_scene_buffer(capi.SCENE_BUFFER_TRIANGLES), scene.triangles())
    # a material edit after it against a fresh upload of the edited scene
    materials, assignments = mu.edit_of(scene, "cornell", "together")
    ctx.update_scene_materials(materials, assignments)
    assert scene.update_materials(materials, assignments) is True
    fresh.upload_scene(scene)
    mine, theirs = buffers(ctx), buffers(fresh)
    assert unequal(mine[:7], theirs[:7]) == []      # the BVH2 nodes are the ones the refit leaves stale
    # a geometry update with the adopted description is accepted, brings the new 4-wide tree and ends the stale state
    ctx.update_scene_geometry(scene)
    assert unequal(buffers(ctx), theirs) == []
    assert ctx.lib.hipr_set_trace_variant(ctx.handle, capi.TRACE_WIDE_PERSISTENT) == 0 and ctx.lib.hipr_set_trace_variant(ctx.handle, capi.TRACE_BVH2) == 0
    ctx.set_trace_variant(-1)
    assert render(ctx, scene, spp=1).tobytes() == render(fresh, scene, spp=1).tobytes()


def test_a_rebuild_with_nothing_moved_reproduces_the_upload(ctx):
    scene = rb.make_scene(rb.MOVES[1][1])
    ctx.upload_scene(scene)
    uploaded = buffers(ctx)
    rebuilt = ctx.rebuild_scene_trees(read_back=False)
    assert rebuilt["status"] == capi.HIPR_OK, ctx.lib.hipr_last_error()
    assert "nodes" not in rebuilt and (rebuilt["node_count"], rebuilt["wide8"]["slot_count"]) == (scene.desc.node_count, scene.desc.wide8_slot_count)
    assert unequal(uploaded, buffers(ctx)) == []


def rebuild_status(context, **capacities):
    """The raw status of hipr_rebuild_scene_trees with outputs of the given capacities (None: a null output)."""
    n = context._scene.desc.triangle_count
    nodes = np.full((capacities.get("nodes", max(n - 1, 1)), 16), 0xA5A5A5A5, np.uint32)
    order = np.full(n, 0xA5A5A5A5, np.uint32)
    slots = np.full((capacities.get("slots", min(2 * n, 0xFFFFFF)), 16), 0xA5A5A5A5, np.uint32)
    result = capi.HiprSceneRebuildResult()
    status = context.lib.hipr_rebuild_scene_trees(context.handle, 62, C.c_void_p(nodes.ctypes.data), len(nodes), C.c_void_p(order.ctypes.data), C.c_void_p(slots.ctypes.data), len(slots),
                                                  C.byref(result) if capacities.get("result", True) else None)
    untouched = bool((nodes == 0xA5A5A5A5).all() and (order == 0xA5A5A5A5).all() and (slots == 0xA5A5A5A5).all() and bytes(result) == bytes(capi.HiprSceneRebuildResult()))
    return status, untouched


def decline_scene(path, with_a_parting_pair=False):
    """300 coincident triangles among a few hundred others (device_rebuild_bindings.write_decline_obj); `with_a_parting_pair`: appended to the OBJ of
    device_refit_bindings.write_parting_pair_obj, and built in its small pose, so that a move to the large pose parts the pair."""
    if not with_a_parting_pair:
        return Scene("file:" + rb.write_decline_obj(path))
    text = Path(refit.write_parting_pair_obj(path)).read_text()
    v = sum(1 for line in text.splitlines() if line.startswith("v "))
    text += "\n".join(["v 40 0 0", "v 40.5 0 0", "v 40 0.5 0"] + ["f %d %d %d" % (v + 1, v + 2, v + 3)] * 300) + "\n"
    Path(path).write_text(text)
    scene = Scene("file:" + str(path))
    assert scene.move_model(1, rebuild_threshold=1e-9, **refit.SMALL_POSE) is False      # rebuilt in the small pose
    return scene


def test_refusals_leave_the_buffers_and_a_render_as_before(ctx, tmp_path):
    # no scene
    empty = Context(0)
    try:
        result = capi.HiprSceneRebuildResult()
        assert empty.lib.hipr_rebuild_scene_trees(empty.handle, 62, None, 0, None, None, 0, C.byref(result)) == capi.HIPR_ERROR_NOT_READY
    finally:
        empty.close()
    # scenes another search walks
    for small in (Scene("cornell"), Scene("cornell", param0=3)):
        ctx.upload_scene(small)
        assert ctx.trace_variant() != capi.TRACE_WIDE8_PERSISTENT
        before = render(ctx, small)
        assert rebuild_status(ctx) == (capi.HIPR_ERROR_UNSUPPORTED, True)
        assert np.array_equal(render(ctx, small), before)
    # too little room, a null result
    scene = rb.make_scene(rb.MOVES[0][1])
    ctx.upload_scene(scene)
    kept, before = buffers(ctx), render(ctx, scene)
    n = scene.desc.triangle_count
    assert rebuild_status(ctx, nodes=n - 2) == (capi.HIPR_ERROR_INVALID_ARGUMENT, True)
    assert rebuild_status(ctx, slots=2 * n - 1) == (capi.HIPR_ERROR_INVALID_ARGUMENT, True)
    assert rebuild_status(ctx, result=False) == (capi.HIPR_ERROR_INVALID_ARGUMENT, True)
    assert unequal(kept, buffers(ctx)) == [] and np.array_equal(render(ctx, scene), before)
    # a decline of the BVH2 build: a median range longer than a lane sorts
    declined = decline_scene(tmp_path / "decline.obj")
    assert declined.build_counts()["longest_median_range"] == 300
    ctx.upload_scene(declined)
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    kept, before = buffers(ctx), render(ctx, declined)
    assert rebuild_status(ctx) == (capi.HIPR_ERROR_UNSUPPORTED, True)
    assert b"median" in ctx.lib.hipr_last_error() and b"hipr_rebuild_scene_trees" in ctx.lib.hipr_last_error()
    assert unequal(kept, buffers(ctx)) == [] and np.array_equal(render(ctx, declined), before)


def test_a_decline_after_needs_rebuild_leaves_the_scene_not_ready_and_an_upload_recovers(ctx, tmp_path):
    scene = decline_scene(tmp_path / "pair_and_decline.obj", with_a_parting_pair=True)
    assert scene.build_counts()["longest_median_range"] == 300
    ctx.upload_scene(scene)
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    assert ctx.refit_scene_transforms(scene.model_pose(1, **refit.LARGE_POSE))["needs_rebuild"]
    kept = buffers(ctx)
    assert rebuild_status(ctx) == (capi.HIPR_ERROR_UNSUPPORTED, True)
    assert not_ready(ctx, scene) and unequal(kept, buffers(ctx)) == []
    assert rebuild_status(ctx) == (capi.HIPR_ERROR_UNSUPPORTED, True)      # still the state the call exists for, not one a failed writer left
    assert scene.move_model(1, rebuild_threshold=1e30, **refit.LARGE_POSE) is False
    ctx.upload_scene(scene)
    image = render(ctx, scene, spp=1)
    assert np.isfinite(image).all()


def test_a_group_of_two_members_rebuilds_like_a_single_context(ctx):
    lib = ctx.lib
    name, arguments, model, pose = rb.MOVES[1][:4]
    scene = rb.make_scene(arguments)
    ctx.upload_scene(scene)
    single = refit_then_rebuild(ctx, scene, model, pose)
    image = render(ctx, scene)
    devices = (C.c_int * 2)(0, 0)
    group = C.c_void_p()
    assert lib.hipr_group_create(devices, 2, C.byref(group)) == 0
    try:
        tables = capi.load_tables()
        t = capi.HiprTables(*[a.ctypes.data_as(C.POINTER(C.c_float)) for a in tables])
        assert lib.hipr_group_upload_tables(group, C.byref(t)) == 0
        assert lib.hipr_group_upload_scene(group, C.byref(scene.desc)) == 0
        state = scene.state
        assert lib.hipr_group_set_scene_state(group, C.byref(state)) == 0
        assert lib.hipr_group_set_frame(group, W, H, 1) == 0
        moved = scene.model_pose(model, **pose)
        array = (capi.HiprInstanceTransform * len(moved))()
        for k, (index, matrix) in enumerate(moved):
            array[k].instance_index = index
            array[k].object_to_world[:] = [float(v) for v in np.asarray(matrix, np.float32).reshape(12)]
        refitted = capi.HiprRefitResult()
        assert lib.hipr_group_refit_scene_transforms(group, array, len(moved), None, 0, C.byref(refitted)) == 0
        rebuilt = ctx.rebuild_scene_trees(group=group)
        assert rebuilt["status"] == capi.HIPR_OK, lib.hipr_last_error()
        assert all(np.array_equal(rebuilt[k], single[k]) for k in ("nodes", "order", "slots")) and bytes(rebuilt["raw"]) == bytes(single["raw"])
        for a in range(SPP):
            cam = scene.camera(W, H, accumulations=a, max_bounce_count=4)
            assert lib.hipr_group_trace_pass(group, C.byref(cam)) == 0
            assert lib.hipr_group_accumulate_samples(group, 0, 1, a, None, 0, 1) == 0
        accumulation = np.zeros((H, W, 4), np.float64)
        assert lib.hipr_group_read_accumulation(group, accumulation.ctypes.data_as(C.POINTER(C.c_double)), W * H) == 0
    finally:
        lib.hipr_group_destroy(group)
    assert np.array_equal(accumulation.view(np.uint64), image.view(np.uint64))


def test_the_two_builds_on_the_same_context_before_and_after_still_give_the_hosts_trees(ctx):
    """The split into shared device cores left hipr_build_bvh2 and hipr_build_wide8 alone."""
    name, arguments, model, pose = rb.MOVES[0][:4]
    host = rb.make_scene(arguments)
    flat = np.zeros_like(host.triangles())
    flat[host.order()] = host.triangles()      # the triangles in flatten order

    def the_two_builds():
        status, nodes, order, deepest = ctx.build_bvh2(flat)
        assert status == capi.HIPR_OK, ctx.lib.hipr_last_error()
        assert np.array_equal(nodes, host.nodes()) and np.array_equal(order, host.order()) and deepest + 1 == host.desc.bvh_max_depth
        status, slots, result = ctx.build_wide8(nodes, flat, order)
        assert status == capi.HIPR_OK, ctx.lib.hipr_last_error()
        assert np.array_equal(slots, host.wide8_slots()) and result["height"] == host.desc.wide8_height

    the_two_builds()
    scene = rb.make_scene(arguments)
    ctx.upload_scene(scene)
    refit_then_rebuild(ctx, scene, model, pose)
    kept = buffers(ctx)
    the_two_builds()
    assert unequal(kept, buffers(ctx)) == []


def test_a_node_dragged_far_through_the_renderer_class():
    """tests/native/DeviceRebuildTest.cpp: with HIPR_DEVICE_REBUILD=1 HIPRenderer::Renderer rebuilds on the device, uploads nothing further and gives the frame of a
    renderer that was given the pose from the start, bit for bit; with the variable unset the counts are the host path's."""
    import subprocess
    binary = Path(__file__).resolve().parent / "native" / "renderer_test"
    assert binary.exists(), f"{binary} is missing: run __graft_entry__.build()"
    p = subprocess.run([str(binary), "--gpu", "DeviceRebuildFixture"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert "[       OK ] DeviceRebuildFixture.a_node_dragged_far_is_rebuilt_on_the_device_without_an_upload" in p.stdout, p.stdout[-4000:]
