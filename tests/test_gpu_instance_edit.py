"""hipr_edit_scene_instances on the GPU (csrc/instance_edit.h): models of the resident scene removed and created by kernels -- a destroyed model, a copy of a model whose
mesh the pools hold -- must leave, byte for byte, what the host path leaves: SceneBuilder::remove_model / insert_model, rebuild(), hipr_upload_scene on a fresh
context. Every equality is of bytes; every refusal leaves the resident scene as the call found it."""
import ctypes as C

import numpy as np
import pytest

import device_rebuild_bindings as rb
import instance_edit_bindings as ie
from bifrost3d_amd import capi
from bifrost3d_amd.host import Scene
from bifrost3d_amd.renderer import Context
from test_gpu_device_rebuild import H, SPP, W, buffers, not_ready, render, same_trees, unequal

pytestmark = pytest.mark.gpu


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


def edit_on_the_device(context, staged, operations):
    """The operations staged in the host scene and applied to the resident one. Returns the call's dict."""
    ie.apply(staged, operations)
    edits = staged.staged_instance_edits()
    assert edits is not None
    edited = context.edit_scene_instances(edits)
    assert edited["status"] == capi.HIPR_OK, context.lib.hipr_last_error()
    return edited


def adopt(staged, edited):
    assert staged.adopt_edited_trees(edited["nodes"], edited["order"], edited["deepest"], edited["slots"], edited["raw"].wide8) is True


@pytest.mark.parametrize("name, arguments, prepare, operations, counts, switches", ie.EDITS, ids=ie.EDIT_IDS)
def test_the_edits_leave_what_a_fresh_upload_of_the_hosts_rebuild_leaves(ctx, fresh, name, arguments, prepare, operations, counts, switches):
    scene, host = ie.prepared(arguments, prepare), ie.edited_on_the_host(arguments, prepare, operations)
    ctx.upload_scene(scene)
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    before = render(ctx, scene, spp=1)
    edited = edit_on_the_device(ctx, scene, operations)
    fresh.upload_scene(host)
    assert (edited["triangle_count"], edited["node_count"], edited["wide8"]["slot_count"]) == counts and edited["instance_count"] == host.desc.instance_count
    assert unequal(buffers(ctx), buffers(fresh)) == []
    same_trees(edited, host)
    assert edited["half_area"] == fresh.refit_scene_transforms([])["uploaded_half_area"] == ctx.refit_scene_transforms([])["uploaded_half_area"]
    # the host's description is brought along without a flatten of the whole scene
    adopt(scene, edited)
    assert rb.differences(rb.description(host), rb.description(scene)) == []
    after = render(ctx, scene, spp=1)
    print(f"{name}: {int((after != before).any(axis=-1).sum())} of {W * H} pixels differ from the image before the edit")
    assert after.tobytes() == render(fresh, host, spp=1).tobytes() and not np.array_equal(after, before)


@pytest.mark.parametrize("arithmetic", ["fast", "exact"])
@pytest.mark.parametrize("which", ["cornell_remove_last", "textured_remove_every_cutout", "atrium_first_coated"])
def test_images_equal_the_fresh_uploads(arithmetic, which):
    """Both arithmetic modes; the two edits that flip a switch pick other kernel instantiations, as a fresh upload does."""
    name, arguments, prepare, operations, counts, switches = ie.EDITS[ie.EDIT_IDS.index(which)]
    context = Context(0, arithmetic=arithmetic)
    try:
        scene, host = ie.prepared(arguments, prepare), ie.edited_on_the_host(arguments, prepare, operations)
        context.upload_scene(scene)
        still = render(context, scene)
        edited = edit_on_the_device(context, scene, operations)
        adopt(scene, edited)
        on_the_device = render(context, scene)
        context.upload_scene(host)
        on_the_host = render(context, host)
        print(f"{which}, {arithmetic}: {int((on_the_device != still).any(axis=-1).sum())} of {W * H} pixels differ from the image before the edit")
        assert not np.array_equal(on_the_device, still)
        assert np.array_equal(on_the_device.view(np.uint64), on_the_host.view(np.uint64))
    finally:
        context.close()


def test_traced_hits_and_counters_equal_the_oracles_on_the_hosts_edited_description(ctx, oracle_q):
    from test_coverage_cpu import cornell_box_rays
    name, arguments, prepare, operations, counts, switches = ie.EDITS[0]
    scene, host = ie.prepared(arguments, prepare), ie.edited_on_the_host(arguments, prepare, operations)
    ctx.upload_scene(scene)
    edit_on_the_device(ctx, scene, operations)
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


def test_life_after_an_edit(ctx, fresh):
    name, arguments, prepare, operations, counts, switches = ie.EDITS[ie.EDIT_IDS.index("atrium_remove_two_add_one")]
    scene = ie.prepared(arguments, prepare)
    ctx.upload_scene(scene)
    adopt(scene, edit_on_the_device(ctx, scene, operations))
    # the other searches' arrays are stale, as after a rebuild
    assert ctx.lib.hipr_set_trace_variant(ctx.handle, capi.TRACE_BVH2) == capi.HIPR_ERROR_UNSUPPORTED
    # a device refit of a moved model -- the new one -- against the host path on the adopted scene
    refitted = ctx.refit_scene_transforms(scene.model_pose(103, **ie.NEAR))
    assert not refitted["needs_rebuild"]
    assert scene.move_model(103, rebuild_threshold=1e30, **ie.NEAR) is True
    assert np.array_equal(ctx.read_scene_buffer(capi.SCENE_BUFFER_WIDE8_SLOTS), scene.wide8_slots()) and np.array_equal(ctx.read_scene_buffer(capi.SCENE_BUFFER_TRIANGLES), scene.triangles())
    # a material edit after it against a fresh upload of the edited scene: an instance given another material, a slot made partly covering
    materials = scene.materials()
    materials[3].coverage = 0.5
    changed, assignments = [(3, materials[3])], [(10, 4)]      # instance 10 is the new model: it becomes coated
    ctx.update_scene_materials(changed, assignments)
    assert scene.update_materials(changed, assignments) is True
    fresh.upload_scene(scene)
    mine, theirs = buffers(ctx), buffers(fresh)
    assert unequal(mine[:7], theirs[:7]) == []      # the BVH2 nodes are the ones the refit leaves stale
    assert render(ctx, scene, spp=1).tobytes() == render(fresh, scene, spp=1).tobytes()
    # a second edit after the first against the host path
    second = [("remove", 103), ("insert", 0, 5, None, ie.ASIDE, 106)]
    host = ie.prepared(arguments, prepare)      # the host path on a twin: the same history, then rebuild()
    ie.apply(host, operations)
    host.rebuild()
    assert host.move_model(103, rebuild_threshold=1e30, **ie.NEAR) is True
    assert host.update_materials(changed, assignments) is True
    ie.apply(host, second)
    host.rebuild()
    edited = edit_on_the_device(ctx, scene, second)
    fresh.upload_scene(host)
    assert unequal(buffers(ctx), buffers(fresh)) == []
    same_trees(edited, host)
    adopt(scene, edited)
    assert rb.differences(rb.description(host), rb.description(scene)) == []
    # a geometry update with the adopted description is accepted, brings the new 4-wide tree and ends the stale state
    ctx.update_scene_geometry(scene)
    assert unequal(buffers(ctx), buffers(fresh)) == []
    assert ctx.lib.hipr_set_trace_variant(ctx.handle, capi.TRACE_WIDE_PERSISTENT) == 0 and ctx.lib.hipr_set_trace_variant(ctx.handle, capi.TRACE_BVH2) == 0
    ctx.set_trace_variant(-1)
    assert render(ctx, scene, spp=1).tobytes() == render(fresh, host, spp=1).tobytes()


def test_an_edit_after_a_refit_that_awaits_a_rebuild(ctx, fresh, tmp_path):
    import device_refit_bindings as refit
    scene, host = refit.scene_with_a_parting_pair(tmp_path / "pair.obj"), refit.scene_with_a_parting_pair(tmp_path / "host.obj")
    ctx.upload_scene(scene)
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    moved = scene.model_pose(1, **refit.LARGE_POSE)
    assert ctx.refit_scene_transforms(moved)["needs_rebuild"]
    assert not_ready(ctx, scene)
    # the list as it stands plus a copy of the model at another place; the kept instance is the one the device holds, moved
    assert host.move_model(1, rebuild_threshold=1e30, **refit.LARGE_POSE) is False
    operations = [("insert", 1000, 1, None, dict(translation=(0.0, 3.0, 0.0)), 50)]
    ie.apply(host, operations)
    edits = host.staged_instance_edits()
    assert edits is not None and [e.source for e in edits][:-1] == list(range(len(edits) - 1))
    edited = ctx.edit_scene_instances(edits)
    assert edited["status"] == capi.HIPR_OK, ctx.lib.hipr_last_error()
    host.rebuild()
    fresh.upload_scene(host)
    assert unequal(buffers(ctx), buffers(fresh)) == []
    same_trees(edited, host)
    assert render(ctx, host, spp=1).tobytes() == render(fresh, host, spp=1).tobytes()      # ready again


def raw_edit(context, edits, count=None, triangles=None, **capacities):
    """The raw status of hipr_edit_scene_instances with outputs of the given capacities, and whether it left them untouched."""
    n = triangles if triangles is not None else context._resident_counts[0] + sum(int(e.primitive_count) for e in edits or [] if e.source == capi.EDIT_NEW_INSTANCE)
    nodes = np.full((capacities.get("nodes", max(n - 1, 1)), 16), 0xA5A5A5A5, np.uint32)
    order = np.full(capacities.get("order", n), 0xA5A5A5A5, np.uint32)
    slots = np.full((capacities.get("slots", min(2 * n, 0xFFFFFF)), 16), 0xA5A5A5A5, np.uint32)
    result = capi.HiprSceneEditResult()
    status = context.lib.hipr_edit_scene_instances(context.handle, edits, len(edits) if count is None else count, 62, C.c_void_p(nodes.ctypes.data), len(nodes), C.c_void_p(order.ctypes.data), len(order),
                                                   C.c_void_p(slots.ctypes.data), len(slots), C.byref(result) if capacities.get("result", True) else None)
    untouched = bool((nodes == 0xA5A5A5A5).all() and (order == 0xA5A5A5A5).all() and (slots == 0xA5A5A5A5).all() and bytes(result) == bytes(capi.HiprSceneEditResult()))
    return status, untouched


def test_refusals_leave_the_buffers_and_a_render_as_before(ctx, tmp_path):
    INVALID, UNSUPPORTED = capi.HIPR_ERROR_INVALID_ARGUMENT, capi.HIPR_ERROR_UNSUPPORTED
    scene = rb.make_scene(ie.CORNELL)
    kept_list = scene.staged_instance_edits()
    # no scene: not ready, and still not ready afterwards
    empty = Context(0)
    try:
        empty._resident_counts = (184, 7, 6)
        assert raw_edit(empty, kept_list) == (capi.HIPR_ERROR_NOT_READY, True)
        assert not_ready(empty, scene)
    finally:
        empty.close()
    # a scene another search walks
    small = Scene("cornell")
    ctx.upload_scene(small)
    assert ctx.trace_variant() != capi.TRACE_WIDE8_PERSISTENT
    before = render(ctx, small)
    assert raw_edit(ctx, small.staged_instance_edits()) == (UNSUPPORTED, True)
    assert np.array_equal(render(ctx, small), before)

    ctx.upload_scene(scene)
    kept, before = buffers(ctx), render(ctx, scene)
    d = scene.desc
    staged = rb.make_scene(ie.CORNELL)
    ie.apply(staged, [("insert", 3, 7, None, ie.NEAR, 170)])
    good = staged.staged_instance_edits()
    new = [k for k, e in enumerate(good) if e.source == capi.EDIT_NEW_INSTANCE][0]

    def changed(**fields):
        """`good` with fields of its new entry (or of the entry itself) set."""
        edits = (capi.HiprInstanceEdit * len(good)).from_buffer_copy(bytes(good))
        for field, value in fields.items():
            setattr(edits[new] if field in ("source", "primitive_count") else edits[new].instance, field, value)
        return edits

    twice = (capi.HiprInstanceEdit * len(kept_list)).from_buffer_copy(bytes(kept_list))
    twice[4].source = 2
    nan = changed()
    nan[new].instance.object_to_world[5] = float("nan")
    primitive_total = d.index_count // 3
    refused = [
        (None, dict(count=3, triangles=184), INVALID),                                    # a null list
        (good, dict(result=False), INVALID),                                              # a null result
        (changed(source=7), {}, INVALID),                                                 # a source out of range
        (twice, {}, INVALID),                                                             # a resident instance named twice
        (changed(index_offset=primitive_total - 11), {}, INVALID),                        # twelve primitives from eleven before the end of the index pool
        (changed(index_offset=primitive_total + 1, primitive_count=0), {}, INVALID),
        (changed(vertex_offset=d.vertex_count + 1), {}, INVALID),
        (changed(material_index=d.material_count), {}, INVALID),
        (changed(material_index=-1), {}, INVALID),
        (changed(mesh_flags=capi_mesh_flag_without_a_pool(d)), {}, INVALID),
        (nan, {}, INVALID),
        (good, dict(nodes=196 - 2), INVALID),                                             # outputs below the bound for the NEW count of 196
        (good, dict(order=195), INVALID),
        (good, dict(slots=2 * 196 - 1), INVALID),
        (kept_list, dict(count=0), UNSUPPORTED),                                          # an empty list
        (changed(primitive_count=0)[new:new + 1], {}, UNSUPPORTED),                       # a list that yields no triangle
    ]
    for edits, arguments, status in refused:
        if edits is not None and not isinstance(edits, C.Array):
            edits = (capi.HiprInstanceEdit * len(edits))(*edits)
        assert raw_edit(ctx, edits, **arguments) == (status, True), (arguments, ctx.lib.hipr_last_error())
    # found on the device: a BVH2 of at most 64 nodes
    small_staged = rb.make_scene(ie.CORNELL)
    ie.apply(small_staged, ie.TOO_SMALL[3])
    assert raw_edit(ctx, small_staged.staged_instance_edits()) == (UNSUPPORTED, True)
    assert b"64" in ctx.lib.hipr_last_error()
    assert unequal(kept, buffers(ctx)) == [] and np.array_equal(render(ctx, scene), before)
    # ... and the sound list is taken afterwards: nothing of the refusals stayed behind
    assert raw_edit(ctx, good)[0] == capi.HIPR_OK


def capi_mesh_flag_without_a_pool(d):
    """A mesh flag whose attribute pool the Cornell box does not upload (it has no per-vertex emission)."""
    assert not d.emissions
    return 8      # HIPR_MESH_EMISSIVE


def test_an_index_outside_the_vertex_pool_and_a_declined_build_are_found_on_the_device(ctx, tmp_path):
    from test_gpu_device_rebuild import decline_scene
    # an index triple of the uploaded pool that points past the vertex pool, in a mesh no resident instance draws: only the edit's kernel can find it
    scene = rb.make_scene(ie.CORNELL)
    d = scene.desc
    spare = d.index_count // 3
    indices = np.concatenate([np.ctypeslib.as_array(d.indices, shape=(d.index_count,)), np.array([0, 1, 2, 0, 2, d.vertex_count, 0, 1, 3], np.uint32)])
    bad = capi.HiprSceneDesc.from_buffer_copy(bytes(d))
    bad.indices, bad.index_count = indices.ctypes.data_as(C.POINTER(C.c_uint32)), len(indices)
    ctx._scene = scene
    assert ctx.lib.hipr_upload_scene(ctx.handle, C.byref(bad)) == capi.HIPR_OK, ctx.lib.hipr_last_error()
    ctx._resident_counts, ctx._rebuilt_counts = (d.triangle_count, d.instance_count, d.material_count), None
    kept, before = buffers(ctx), render(ctx, scene)
    edits = (capi.HiprInstanceEdit * 8)()
    for k in range(7):
        edits[k].source = k
    edits[7].source, edits[7].primitive_count = capi.EDIT_NEW_INSTANCE, 3
    last = np.ascontiguousarray(scene.instances_array()[6])      # the record of a resident instance, drawn from the spare triples
    C.memmove(C.byref(edits[7].instance), last.ctypes.data, C.sizeof(capi.HiprInstance))
    edits[7].instance.index_offset, edits[7].instance.vertex_offset = spare, 0
    assert raw_edit(ctx, edits) == (capi.HIPR_ERROR_UNSUPPORTED, True)
    assert b"vertex pool" in ctx.lib.hipr_last_error()
    assert unequal(kept, buffers(ctx)) == [] and np.array_equal(render(ctx, scene), before)
    # a decline of the BVH2 build: a median range longer than a lane sorts
    declined = decline_scene(tmp_path / "decline.obj")
    ctx.upload_scene(declined)
    kept, before = buffers(ctx), render(ctx, declined)
    assert raw_edit(ctx, declined.staged_instance_edits()) == (capi.HIPR_ERROR_UNSUPPORTED, True)
    assert b"median" in ctx.lib.hipr_last_error() and b"hipr_edit_scene_instances" in ctx.lib.hipr_last_error()
    assert unequal(kept, buffers(ctx)) == [] and np.array_equal(render(ctx, declined), before)


def test_a_group_of_one_member_edits_like_a_single_context(ctx):
    lib = ctx.lib
    name, arguments, prepare, operations, counts, switches = ie.EDITS[ie.EDIT_IDS.index("atrium_insert_middle")]
    scene, staged = ie.prepared(arguments, prepare), ie.prepared(arguments, prepare)
    ctx.upload_scene(scene)
    single = edit_on_the_device(ctx, staged, operations)
    adopt(staged, single)
    image = render(ctx, staged)
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
        again = ie.prepared(arguments, prepare)
        ie.apply(again, operations)
        edited = ctx.edit_scene_instances(again.staged_instance_edits(), group=group, capacities=(counts[0] - 1, counts[0], 2 * counts[0]))
        assert edited["status"] == capi.HIPR_OK, lib.hipr_last_error()
        assert all(np.array_equal(edited[k], single[k]) for k in ("nodes", "order", "slots")) and bytes(edited["raw"]) == bytes(single["raw"])
        for a in range(SPP):
            cam = staged.camera(W, H, accumulations=a, max_bounce_count=4)
            assert lib.hipr_group_trace_pass(group, C.byref(cam)) == 0
            assert lib.hipr_group_accumulate_samples(group, 0, 1, a, None, 0, 1) == 0
        accumulation = np.zeros((H, W, 4), np.float64)
        assert lib.hipr_group_read_accumulation(group, accumulation.ctypes.data_as(C.POINTER(C.c_double)), W * H) == 0
    finally:
        lib.hipr_group_destroy(group)
    assert np.array_equal(accumulation.view(np.uint64), image.view(np.uint64))


def test_a_model_destroyed_and_a_copy_created_through_the_renderer_class():
    """tests/native/InstanceEditTest.cpp: with HIPR_DEVICE_INSTANCE_EDIT=1 HIPRenderer::Renderer edits the resident scene, counts the tick, uploads nothing further and
    gives the frame of the host path bit for bit; with the variable unset the scene is retired and the camera takes the upload."""
    import subprocess
    from pathlib import Path
    binary = Path(__file__).resolve().parent / "native" / "renderer_test"
    assert binary.exists(), f"{binary} is missing: run __graft_entry__.build()"
    p = subprocess.run([str(binary), "--gpu", "InstanceEditFixture"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert "[       OK ] InstanceEditFixture.a_destroyed_model_and_a_created_copy_edit_the_resident_scene" in p.stdout, p.stdout[-4000:]
