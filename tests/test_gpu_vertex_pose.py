"""hipr_set_scene_rigs / hipr_pose_scene_rigs on the GPU: rigs bound to the resident scene and posed by k_pose_vertices (csrc/vertex_pose.h), followed by the vertex
update's continuation, must leave, byte for byte, (a) what the host path leaves -- Scene.pose_rigs on the builder (tests/test_vertex_pose_on_host_cpu.py), then
hipr_upload_scene of its description on a fresh context -- and (b) what hipr_update_scene_vertices leaves on a twin context that is given Scene.posed_geometry: the
four vertex pools, the triangles, the 8-wide tree, the trace and shading records, the class bytes, the grid and both half areas, the search the context picks and
the image in both arithmetic modes -- and refuse what it cannot do before it touches anything. Every refusal here is a check on the host that returns a status."""
import ctypes as C

import numpy as np
import pytest

import pool_growth_bindings as pg
import vertex_pose_bindings as vp
import vertex_update_bindings as vu
from bifrost3d_amd import capi
from bifrost3d_amd.renderer import Context
from test_gpu_vertex_update import BUFFERS, MODES, NEVER_REBUILD, bits, buffers, not_ready, render, same_as_a_fresh_upload, unequal
from test_vertex_pose_on_host_cpu import edit_inside_the_tube_rig, refused_poses, refused_rigs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pairs():
    """Per arithmetic mode: the context that is posed, and the second one, which takes a fresh upload of the posed scene."""
    made = {mode: (Context(0, arithmetic=mode), Context(0, arithmetic=mode)) for mode in MODES}
    yield made
    for ctx, fresh in made.values():
        ctx.close()
        fresh.close()


@pytest.fixture(scope="module")
def ctx(pairs):
    return pairs["fast"][0]


@pytest.fixture(scope="module")
def fresh(pairs):
    return pairs["fast"][1]


@pytest.fixture(scope="module")
def twin():
    """The context that receives hipr_update_scene_vertices with Scene.posed_geometry: the new entry and the existing one must meet."""
    made = Context(0, arithmetic="fast")
    yield made
    made.close()


def bound(ctx, scene, rigs):
    ctx.upload_scene(scene)
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    assert ctx.set_scene_rigs(scene.pooled_rigs(rigs)) == capi.HIPR_OK, ctx.lib.hipr_last_error()


def pose_status(ctx, poses, group=None, null_poses=False, null_out=False):
    """The raw status of hipr_pose_scene_rigs (the refusals), or of hipr_group_pose_scene_rigs on the HiprGroup handle `group`."""
    poses = list(poses)
    array, keep = capi.rig_poses(poses)
    result = capi.HiprVertexUpdateResult()
    call, handle = (ctx.lib.hipr_group_pose_scene_rigs, group) if group is not None else (ctx.lib.hipr_pose_scene_rigs, ctx.handle)
    return call(handle, None if null_poses else array, max(len(poses), int(null_poses)), None if null_out else C.byref(result))


def posed_on_both(ctx, scene, rigs, poses, kept=True):
    """The poses on the device of `ctx`, then in the builder of `scene`; the device's answer, checked against the count made from the builder's arrays."""
    moved = vp.moved_count(scene, rigs, poses)
    answer = ctx.pose_scene_rigs(poses)
    assert answer["status"] == capi.HIPR_OK, ctx.lib.hipr_last_error()
    assert scene.pose_rigs(poses, NEVER_REBUILD) is kept
    assert answer["moved_triangles"] == moved and answer["needs_rebuild"] == (not kept) and (answer["candidate_triangles"], answer["changed_triangles"]) == (0, 0), answer
    return answer


def rebuilt_equals_a_fresh_upload(ctx, fresh, scene):
    """A context that awaits its rebuild is not ready; rebuilt, it holds what a fresh upload of the builder (which rebuilt) holds."""
    assert not_ready(ctx, scene) and pose_status(ctx, []) == capi.HIPR_ERROR_NOT_READY
    assert ctx.rebuild_scene_trees()["status"] == capi.HIPR_OK
    fresh.upload_scene(scene)
    held = buffers(ctx)
    assert unequal(held, buffers(fresh)) == []
    assert np.array_equal(held[capi.SCENE_BUFFER_TRIANGLES], scene.triangles()) and np.array_equal(held[capi.SCENE_BUFFER_WIDE8_SLOTS], scene.wide8_slots())
    return held


@pytest.mark.parametrize("name", vp.CASE_IDS)
def test_buffers_grid_areas_search_and_images_equal_a_fresh_uploads_and_the_vertex_updates(pairs, twin, name):
    scene, info, rigs, steps = vp.case(name)
    other, _, _, _ = vp.case(name)      # the exact mode's builder: each context is followed by a builder of its own
    scenes = dict(fast=scene, exact=other)
    for mode in MODES:
        bound(pairs[mode][0], scenes[mode], rigs)
    twin.upload_scene(scene)
    kept = name != "zero_matrix_collapses_a_limb"      # its triangles fall onto each other: a leaf record cannot be refitted (tests/test_vertex_pose_on_host_cpu.py)
    for step, poses in enumerate(steps):
        edits = vp.as_vertex_edits(scene, rigs, poses)
        for mode in MODES:
            ctx, fresh = pairs[mode]
            answer = posed_on_both(ctx, scenes[mode], rigs, poses, kept)
            held = same_as_a_fresh_upload(ctx, fresh, scenes[mode], answer) if kept else rebuilt_equals_a_fresh_upload(ctx, fresh, scenes[mode])
        # (b) the twin, which is given finished vertices
        theirs = twin.update_scene_vertices(edits)
        assert theirs["status"] == capi.HIPR_OK and theirs["needs_rebuild"] == (not kept) and theirs["moved_triangles"] == answer["moved_triangles"]
        if not kept:
            assert twin.rebuild_scene_trees()["status"] == capi.HIPR_OK
        else:
            assert theirs["child_half_area"] == answer["child_half_area"] and theirs["uploaded_half_area"] == answer["uploaded_half_area"]
            assert np.array_equal(bits(theirs["grid_min"]), bits(answer["grid_min"])) and np.array_equal(bits(theirs["grid_cell"]), bits(answer["grid_cell"]))
        assert unequal(held, buffers(twin)) == [] and twin.trace_variant() == pairs["fast"][0].trace_variant()
        if name == "bounds_grow_and_shrink_back":      # the grid grew with the box, then shrank to the floor again
            assert float(answer["grid_min"][1]) < -1.0 if step == 0 else float(answer["grid_min"][1]) == -0.5
            assert answer["child_half_area"] != answer["uploaded_half_area"]
        if name == "zero_matrix_collapses_a_limb":      # the top row lies in the origin and wears its rest normals' codes
            top = held[capi.SCENE_BUFFER_GEOMETRY].view(vp.GEOMETRY).reshape(-1)[scene.pooled_rigs(rigs)[0]["first"] + 272:][:17]
            assert not top["position"].view(np.uint32).any() and top["oct_normal"].any()
        if name == "mesh_without_normals":
            first = scene.pooled_rigs(rigs)[0]["first"]
            assert not held[capi.SCENE_BUFFER_GEOMETRY].view(vp.GEOMETRY).reshape(-1)[first:first + 7]["oct_normal"].any()
    for mode in MODES:
        ctx, fresh = pairs[mode]
        assert np.array_equal(render(ctx, scenes[mode]).view(np.uint64), render(fresh, scenes[mode]).view(np.uint64)), mode
    assert np.array_equal(render(twin, scene).view(np.uint64), render(pairs["fast"][0], scene).view(np.uint64))
    print("times of the last pose (ms):", pairs["fast"][0].vertex_pose_times())


def test_both_matrix_paths_leave_the_same_bytes(ctx):
    scene, info, rigs, steps = vp.case("box_worn_by_two_and_a_mirrored_twin_all_four_slots")
    bound(ctx, scene, rigs)
    held = []
    try:
        for budget in (vp.lds_capacity(), vp.lds_joints(), 3, 0):
            assert ctx.lib.hipr_debug_set_pose_lds_joints(ctx.handle, budget) == capi.HIPR_OK
            assert ctx.pose_scene_rigs(steps[0])["status"] == capi.HIPR_OK
            held.append(buffers(ctx))
        assert ctx.lib.hipr_debug_set_pose_lds_joints(ctx.handle, vp.lds_capacity() + 1) == capi.HIPR_ERROR_INVALID_ARGUMENT
    finally:
        ctx.lib.hipr_debug_set_pose_lds_joints(ctx.handle, vp.lds_joints())
    assert all(unequal(held[0], other) == [] for other in held[1:])
    assert scene.pose_rigs(steps[0], NEVER_REBUILD) is True
    assert np.array_equal(held[0][capi.SCENE_BUFFER_GEOMETRY].view(np.uint8).reshape(-1), vu.pool(scene, "geometry").view(np.uint8).reshape(-1))


def test_pose_a_then_pose_b_leaves_what_b_alone_leaves(ctx, fresh):
    scene, info, rigs, _ = vp.case("tube_257")
    alone, _, _, _ = vp.case("tube_257")
    bound(ctx, scene, rigs)
    a, b = [dict(rig=0, matrices=vp.bend(2, 1.1))], [dict(rig=0, matrices=vp.bend(2, -0.4, seed=3))]
    posed_on_both(ctx, scene, rigs, a)
    posed_on_both(ctx, scene, rigs, b)
    assert alone.pose_rigs(b, NEVER_REBUILD) is True
    fresh.upload_scene(alone)
    assert unequal(buffers(ctx), buffers(fresh)) == []
    assert np.array_equal(render(ctx, scene).view(np.uint64), render(fresh, alone).view(np.uint64))


def test_a_vertex_edit_after_a_staged_pose_wins_in_the_builder_as_on_the_device(ctx, fresh):
    scene, info, rigs, _ = vp.case("tube_257")
    bound(ctx, scene, rigs)
    staged = scene.stage_rig_poses([dict(rig=0, matrices=vp.bend(2, 1.1))])
    assert staged is not None and ctx.pose_scene_rigs(staged)["status"] == capi.HIPR_OK
    pooled = scene.stage_vertex_edits([edit_inside_the_tube_rig(scene, info)])      # inside the posed range, before the builder has caught up
    answer = ctx.update_scene_vertices(pooled)
    assert answer["status"] == capi.HIPR_OK and not answer["needs_rebuild"]
    assert scene.apply_staged(NEVER_REBUILD) is True
    same_as_a_fresh_upload(ctx, fresh, scene, answer)


def seam_rig(info, apart):
    """The seam quad: vertices 0 and 3, 1 and 5 share their rest data. apart: vertex 5 follows the other joint."""
    rig = vp.of_mesh(info, "seam", 0, 6)
    rig["joints"] = np.tile(np.array([0, 1, 0, 0], np.uint16), (6, 1))
    rig["weights"] = np.tile(np.array([0.5, 0.5, 0.0, 0.0], np.float32), (6, 1))
    if apart:
        rig["weights"][5] = (1.0, 0.0, 0.0, 0.0)
    rig["joint_count"] = 2
    return rig


def test_seam_vertices_with_the_same_rest_data_stay_one_corner_and_with_other_weights_part(ctx, fresh):
    pose = [dict(rig=0, matrices=np.stack([vp.matrix(translation=(0.0, 0.0, 0.1)), vp.matrix(angle=0.3, translation=(0.05, 0.0, 0.3))]))]
    scene, info = vp.make_scene()
    rigs = [seam_rig(info, apart=False)]
    assert scene.set_rigs(rigs)
    bound(ctx, scene, rigs)
    answer = posed_on_both(ctx, scene, rigs, pose)
    assert answer["moved_triangles"] == 2
    same_as_a_fresh_upload(ctx, fresh, scene, answer)
    # the same two with different weights part: the scene awaits its rebuild
    scene, info = vp.make_scene()
    rigs = [seam_rig(info, apart=True)]
    assert scene.set_rigs(rigs)
    bound(ctx, scene, rigs)
    posed_on_both(ctx, scene, rigs, pose, kept=False)
    rebuilt_equals_a_fresh_upload(ctx, fresh, scene)
    assert np.array_equal(render(ctx, scene).view(np.uint64), render(fresh, scene).view(np.uint64))
    # the rigs outlive the rebuild: the same pose again moves every vertex to where it is
    same_as_a_fresh_upload(ctx, fresh, scene, posed_on_both(ctx, scene, rigs, pose))


def test_the_rigs_outlive_the_other_writers_and_go_with_an_upload(ctx, fresh):
    scene, info = vp.make_scene()
    rigs = [vp.flag_rig(info, 0, 289, 2, True, joints=2), vp.box_rig(info)]
    assert scene.set_rigs(rigs)
    bound(ctx, scene, rigs)
    poses = lambda k: [dict(rig=0, matrices=vp.bend(2, 0.1 * k), weights=[0.1 * k, -0.2]), dict(rig=1, matrices=vp.box_pose(k))]

    def pose_and_compare(k):
        same_as_a_fresh_upload(ctx, fresh, scene, posed_on_both(ctx, scene, rigs, poses(k)))

    pose_and_compare(1)
    # a material edit
    materials = [(info["cutout"], pg.material(tint=(0.2, 0.9, 0.3)))]
    ctx.update_scene_materials(materials)
    assert scene.update_materials(materials) is True
    pose_and_compare(2)
    # a texel edit
    texels = [(1, 24, 24, np.full((8, 8), 255, np.uint8))]
    assert ctx.update_scene_texels(texels)["status"] == capi.HIPR_OK and scene.update_texels(texels) is True
    pose_and_compare(3)
    # a vertex edit beside the rigs
    edits = [vu.geometry_edit(scene, info, "glowing", 0, 8, move=vu.wobble(23))]
    assert ctx.update_scene_vertices(vu.pooled(scene, edits))["status"] == capi.HIPR_OK and scene.update_vertices(edits, NEVER_REBUILD) is True
    pose_and_compare(4)
    # an instance edit: a model over the rigged box leaves
    assert scene.remove_model(vu.BOX_B)
    edited = ctx.edit_scene_instances(scene.staged_instance_edits())
    assert edited["status"] == capi.HIPR_OK, ctx.lib.hipr_last_error()
    assert scene.adopt_edited_trees(edited["nodes"], edited["order"], edited["deepest"], edited["slots"], edited["wide8"])
    pose_and_compare(5)
    # a pool growth: a model over a new mesh
    info["mesh"]["appended"] = scene.add_mesh(**vu.mesh_data()["box"])
    assert scene.insert_model(1000, info["mesh"]["appended"], info["plain"], model_index=301, **pg.IN_THE_BOX) == 301
    growth, edits = scene.staged_scene_growth()
    assert ctx.append_scene_pools(growth) == capi.HIPR_OK, ctx.lib.hipr_last_error()
    edited = ctx.edit_scene_instances(edits)
    assert edited["status"] == capi.HIPR_OK, ctx.lib.hipr_last_error()
    assert scene.adopt_edited_trees(edited["nodes"], edited["order"], edited["deepest"], edited["slots"], edited["wide8"])
    pose_and_compare(6)
    # set_scene_rigs replaces the set (rig 0 is now the box) and removes it
    assert ctx.set_scene_rigs(scene.pooled_rigs(rigs[1:])) == capi.HIPR_OK and scene.set_rigs(rigs[1:])
    assert pose_status(ctx, [dict(rig=1, matrices=vp.box_pose(7))]) == capi.HIPR_ERROR_INVALID_ARGUMENT      # rig 1 is not bound any more
    same_as_a_fresh_upload(ctx, fresh, scene, posed_on_both(ctx, scene, rigs[1:], [dict(rig=0, matrices=vp.box_pose(7))]))
    assert ctx.set_scene_rigs([]) == capi.HIPR_OK
    assert pose_status(ctx, [dict(rig=0, matrices=vp.box_pose(7))]) == capi.HIPR_ERROR_INVALID_ARGUMENT and pose_status(ctx, []) == capi.HIPR_OK
    # an upload drops the rigs
    assert ctx.set_scene_rigs(scene.pooled_rigs(rigs[1:])) == capi.HIPR_OK and pose_status(ctx, [dict(rig=0, matrices=vp.box_pose(8))]) == capi.HIPR_OK
    ctx.upload_scene(scene)
    held = buffers(ctx)
    assert pose_status(ctx, [dict(rig=0, matrices=vp.box_pose(8))]) == capi.HIPR_ERROR_INVALID_ARGUMENT and unequal(buffers(ctx), held) == []


def test_refusals_leave_everything_as_it_was(ctx):
    from bifrost3d_amd.host import Scene
    lib = ctx.lib
    scene, info = vp.make_scene(tube=True)
    rigs = [vp.tube_rig(info, 0, 16, 2), vp.flag_rig(info, 100, 16, 2)]
    sound = [dict(rig=0, matrices=vp.bend(2))]
    empty = Context(0)
    try:
        assert empty.set_scene_rigs(scene.pooled_rigs(rigs)) == capi.HIPR_ERROR_NOT_READY and pose_status(empty, sound) == capi.HIPR_ERROR_NOT_READY
    finally:
        empty.close()
    # a scene that is not traced through the 8-wide tree takes rigs (they are data) and refuses poses: the exhaustive search's items, and another search walked
    small = Scene("cornell", param0=1)
    ctx.upload_scene(small)
    assert ctx.trace_variant() == capi.TRACE_EXHAUSTIVE
    wall = dict(first=0, rest_positions=np.zeros((2, 3), np.float32), target_positions=np.zeros((1, 2, 3), np.float32))
    assert ctx.set_scene_rigs([wall]) == capi.HIPR_OK
    image, held = render(ctx, small), buffers(ctx)
    assert pose_status(ctx, [dict(rig=0, weights=[1.0])]) == capi.HIPR_ERROR_UNSUPPORTED and b"upload" in lib.hipr_last_error()
    assert unequal(buffers(ctx), held) == [] and np.array_equal(render(ctx, small), image)
    ctx.set_trace_variant(capi.TRACE_WIDE_PERSISTENT)
    try:
        ctx.upload_scene(scene)
        assert ctx.set_scene_rigs(scene.pooled_rigs(rigs)) == capi.HIPR_OK and pose_status(ctx, sound) == capi.HIPR_ERROR_UNSUPPORTED
    finally:
        ctx.set_trace_variant(-1)

    ctx.upload_scene(scene)
    image, held = render(ctx, scene), buffers(ctx)
    count = scene.desc.vertex_count
    # every refusal of hipr_set_scene_rigs: the lists of the CPU suite in pool coordinates (those about a mesh's end are the builder's), and the pool's end
    of_the_mesh = ("begins past the mesh", "reaches past the mesh", "first + count wraps around 32 bits")
    for what, bad in refused_rigs(info).items():
        if what not in of_the_mesh:
            assert ctx.set_scene_rigs(scene.pooled_rigs(bad)) == capi.HIPR_ERROR_INVALID_ARGUMENT, what
    pool_rig = lambda first, n: dict(first=first, rest_positions=np.zeros((n, 3), np.float32), target_positions=np.zeros((1, n, 3), np.float32))
    assert [ctx.set_scene_rigs([pool_rig(count, 1)]), ctx.set_scene_rigs([pool_rig(count - 1, 2)]), ctx.set_scene_rigs([pool_rig(0xFFFFFFFF, 2)])] == [capi.HIPR_ERROR_INVALID_ARGUMENT] * 3
    array, keep = capi.rig_descs(scene.pooled_rigs(rigs))
    assert lib.hipr_set_scene_rigs(ctx.handle, None, 2) == capi.HIPR_ERROR_INVALID_ARGUMENT
    assert pose_status(ctx, sound) == capi.HIPR_ERROR_INVALID_ARGUMENT      # none of them bound anything
    # every refusal of hipr_pose_scene_rigs
    assert ctx.set_scene_rigs(scene.pooled_rigs(rigs)) == capi.HIPR_OK
    for what, poses in refused_poses().items():
        assert pose_status(ctx, poses) == capi.HIPR_ERROR_INVALID_ARGUMENT, what
    assert pose_status(ctx, sound, null_out=True) == capi.HIPR_ERROR_INVALID_ARGUMENT and pose_status(ctx, sound, null_poses=True) == capi.HIPR_ERROR_INVALID_ARGUMENT
    assert unequal(buffers(ctx), held) == [] and np.array_equal(render(ctx, scene), image)
    # a refused rig list leaves the bound set: the sound pose is served; an empty list of poses changes nothing
    assert ctx.set_scene_rigs(scene.pooled_rigs(refused_rigs(info)["two rigs overlap"])) == capi.HIPR_ERROR_INVALID_ARGUMENT
    assert pose_status(ctx, []) == capi.HIPR_OK and unequal(buffers(ctx), held) == []
    assert lib.hipr_set_trace_variant(ctx.handle, capi.TRACE_BVH2) == 0
    ctx.set_trace_variant(-1)
    assert pose_status(ctx, sound) == capi.HIPR_OK
    assert lib.hipr_set_trace_variant(ctx.handle, capi.TRACE_BVH2) != 0      # the BVH2 and the 4-wide arrays are stale, as after a refit
    ctx.set_trace_variant(-1)


def test_a_group_of_one_device_binds_and_poses_like_a_single_context(ctx, fresh):
    lib = ctx.lib
    scene, info, rigs, steps = vp.case("box_worn_by_two_and_a_mirrored_twin_all_four_slots")
    pooled, keep = capi.rig_descs(scene.pooled_rigs(rigs))
    devices = (C.c_int * 1)(0)
    group = C.c_void_p()
    assert lib.hipr_group_create(devices, 1, C.byref(group)) == 0
    member = Context.__new__(Context)      # a handle on the group's member 0, for the read-backs; the group owns the context
    member.lib, member.handle, member._scene = lib, C.c_void_p(), scene
    try:
        tables = capi.load_tables()
        t = capi.HiprTables(*[a.ctypes.data_as(C.POINTER(C.c_float)) for a in tables])
        assert lib.hipr_group_upload_tables(group, C.byref(t)) == 0
        assert lib.hipr_group_set_scene_rigs(group, pooled, 1) == capi.HIPR_ERROR_NOT_READY and pose_status(ctx, steps[0], group=group) == capi.HIPR_ERROR_NOT_READY
        assert lib.hipr_group_upload_scene(group, C.byref(scene.desc)) == 0
        member.handle = C.c_void_p(lib.hipr_group_context(group, 0))
        uploaded = buffers(member)
        assert pose_status(ctx, steps[0], group=group) == capi.HIPR_ERROR_INVALID_ARGUMENT      # nothing bound yet
        assert ctx.set_scene_rigs(scene.pooled_rigs(refused_rigs(info)["two rigs overlap"]), group=group) == capi.HIPR_ERROR_INVALID_ARGUMENT
        assert lib.hipr_group_set_scene_rigs(group, pooled, 1) == capi.HIPR_OK
        assert pose_status(ctx, steps[0], group=group, null_out=True) == capi.HIPR_ERROR_INVALID_ARGUMENT
        assert pose_status(ctx, steps[0] + steps[0], group=group) == capi.HIPR_ERROR_INVALID_ARGUMENT
        assert unequal(buffers(member), uploaded) == []
        moved = vp.moved_count(scene, rigs, steps[0])
        answer = ctx.pose_scene_rigs(steps[0], group=group)
        assert answer["status"] == capi.HIPR_OK and answer["moved_triangles"] == moved == 36 and not answer["needs_rebuild"]
        assert scene.pose_rigs(steps[0], NEVER_REBUILD) is True
        fresh.upload_scene(scene)
        assert unequal(buffers(member), buffers(fresh)) == []
    finally:
        member.handle = C.c_void_p()      # nothing of the group's is closed through the borrowed handle
        lib.hipr_group_destroy(group)
