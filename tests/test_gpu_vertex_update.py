"""hipr_update_scene_vertices on the GPU: a vertex edit of a resident mesh applied to the resident scene by kernels (csrc/vertex_update.h over the refit's routines and
the flag rules of csrc/material_rules.h) must leave, byte for byte, what the host path leaves -- Scene.update_vertices on the builder
(tests/test_vertex_update_on_host_cpu.py), then hipr_upload_scene of its description on a fresh context: the four vertex pools, the triangles, the 8-wide tree, the
trace and shading records, the class bytes, the grid and both half areas, the search the context picks and the image in both arithmetic modes -- and refuse what it
cannot do before it touches anything. Every refusal here is a check on the host that returns a status."""
import ctypes as C

import numpy as np
import pytest

import pool_growth_bindings as pg
import vertex_update_bindings as vu
from bifrost3d_amd import capi
from bifrost3d_amd.renderer import Context

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 36, 4
POOLS = (capi.SCENE_BUFFER_GEOMETRY, capi.SCENE_BUFFER_TEXCOORDS, capi.SCENE_BUFFER_TINTS, capi.SCENE_BUFFER_EMISSIONS)
BUFFERS = capi.SCENE_BUFFERS + POOLS
NEVER_REBUILD = 1e30      # the ratio rule is the caller's policy: the device refits whatever the area
MODES = ("fast", "exact")


@pytest.fixture(scope="module")
def pairs():
    """Per arithmetic mode: the context that is edited, and the second one, which takes a fresh upload of the edited scene."""
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


def render(ctx, scene, spp=SPP):
    ctx.set_frame(W, H)
    for a in range(spp):
        ctx.render_pass(scene.camera(W, H, accumulations=a, max_bounce_count=4), synchronize=True)
    return ctx.read_accumulation()


def buffers(ctx, which=BUFFERS):
    return {b: ctx.read_scene_buffer(b) for b in which}


def unequal(a, b):
    return [which for which in a if a[which].shape != b[which].shape or not np.array_equal(a[which], b[which])]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def not_ready(ctx, scene):
    ctx.set_frame(W, H)
    return ctx.lib.hipr_render_pass(ctx.handle, C.byref(scene.camera(W, H, max_bounce_count=4)), None, 0, 1) == capi.HIPR_ERROR_NOT_READY


def status_of(ctx, edits, group=None, null_edits=False, null_out=False):
    """The raw status of hipr_update_scene_vertices (the refusals), or of hipr_group_update_scene_vertices on the HiprGroup handle `group`."""
    edits = list(edits)
    array, keep = capi.vertex_edits(edits)
    result = capi.HiprVertexUpdateResult()
    call, handle = (ctx.lib.hipr_group_update_scene_vertices, group) if group is not None else (ctx.lib.hipr_update_scene_vertices, ctx.handle)
    return call(handle, None if null_edits else array, max(len(edits), int(null_edits)), None if null_out else C.byref(result))


def same_as_a_fresh_upload(ctx, fresh, scene, answer=None):
    """The buffers, the builder's own arrays, the search, the grid and the areas of `ctx` against a fresh upload of `scene` to `fresh`."""
    fresh.upload_scene(scene)
    held = buffers(ctx)
    assert unequal(held, buffers(fresh)) == []
    assert np.array_equal(held[capi.SCENE_BUFFER_TRIANGLES], scene.triangles()) and np.array_equal(held[capi.SCENE_BUFFER_WIDE8_SLOTS], scene.wide8_slots())
    assert ctx.trace_variant() == fresh.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    mine, theirs = ctx.update_scene_vertices([]), fresh.update_scene_vertices([])      # an empty list reports what is resident
    assert mine["status"] == theirs["status"] == capi.HIPR_OK
    assert np.array_equal(bits(mine["grid_min"]), bits(theirs["grid_min"])) and np.array_equal(bits(mine["grid_cell"]), bits(theirs["grid_cell"]))
    assert np.array_equal(bits(mine["grid_min"]), bits(scene.desc.wide8_grid_min[:])) and np.array_equal(bits(mine["grid_cell"]), bits(scene.desc.wide8_grid_cell[:]))
    assert mine["child_half_area"] == theirs["child_half_area"] == theirs["uploaded_half_area"] and mine["all_triangles_opaque"] == theirs["all_triangles_opaque"]
    if answer is not None:
        assert answer["child_half_area"] == mine["child_half_area"] and answer["uploaded_half_area"] == mine["uploaded_half_area"]
        assert np.array_equal(bits(answer["grid_min"]), bits(mine["grid_min"])) and np.array_equal(bits(answer["grid_cell"]), bits(mine["grid_cell"]))
    return held


def applied_on_both(ctx, scene, info, host_edits, device_edits=None):
    """The edits on the device of `ctx`, then in the builder of `scene`; the device's answer, checked against counts made from the builder's arrays."""
    moved, candidates = vu.expected_counts(scene, info, host_edits)
    flags_before = scene.triangles()[:, 11]
    answer = ctx.update_scene_vertices(device_edits if device_edits is not None else vu.pooled(scene, host_edits))
    assert answer["status"] == capi.HIPR_OK, ctx.lib.hipr_last_error()
    assert scene.update_vertices(host_edits, NEVER_REBUILD) is True
    flags = scene.triangles()[:, 11]
    assert (answer["moved_triangles"], answer["candidate_triangles"], answer["changed_triangles"]) == (moved, candidates, int((flags != flags_before).sum())), answer
    assert answer["all_triangles_opaque"] == bool((flags & capi.TRIANGLE_OPAQUE != 0).all()) and not answer["needs_rebuild"]
    return answer


@pytest.mark.parametrize("name", vu.CASE_IDS)
def test_buffers_grid_areas_search_and_images_equal_a_fresh_uploads(pairs, name):
    scene, info = vu.make_scene()
    twin, _ = vu.make_scene()      # the exact mode's builder: each context is followed by a builder of its own
    scenes = dict(fast=scene, exact=twin)
    for mode in MODES:
        pairs[mode][0].upload_scene(scenes[mode])
        assert pairs[mode][0].trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    uploaded, image = buffers(pairs["fast"][0]), None
    for step, (host_edits, device_edits) in enumerate(vu.CASES[name](scene, info)):
        before = buffers(pairs["fast"][0])
        if name == "tints_and_emissions" and step == 1:
            image = render(pairs["fast"][0], scene)
        for mode in MODES:
            ctx, fresh = pairs[mode]
            answer = applied_on_both(ctx, scenes[mode], info, host_edits, device_edits)
            held = same_as_a_fresh_upload(ctx, fresh, scenes[mode], answer)
        # what each case is about, on the fast pair
        if name == "vertices_no_triangle_reads":
            assert answer["moved_triangles"] == 0 and unequal(held, before) == [capi.SCENE_BUFFER_GEOMETRY]
        if name == "identical_values":
            assert answer["moved_triangles"] == 512 and unequal(held, before) == []
        if name == "mesh_worn_by_two_and_a_mirrored_twin":
            assert answer["moved_triangles"] == 36
        if name == "normals_only":
            assert unequal(held, before) == [capi.SCENE_BUFFER_SHADE_TRIANGLES, capi.SCENE_BUFFER_GEOMETRY]
        if name == "beyond_the_bounds_and_inward_again":
            assert float(answer["grid_min"][1]) < -1.0 if step == 0 else float(answer["grid_min"][1]) == -0.5      # the grid grew with the vertex, then shrank to the floor again
            assert answer["child_half_area"] != answer["uploaded_half_area"]
        if name == "onto_the_hole_and_back":
            assert answer["all_triangles_opaque"] == (step == 1) and answer["changed_triangles"] > 0
            if step == 1:
                assert unequal(held, uploaded) == []
        if name == "tints_and_emissions" and step == 1:      # a mesh whose flags lack them: the pools are written, the image stays
            assert unequal(held, before) == [capi.SCENE_BUFFER_TINTS, capi.SCENE_BUFFER_EMISSIONS]
            assert np.array_equal(render(pairs["fast"][0], scene), image)
    for mode in MODES:
        ctx, fresh = pairs[mode]
        assert np.array_equal(render(ctx, scenes[mode]).view(np.uint64), render(fresh, scenes[mode]).view(np.uint64)), mode
    print("times of the last update (ms):", pairs["fast"][0].vertex_update_times())


def test_normals_tints_and_emissions_show_in_the_image(ctx):
    scene, info = vu.make_scene()
    ctx.upload_scene(scene)
    image = render(ctx, scene)
    for edits in (vu.CASES["normals_only"](scene, info)[0][0], vu.CASES["tints_and_emissions"](scene, info)[0][0]):
        applied_on_both(ctx, scene, info, edits)
        updated = render(ctx, scene)
        assert not np.array_equal(updated, image)
        image = updated


def test_a_mesh_without_a_coverage_material_has_no_candidates(ctx, fresh):
    scene, info = vu.make_scene(lace_material="plain")
    ctx.upload_scene(scene)
    answer = applied_on_both(ctx, scene, info, [vu.onto_the_hole(scene, info, 0, 40)])
    assert (answer["candidate_triangles"], answer["changed_triangles"], answer["all_triangles_opaque"]) == (0, 0, True)
    same_as_a_fresh_upload(ctx, fresh, scene, answer)


def test_parted_seam_vertices_await_the_rebuild_which_leaves_a_fresh_builds_scene(ctx, fresh):
    scene, info = vu.make_scene()
    ctx.upload_scene(scene)
    edits = [vu.geometry_edit(scene, info, "seam", 1, 1, move=(0.0, 0.0, 0.3))]
    answer = ctx.update_scene_vertices(vu.pooled(scene, edits))
    assert answer["status"] == capi.HIPR_OK and answer["needs_rebuild"] and answer["moved_triangles"] == 1
    assert not_ready(ctx, scene)
    assert status_of(ctx, vu.pooled(scene, edits)) == capi.HIPR_ERROR_NOT_READY      # a scene awaiting a rebuild takes no vertex edit
    assert scene.update_vertices(edits, NEVER_REBUILD) is False      # the builder rebuilt
    assert ctx.rebuild_scene_trees()["status"] == capi.HIPR_OK
    fresh.upload_scene(scene)
    held = buffers(ctx)
    assert unequal(held, buffers(fresh)) == []
    assert np.array_equal(held[capi.SCENE_BUFFER_TRIANGLES], scene.triangles()) and np.array_equal(held[capi.SCENE_BUFFER_WIDE8_SLOTS], scene.wide8_slots())
    assert np.array_equal(render(ctx, scene).view(np.uint64), render(fresh, scene).view(np.uint64))


def test_refusals_leave_everything_as_it_was(ctx):
    from bifrost3d_amd.host import Scene
    lib = ctx.lib
    one = np.zeros(1, np.uint32)
    empty = Context(0)
    try:
        assert status_of(empty, [dict(first=0, tints=one)]) == capi.HIPR_ERROR_NOT_READY
    finally:
        empty.close()
    # a scene that is not traced through the 8-wide tree: the exhaustive search's items
    small = Scene("cornell", param0=1)
    ctx.upload_scene(small)
    assert ctx.trace_variant() == capi.TRACE_EXHAUSTIVE
    image, held = render(ctx, small), buffers(ctx)
    assert status_of(ctx, [dict(first=0, tints=one)]) == capi.HIPR_ERROR_UNSUPPORTED and b"upload" in lib.hipr_last_error()
    assert unequal(buffers(ctx), held) == [] and np.array_equal(render(ctx, small), image)
    # ... and another search walked
    ctx.set_trace_variant(capi.TRACE_WIDE_PERSISTENT)
    try:
        scene, info = vu.make_scene()
        ctx.upload_scene(scene)
        assert status_of(ctx, [dict(first=0, tints=one)]) == capi.HIPR_ERROR_UNSUPPORTED
    finally:
        ctx.set_trace_variant(-1)
    # no texcoord or emission pool on the device
    bare = Scene("cornell", param0=4)
    ctx.upload_scene(bare)
    absent = [status_of(ctx, [dict(first=0, texcoords=np.zeros((1, 2), np.float32))]), status_of(ctx, [dict(first=0, emissions=np.zeros((1, 3), np.float32))])]
    assert absent == [capi.HIPR_ERROR_INVALID_ARGUMENT] * 2 and status_of(ctx, [dict(first=0, tints=one)]) == capi.HIPR_OK

    ctx.upload_scene(scene)
    image, held = render(ctx, scene), buffers(ctx)
    count = scene.desc.vertex_count
    good = dict(first=3, tints=one)
    bad_position = vu.pooled(scene, [vu.geometry_edit(scene, info, "lace", 0, 2)])[0]
    bad_position["geometry"]["position"][1, 2] = np.nan
    refused = [
        status_of(ctx, [good], null_out=True),
        status_of(ctx, [good], null_edits=True),
        status_of(ctx, [good, dict(first=0, count=0, tints=one)]),                                 # no vertices
        status_of(ctx, [good, dict(first=0, count=1)]),                                            # no attribute
        status_of(ctx, [good, dict(first=count, tints=one)]),                                      # begins past the pool
        status_of(ctx, [good, dict(first=count - 1, tints=np.zeros(2, np.uint32))]),               # reaches past the pool
        status_of(ctx, [good, dict(first=0xFFFFFFFF, tints=np.zeros(2, np.uint32))]),              # first + count wraps around 32 bits
        status_of(ctx, [good, bad_position]),
        status_of(ctx, [good, dict(first=0, texcoords=np.array([[0.0, np.inf]], np.float32))]),
    ]
    assert refused == [capi.HIPR_ERROR_INVALID_ARGUMENT] * len(refused), refused
    assert unequal(buffers(ctx), held) == [] and np.array_equal(render(ctx, scene), image)
    # an empty list is served and changes nothing
    assert status_of(ctx, []) == capi.HIPR_OK and unequal(buffers(ctx), held) == []
    # the BVH2 and the 4-wide arrays go stale with an edit of geometry, as after a device refit; an edit of tints leaves them
    assert status_of(ctx, [good]) == capi.HIPR_OK and lib.hipr_set_trace_variant(ctx.handle, capi.TRACE_BVH2) == 0
    ctx.set_trace_variant(-1)
    assert status_of(ctx, vu.pooled(scene, [vu.geometry_edit(scene, info, "box", 0, 1, move=(0.01, 0.0, 0.0))])) == capi.HIPR_OK
    assert lib.hipr_set_trace_variant(ctx.handle, capi.TRACE_BVH2) != 0
    ctx.set_trace_variant(-1)


def life_afterwards(scene, info, ctx=None, fresh=None):
    """A vertex edit, then every other writer of the resident scene, each followed in the builder; with contexts, the device follows and is held to a fresh upload
    after every step (without, the builder's side alone runs: the CPU suite's dry run of this script)."""
    def check(answer=None):
        if ctx is not None:
            same_as_a_fresh_upload(ctx, fresh, scene, answer)

    def vertex_edit(edits):
        if ctx is not None:
            check(applied_on_both(ctx, scene, info, edits))
        else:
            assert scene.update_vertices(edits, NEVER_REBUILD) is True

    vertex_edit([vu.geometry_edit(scene, info, "lace", 0, 289, move=vu.wobble(21)), vu.onto_the_hole(scene, info, 100, 4)])
    # a device refit
    pose = dict(translation=(-0.15, 0.0, -0.2), rotation=(0.0, 0.0, 0.0, 1.0), scale=0.2)
    if ctx is not None:
        assert not ctx.refit_scene_transforms(scene.model_pose(vu.BOX_A, **pose))["needs_rebuild"]
    assert scene.move_model(vu.BOX_A, rebuild_threshold=NEVER_REBUILD, **pose) is True
    check()
    vertex_edit([vu.geometry_edit(scene, info, "box", 2, 3, move=vu.wobble(22, 0.1))])
    # a material edit: the lace's material no longer cuts out
    materials = [(info["cutout"], pg.material(tint=(0.2, 0.9, 0.3)))]
    if ctx is not None:
        ctx.update_scene_materials(materials)
    assert scene.update_materials(materials) is True
    check()
    materials = [(info["cutout"], pg.material(flags=capi.MATERIAL_THIN_WALLED | capi.MATERIAL_CUTOUT, coverage=0.5, coverage_texture=1))]
    if ctx is not None:
        ctx.update_scene_materials(materials)
    assert scene.update_materials(materials) is True
    check()
    # a texel edit: the hole closed
    texels = [(1, 24, 24, np.full((8, 8), 255, np.uint8))]
    if ctx is not None:
        assert ctx.update_scene_texels(texels)["status"] == capi.HIPR_OK
    assert scene.update_texels(texels) is True
    check()
    vertex_edit([vu.lace_texcoords(scene, info, 100, 4)])
    # an instance edit: a model leaves
    assert scene.remove_model(vu.BOX_B)
    edits = scene.staged_instance_edits()
    assert edits is not None
    if ctx is not None:
        edited = ctx.edit_scene_instances(edits)
        assert edited["status"] == capi.HIPR_OK, ctx.lib.hipr_last_error()
        assert scene.adopt_edited_trees(edited["nodes"], edited["order"], edited["deepest"], edited["slots"], edited["wide8"])
    else:
        scene.rebuild()
    check()
    vertex_edit([vu.geometry_edit(scene, info, "glowing", 0, 8, move=vu.wobble(23))])
    # a pool growth: a model over a new mesh, whose vertices are then edited
    info["mesh"]["appended"] = scene.add_mesh(**vu.mesh_data()["box"])
    assert scene.insert_model(1000, info["mesh"]["appended"], info["plain"], model_index=301, **pg.IN_THE_BOX) == 301
    growth, edits = scene.staged_scene_growth()
    if ctx is not None:
        assert ctx.append_scene_pools(growth) == capi.HIPR_OK, ctx.lib.hipr_last_error()
        edited = ctx.edit_scene_instances(edits)
        assert edited["status"] == capi.HIPR_OK, ctx.lib.hipr_last_error()
        assert scene.adopt_edited_trees(edited["nodes"], edited["order"], edited["deepest"], edited["slots"], edited["wide8"])
    else:
        scene.rebuild()
    check()
    vertex_edit([vu.geometry_edit(scene, info, "appended", 0, 8, move=vu.wobble(24, 0.2))])


def test_the_other_writers_serve_the_scene_after_a_vertex_edit_and_it_serves_theirs(ctx, fresh):
    scene, info = vu.make_scene()
    ctx.upload_scene(scene)
    life_afterwards(scene, info, ctx, fresh)
    assert np.array_equal(render(ctx, scene).view(np.uint64), render(fresh, scene).view(np.uint64))


def test_a_group_of_one_device_updates_like_a_single_context(ctx, fresh):
    lib = ctx.lib
    scene, info = vu.make_scene()
    host_edits = [vu.geometry_edit(scene, info, "box", 0, 8, move=vu.wobble(31, 0.1)), vu.onto_the_hole(scene, info, 0, 3)]
    edits = vu.pooled(scene, host_edits)
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
        assert status_of(ctx, edits + [dict(first=scene.desc.vertex_count, tints=np.zeros(1, np.uint32))], group=group) == capi.HIPR_ERROR_INVALID_ARGUMENT
        assert status_of(ctx, edits, group=group, null_out=True) == capi.HIPR_ERROR_INVALID_ARGUMENT
        assert unequal(buffers(member), uploaded) == []
        moved, candidates = vu.expected_counts(scene, info, host_edits)
        answer = ctx.update_scene_vertices(edits, group=group)
        assert answer["status"] == capi.HIPR_OK and (answer["moved_triangles"], answer["candidate_triangles"]) == (moved, candidates) and not answer["all_triangles_opaque"]
        assert scene.update_vertices(host_edits, NEVER_REBUILD) is True
        fresh.upload_scene(scene)
        assert unequal(buffers(member), buffers(fresh)) == []
    finally:
        member.handle = C.c_void_p()      # nothing of the group's is closed through the borrowed handle
        lib.hipr_group_destroy(group)
