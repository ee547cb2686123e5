"""hipr_update_scene_vertices without a GPU: the bodies of csrc/vertex_update.h compiled for the host (tests/native/VertexUpdateHost.hip) and walked in the kernels'
shape -- the staging plan, the word writes block by block with threads backwards, the marked triangles with the bounds, the refit of the tree, the flags, the leaf
pass -- must leave, byte for byte, what SceneBuilder::update_vertices leaves; stage_vertex_edits + apply_staged_transforms must leave the same; and a builder made
anew from the edited mesh data must agree in the pools and, triangle by triangle, in corners and flags (its trees are another build and are not compared). The trace
and shading records are built by the kernels of triangle_records.h and are the GPU suite's business."""
import numpy as np
import pytest

import material_update_bindings as mu
import vertex_update_bindings as vu
from bifrost3d_amd import capi

NEVER_REBUILD = 1e30      # the ratio rule is the caller's policy: the device refits whatever the area


def assert_held_equals(held, scene, what):
    d = scene.desc
    trace, shade, classes = mu.derived_arrays(scene)
    for name in capi.VERTEX_ATTRIBUTES:
        assert np.array_equal(held[name].view(np.uint8), vu.pool(scene, name).view(np.uint8)), (what, name)
    assert np.array_equal(held["triangles"], scene.triangles()), what
    assert np.array_equal(held["slots"], scene.wide8_slots()), what
    assert np.array_equal(held["trace"], trace) and np.array_equal(held["shade"], shade) and np.array_equal(held["classes"], classes), what
    assert np.array_equal(held["grid_min"].view(np.uint32), np.array(d.wide8_grid_min[:], np.float32).view(np.uint32)), what
    assert np.array_equal(held["grid_cell"].view(np.uint32), np.array(d.wide8_grid_cell[:], np.float32).view(np.uint32)), what


def by_instance_and_primitive(scene):
    triangles = scene.triangles()
    return triangles[np.lexsort((triangles[:, 10], triangles[:, 9]))]


def edited_mesh_data(info, applied):
    """info["data"] with the edits of `applied` (mesh-relative, with the scene's mesh indices) written into it. Geometry edits carry packed normals, which mesh data
    does not take back: the cases this is used for leave normals alone or are compared in the pools through the packed words."""
    name_of = {index: name for name, index in info["mesh"].items()}
    data = {name: {k: np.array(v, copy=True) for k, v in mesh.items()} for name, mesh in info["data"].items()}
    for e in applied:
        mesh = data[name_of[e["mesh"]]]
        first = e["first"]
        if e.get("geometry") is not None:
            mesh["positions"][first:first + len(e["geometry"])] = e["geometry"]["position"]
        if e.get("texcoords") is not None:
            mesh["texcoords"][first:first + len(e["texcoords"])] = e["texcoords"]
    return data


@pytest.mark.parametrize("name", vu.CASE_IDS)
def test_the_passes_leave_what_the_builder_leaves(name):
    scene, info = vu.make_scene()
    staged, _ = vu.make_scene()
    held = vu.arrays_of(scene)
    applied = []
    for host_edits, device_edits in vu.CASES[name](scene, info):
        moved, candidates = vu.expected_counts(scene, info, host_edits)
        flags_before = scene.triangles()[:, 11]
        answer = vu.run_kernel_bodies(scene, held, device_edits if device_edits is not None else vu.pooled(scene, host_edits))
        assert scene.update_vertices(host_edits, NEVER_REBUILD) is True
        assert_held_equals(held, scene, "against SceneBuilder::update_vertices")
        flags = scene.triangles()[:, 11]
        assert (answer["moved"], answer["decided"], answer["changed"]) == (moved, candidates, int((flags != flags_before).sum())), answer
        assert answer["all_opaque"] == bool((flags & capi.TRIANGLE_OPAQUE != 0).all()) and not answer["needs_rebuild"]
        # the device path's companion: the edits staged, then applied
        pooled = staged.stage_vertex_edits(host_edits)
        assert [e["first"] for e in pooled] == [e["first"] for e in vu.pooled(scene, host_edits)]
        assert staged.apply_staged(NEVER_REBUILD) is True
        assert_held_equals(held, staged, "against stage_vertex_edits + apply_staged_transforms")
        applied += host_edits
    if name in ("normals_only", "tints_and_emissions", "first_and_last_vertex_of_the_pool"):
        return      # mesh data takes normals as vectors and no Cornell wall: the builder made anew is the other cases'
    anew, _ = vu.make_scene(edited_mesh_data(info, applied))
    for attribute in capi.VERTEX_ATTRIBUTES:
        assert np.array_equal(vu.pool(scene, attribute).view(np.uint8), vu.pool(anew, attribute).view(np.uint8)), attribute
    assert np.array_equal(by_instance_and_primitive(scene), by_instance_and_primitive(anew))


def test_the_plan_resolves_overlaps_into_disjoint_segments_where_the_later_edit_wins():
    ones, twos, threes = np.full(10, 1, np.uint32), np.full(10, 2, np.uint32), np.full(1, 3, np.uint32)
    segments, words = vu.plan_of([dict(first=0, tints=ones), dict(first=5, tints=twos), dict(first=2, tints=threes, texcoords=np.zeros((1, 2), np.float32))])
    # texcoords first (pool 1: vertex 2 = word 4), then the tints [0, 2) of the first edit, [2, 3) of the third, [3, 5) of the first, [5, 15) of the second
    assert segments.tolist() == [[0, 1, 4], [2, 2, 0], [4, 2, 2], [5, 2, 3], [7, 2, 5]] and words == 17
    # an edit wholly covered by a later one leaves no segment; one that covers a later one's neighbours is split around it
    segments, words = vu.plan_of([dict(first=4, tints=threes), dict(first=0, tints=ones), dict(first=20, emissions=np.zeros((2, 3), np.float32))])
    assert segments.tolist() == [[0, 2, 0], [10, 3, 60]] and words == 16


def test_many_small_edits_cross_block_and_wave_boundaries():
    """300 one-vertex tint edits and a long geometry range: blocks of 256 words that hold 256 segments, a segment that spans blocks."""
    scene, info = vu.make_scene()
    held = vu.arrays_of(scene)
    rng = np.random.default_rng(12)
    vertices = rng.permutation(scene.desc.vertex_count)[:300]
    edits = [dict(first=int(v), tints=np.array([0x01000000 + int(v)], np.uint32)) for v in vertices] + [dict(first=1, emissions=rng.uniform(0, 1, (380, 3)).astype(np.float32))]
    before = {name: held[name].copy() for name in ("geometry", "texcoords", "triangles", "slots")}
    answer = vu.run_kernel_bodies(scene, held, edits)
    expected = vu.pool(scene, "tints")
    expected[vertices, 0] = 0x01000000 + vertices
    assert np.array_equal(held["tints"], expected) and np.array_equal(held["emissions"][1:381], edits[-1]["emissions"])
    assert np.array_equal(held["emissions"][0], vu.pool(scene, "emissions")[0]) and np.array_equal(held["emissions"][381:], vu.pool(scene, "emissions")[381:])
    assert all(np.array_equal(held[name], before[name]) for name in before) and answer["moved"] == 0


def test_parted_seam_vertices_ask_for_a_rebuild_on_both_sides():
    scene, info = vu.make_scene()
    held = vu.arrays_of(scene)
    edits = [vu.geometry_edit(scene, info, "seam", 1, 1, move=(0.0, 0.0, 0.3))]
    answer = vu.run_kernel_bodies(scene, held, vu.pooled(scene, edits))
    assert answer["needs_rebuild"] and answer["moved"] == 1
    assert scene.update_vertices(edits, NEVER_REBUILD) is False      # rebuilt: a leaf record could not be refitted
    assert np.array_equal(held["geometry"], vu.pool(scene, "geometry"))
    assert np.array_equal(held["triangles"][np.lexsort((held["triangles"][:, 10], held["triangles"][:, 9]))], by_instance_and_primitive(scene))


def test_the_builder_refuses_what_the_device_refuses():
    scene, info = vu.make_scene()
    before = vu.arrays_of(scene)
    lace, one = info["mesh"]["lace"], np.zeros(1, np.uint32)
    bad_position = vu.geometry_edit(scene, info, "lace", 0, 1)
    bad_position["geometry"]["position"][0, 1] = np.inf
    refused = [[dict(mesh=99, first=0, tints=one)], [dict(mesh=lace, first=289, tints=one)], [dict(mesh=lace, first=288, tints=np.zeros(2, np.uint32))], [dict(mesh=lace, first=0, count=0, tints=one)],
               [dict(mesh=lace, first=0, count=1)], [bad_position], [dict(mesh=lace, first=0, texcoords=np.array([[np.nan, 0.0]], np.float32))],
               [dict(mesh=lace, first=0, tints=one), dict(mesh=lace, first=0xFFFFFFFF, tints=np.zeros(2, np.uint32))]]
    for edits in refused:
        assert scene.update_vertices(edits) is None, edits
        assert scene.stage_vertex_edits(edits) is None, edits
    after = vu.arrays_of(scene)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    # a mesh added since the last build is not the device's yet
    added = scene.add_mesh(**vu.mesh_data()["box"])
    assert scene.update_vertices([dict(mesh=added, first=0, tints=one)]) is None
    # a scene whose pools lack an attribute refuses it
    from bifrost3d_amd.host import Scene
    bare = Scene("cornell", param0=4)
    assert bare.desc.tints and not bare.desc.texcoords and not bare.desc.emissions
    assert bare.update_vertices([dict(mesh=0, first=0, texcoords=np.zeros((1, 2), np.float32))]) is None and bare.update_vertices([dict(mesh=0, first=0, emissions=np.zeros((1, 3), np.float32))]) is None
    assert bare.update_vertices([dict(mesh=0, first=0, tints=one)]) is True


def test_the_builders_side_of_the_script_of_edits_among_the_other_writers():
    """tests/test_gpu_vertex_update.py's sequence -- vertex edits between a refit, material edits, a texel edit, an instance edit and a pool growth -- on the builder
    alone: it must end where a rebuild of the same builder ends, triangle by triangle."""
    from test_gpu_vertex_update import life_afterwards
    scene, info = vu.make_scene()
    life_afterwards(scene, info)
    left = by_instance_and_primitive(scene)
    scene.rebuild()
    assert np.array_equal(left, by_instance_and_primitive(scene))
