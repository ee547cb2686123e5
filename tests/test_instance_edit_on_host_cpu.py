"""Models of a built scene removed and created on the host (SceneBuilder::remove_model / insert_model), and the routines of hipr_edit_scene_instances
(csrc/instance_edit.h) walked on the host in the kernels' shape (tests/native/InstanceEditHost.hip), chained with the walks of the BVH2 build and the 8-wide collapse,
against the same operations followed by SceneBuilder::rebuild(). The input of the walk is what the device holds: the triangles and class bytes of the scene BEFORE the
edit in its tree's order, its pools and its instances, and the new instance list. Every equality is of bytes.

The banners of the textured atrium are cut-outs through a coverage texture: a new banner's flags go through covered_everywhere over the texel pool (which finds none of
its triangles wholly on solid texels at this tessellation; the host says the same)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import device_rebuild_bindings as rb
import instance_edit_bindings as ie
import material_update_bindings as mu
from bifrost3d_amd import capi

REPO = Path(__file__).resolve().parent.parent


def walked(before, staged):
    """The routines over what the device holds of `before`, for the edits staged in `staged`."""
    edits = staged.staged_instance_edits()
    assert edits is not None
    return ie.routines_edit(before.triangles(), mu.derived_arrays(before)[2], before.desc, edits), edits


def test_a_model_removed_and_inserted_again_at_its_place_gives_back_the_description():
    scene = ie.prepared(ie.ATRIUM, [("insert", 9, 30, 11, ie.NEAR, 150)])
    original = rb.description(scene)
    info = scene.model_info(150)
    assert info["position"] == 9
    assert scene.remove_model(150) and not scene.remove_model(150)
    assert scene.insert_model(9, info["mesh"], info["material"], model_index=150, **ie.NEAR) == 150
    scene.rebuild()
    assert rb.differences(rb.description(scene), original) == []


def test_a_last_model_removed_leaves_the_scene_that_never_had_it():
    never = rb.make_scene(ie.ATRIUM)
    scene = ie.prepared(ie.ATRIUM, [("insert", 1000, 6, None, ie.NEAR, 151)])
    assert scene.desc.triangle_count == never.desc.triangle_count + 294
    assert scene.remove_model(151)
    scene.rebuild()
    assert rb.differences(rb.description(scene), rb.description(never)) == []      # a copy of a resident mesh under a resident material: every pool agrees as well


@pytest.mark.parametrize("name, arguments, prepare, operations, counts, switches", ie.EDITS, ids=ie.EDIT_IDS)
def test_the_edits_walked_on_the_host_and_adopted_leave_what_rebuild_leaves(name, arguments, prepare, operations, counts, switches):
    before, staged, host = ie.prepared(arguments, prepare), ie.prepared(arguments, prepare), ie.edited_on_the_host(arguments, prepare, operations)
    d = host.desc
    assert (d.triangle_count, d.node_count, d.wide8_slot_count) == counts and d.node_count > 64 and ie.switches(host) == switches
    ie.apply(staged, operations)
    answer, edits = walked(before, staged)
    assert answer["status"] == ie.EDITED
    assert len(edits) == d.instance_count
    assert np.array_equal(answer["order"], host.order()) and np.array_equal(answer["nodes"], host.nodes())
    assert np.array_equal(answer["triangles"], host.triangles()) and np.array_equal(answer["classes"], mu.derived_arrays(host)[2])
    assert np.array_equal(answer["slots"], host.wide8_slots())
    result = answer["result"]
    assert (int(result[0]), int(result[1]), int(result[2]) + 1, int(result[3]), int(result[4])) == (d.triangle_count, d.node_count, d.bvh_max_depth, d.wide8_slot_count, d.wide8_height)
    assert np.array_equal(result[5:11], np.array(list(d.wide8_grid_min[:]) + list(d.wide8_grid_cell[:]), np.float32).view(np.uint32))
    assert (bool(result[14]), bool(result[15])) == switches
    # the builder takes the trees over without a flatten of the whole scene
    assert staged.adopt_edited_trees(answer["nodes"], answer["order"], int(result[2]), answer["slots"], ie.wide8_of(result))
    assert rb.differences(rb.description(staged), rb.description(host)) == []
    assert staged.rebuild_counts() == dict(adopted=1, refused=0) and staged.staged_instance_edits() is not None and len(staged.staged_instance_edits()) == d.instance_count


def test_the_switches_flip_where_the_edits_say():
    by_name = {e[0]: e for e in ie.EDITS}
    _, arguments, prepare, _, _, after = by_name["textured_remove_every_cutout"]
    assert ie.switches(ie.prepared(arguments, prepare)) == (False, True) and after == (True, True)
    _, arguments, prepare, _, _, after = by_name["atrium_first_coated"]
    assert ie.switches(ie.prepared(arguments, prepare)) == (True, False) and after == (True, True)


def test_trees_that_do_not_fit_the_edited_list_are_refused_untouched():
    name, arguments, prepare, operations, counts, switches = ie.EDITS[1]
    before, staged, host = ie.prepared(arguments, prepare), ie.prepared(arguments, prepare), ie.edited_on_the_host(arguments, prepare, operations)
    ie.apply(staged, operations)
    d = host.desc
    wide8 = capi.HiprWide8BuildResult(d.wide8_slot_count, d.wide8_height, d.wide8_grid_min, d.wide8_grid_cell, 0, 0, 0)
    assert not staged.adopt_edited_trees(before.nodes(), before.order(), before.desc.bvh_max_depth - 1, before.wide8_slots(), wide8)      # the OLD order: another count
    twice = host.order().copy()
    twice[3] = twice[4]
    assert not staged.adopt_edited_trees(host.nodes(), twice, d.bvh_max_depth - 1, host.wide8_slots(), wide8)      # no permutation
    assert staged.rebuild_counts() == dict(adopted=0, refused=2)
    assert staged.adopt_edited_trees(host.nodes(), host.order(), d.bvh_max_depth - 1, host.wide8_slots(), wide8)
    assert rb.differences(rb.description(staged), rb.description(host)) == []


def test_a_new_mesh_or_a_staged_move_is_not_the_devices():
    scene = rb.make_scene(ie.CORNELL)
    assert len(scene.staged_instance_edits()) == 7      # nothing staged: the list as it stands
    assert scene.stage_model(6, **rb.POSE)
    assert scene.staged_instance_edits() is None        # a move in the same tick: the full path
    scene.rebuild()
    ie.apply(scene, [("remove", 7)])
    edits = scene.staged_instance_edits()
    assert [e.source for e in edits] == [0, 1, 2, 3, 4, 5]
    mirrored = dict(ie.NEAR, scale=-0.7)      # a mirrored copy needs index triples the pools do not hold yet: the index pool grows
    info = scene.model_info(6)
    scene.insert_model(2, info["mesh"], info["material"], model_index=160, **mirrored)
    assert scene.staged_instance_edits() is None
    scene.rebuild()
    assert len(scene.staged_instance_edits()) == 7


def test_the_host_build_of_the_routines_refuses_untouched():
    # a BVH2 of at most 64 nodes: a fresh upload would choose another search
    _, arguments, prepare, operations, _, _ = ie.TOO_SMALL
    before, staged = ie.prepared(arguments, prepare), ie.prepared(arguments, prepare)
    ie.apply(staged, operations)
    answer, edits = walked(before, staged)
    assert answer["status"] == ie.TOO_FEW_NODES and ie.untouched(answer)
    host = ie.edited_on_the_host(arguments, prepare, operations)
    assert host.desc.node_count <= 64
    # a position claimed twice (and with it one claimed not at all)
    staged = ie.prepared(*ie.EDITS[0][1:3])
    ie.apply(staged, ie.EDITS[0][3])
    resident, classes = before.triangles(), mu.derived_arrays(before)[2]
    twice = resident.copy()
    of_first = np.nonzero(twice[:, 9] == 0)[0]
    twice[of_first[0], 10] = twice[of_first[1], 10]
    answer = ie.routines_edit(twice, classes, before.desc, staged.staged_instance_edits())
    assert answer["status"] == ie.CLAIMED and ie.untouched(answer)
    # a vertex index of a new instance outside the pool: refused before the vertex is loaded
    staged = rb.make_scene(ie.CORNELL)
    ie.apply(staged, [("insert", 3, 7, None, ie.NEAR, 170)])
    edits = staged.staged_instance_edits()
    new = [e for e in edits if e.source == capi.EDIT_NEW_INSTANCE][0]
    pools = capi.HiprSceneDesc.from_buffer_copy(bytes(before.desc))
    indices = np.ctypeslib.as_array(before.desc.indices, shape=(before.desc.index_count,)).copy()
    indices[3 * (new.instance.index_offset + 5) + 2] = before.desc.vertex_count - new.instance.vertex_offset      # one past the pool, seen from the instance
    pools.indices = indices.ctypes.data_as(C.POINTER(C.c_uint32))
    answer = ie.routines_edit(resident, classes, pools, edits)
    assert answer["status"] == ie.BAD_INDEX and ie.untouched(answer)
    assert ie.routines_edit(resident, classes, before.desc, edits)["status"] == ie.EDITED      # the same list over the sound pool
    # a list that yields no triangle
    empty = (capi.HiprInstanceEdit * 1)()
    empty[0].source, empty[0].primitive_count, empty[0].instance = capi.EDIT_NEW_INSTANCE, 0, new.instance
    answer = ie.routines_edit(resident, classes, before.desc, empty)
    assert answer["status"] == ie.NO_TRIANGLE and ie.untouched(answer)


def test_the_walk_under_the_sanitizers():
    """`make sanitize-instance-edit`: the stand-alone program (tests/native/InstanceEditSanitize.cpp) walks its three lists and two refusals under ASan + UBSan on the CPU."""
    done = subprocess.run(["make", "-C", str(REPO / "bifrost3d_amd"), "sanitize-instance-edit"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "3 lists walked" in done.stdout and "an index past the vertex pool: status 4" in done.stdout and "a position claimed twice: status 1" in done.stdout
