"""The routines of the device rebuild of the resident scene's trees (csrc/scene_rebuild.h) walked on the host in the kernels' shape (tests/native/DeviceRebuildHost.hip),
chained with the host walks of the BVH2 build and the 8-wide collapse -- the collapse's level lists handed over from the build's place[] and level sizes, not from the
host's index walk -- against SceneBuilder::rebuild(). The input is what the device holds after its refit: the host's world-space triangles at the new pose, stored in
the OLD tree's order, with their class bytes. Every equality is of bytes."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import device_collapse_bindings as collapse
import device_rebuild_bindings as rb
import material_update_bindings as mu

REPO = Path(__file__).resolve().parent.parent


def in_flatten_order(scene):
    """A scene's triangles and class bytes in the order its builder flattens in."""
    triangles, classes, order = scene.triangles(), mu.derived_arrays(scene)[2], scene.order()
    flat, flat_classes = np.zeros_like(triangles), np.zeros_like(classes)
    flat[order], flat_classes[order] = triangles, classes
    return flat, flat_classes


def untouched(answer, resident, classes):
    return (np.array_equal(answer["triangles"], resident) and np.array_equal(answer["classes"], classes) and (answer["nodes"] == rb.PATTERN).all() and (answer["order"] == rb.PATTERN).all()
            and (answer["slots"] == rb.PATTERN).all() and (answer["result"] == rb.PATTERN).all())


@pytest.mark.parametrize("name, arguments, model, pose, uploaded, rebuilt, kept_at_the_rule", rb.MOVES, ids=rb.MOVE_IDS)
def test_the_three_moves_walked_on_the_host_leave_what_rebuild_leaves(name, arguments, model, pose, uploaded, rebuilt, kept_at_the_rule):
    before, host = rb.make_scene(arguments), rb.make_scene(arguments)
    old_order = before.order()
    assert host.move_model(model, **pose) is False      # moved and rebuilt
    flat, flat_classes = in_flatten_order(host)
    resident, classes = flat[old_order], flat_classes[old_order]      # the moved triangles where the old tree keeps them
    assert not np.array_equal(old_order, host.order())
    answer = rb.routines_rebuild(resident, classes, host.desc.instance_count)
    assert answer["status"] == rb.REBUILT
    d = host.desc
    assert np.array_equal(answer["order"], host.order()) and np.array_equal(answer["nodes"], host.nodes())
    assert np.array_equal(answer["triangles"], host.triangles()) and np.array_equal(answer["classes"], mu.derived_arrays(host)[2])
    different = np.nonzero((answer["slots"] != host.wide8_slots()).any(axis=1))[0] if answer["slots"].shape == host.wide8_slots().shape else [-1]
    assert len(different) == 0, different[:8]
    result = answer["result"]
    assert (int(result[0]), int(result[1]) + 1, int(result[2]), int(result[3])) == (d.node_count, d.bvh_max_depth, d.wide8_slot_count, d.wide8_height)
    assert np.array_equal(result[4:10], np.array(list(d.wide8_grid_min[:]) + list(d.wide8_grid_cell[:]), np.float32).view(np.uint32))
    assert (d.node_count, d.wide8_slot_count) == rebuilt


def two_instances():
    """grid16 twice at the same place as instances 0 and 1, in flatten order: neighbours in a leaf share corners across instances, and must not pair."""
    one = collapse.grid_mesh(16)
    both = np.concatenate([one, one])
    both[:, 9] = np.repeat([0, 1], len(one))
    both[:, 10] = np.tile(np.arange(len(one)), 2)
    return both


def test_a_two_instance_set_stored_in_a_bvh_order():
    flat = two_instances()
    host = collapse.host_collapse(flat)
    classes = (np.arange(len(flat)) % 3 == 0).astype(np.uint8)      # by flatten position
    stored = host["order"][::-1].copy()      # a BVH order, reversed: nothing the flatten scatter may rely on
    answer = rb.routines_rebuild(flat[stored], classes[stored], 2)
    assert answer["status"] == rb.REBUILT
    assert np.array_equal(answer["order"], host["order"]) and np.array_equal(answer["nodes"], host["nodes"])
    assert np.array_equal(answer["triangles"], flat[host["order"]]) and np.array_equal(answer["classes"], classes[host["order"]])
    collapse.same_wide8(collapse.wide8_of_result(answer["slots"], answer["result"][2:]), host["wide8"])
    assert np.array_equal(rb.routines_rebuild(flat, classes, 2)["slots"], answer["slots"])      # the stored order decides nothing


def test_a_position_claimed_twice_raises_the_flag_and_nothing_is_written():
    flat = two_instances()
    classes = np.zeros(len(flat), np.uint8)
    twice = flat.copy()
    twice[5, 10] = twice[6, 10]      # two triangles of instance 0 with one primitive index
    answer = rb.routines_rebuild(twice, classes, 2)
    assert answer["status"] == rb.CLAIMED_TWICE and untouched(answer, twice, classes)
    outside = flat.copy()
    outside[5, 9] = 2      # an instance the scene does not have
    answer = rb.routines_rebuild(outside, classes, 2)
    assert answer["status"] == rb.CLAIMED_TWICE and untouched(answer, outside, classes)
    beyond = flat.copy()
    beyond[5, 10] = len(flat)      # a primitive past its instance's count
    answer = rb.routines_rebuild(beyond, classes, 2)
    assert answer["status"] == rb.CLAIMED_TWICE and untouched(answer, beyond, classes)


def test_a_median_range_longer_than_a_lane_sorts_declines(tmp_path):
    from bifrost3d_amd.host import Scene
    scene = Scene("file:" + rb.write_decline_obj(tmp_path / "decline.obj"))
    assert scene.build_counts()["longest_median_range"] == 300
    resident, classes = scene.triangles(), mu.derived_arrays(scene)[2]
    answer = rb.routines_rebuild(resident, classes, scene.desc.instance_count)
    assert answer["status"] == rb.BUILD_DECLINED and untouched(answer, resident, classes)


def test_the_walk_under_the_sanitizers():
    """`make sanitize-device-rebuild`: the stand-alone program (tests/native/DeviceRebuildSanitize.cpp) walks its three sets and a duplicate position under ASan + UBSan on the CPU."""
    done = subprocess.run(["make", "-C", str(REPO / "bifrost3d_amd"), "sanitize-device-rebuild"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "3 sets walked" in done.stdout and "a position claimed twice: status 1" in done.stdout
