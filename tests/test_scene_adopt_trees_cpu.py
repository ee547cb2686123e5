"""SceneBuilder::adopt_rebuilt_trees on the CPU: a builder that is handed the trees a rebuild made of its scene -- by the device (hipr_rebuild_scene_trees), here by
another builder -- must leave, in every array and scalar of its description, what its own rebuild() leaves, without a flatten and without a refit. Every equality
is of bytes. The first test holds the three moves of the device rebuild's tests to what makes them tests: the host alone stays inside every condition the device
refuses on, and no new tree equals the old one."""
import numpy as np
import pytest

import device_rebuild_bindings as rb
import device_refit_bindings as refit
import material_update_bindings as mu


def wide8_result(scene):
    """The HiprWide8BuildResult of a scene's 8-wide tree, counted from its slots."""
    slots, d = scene.wide8_slots(), scene.desc
    is_node, _ = refit.decode_tree(slots)
    leaves = slots[~is_node]
    return dict(slot_count=len(slots), height=d.wide8_height, grid_min=np.array(d.wide8_grid_min[:], np.float32), grid_cell=np.array(d.wide8_grid_cell[:], np.float32),
                node_count=int(is_node.sum()), leaf_count=len(leaves), paired_leaves=int((leaves[:, 13] != 0xFFFFFFFF).sum()))


def trees_of(scene):
    return dict(nodes=scene.nodes(), order=scene.order(), deepest=scene.desc.bvh_max_depth - 1, slots=scene.wide8_slots(), wide8=wide8_result(scene))


@pytest.mark.parametrize("name, arguments, model, pose, uploaded, rebuilt, kept_at_the_rule", rb.MOVES, ids=rb.MOVE_IDS)
def test_the_three_moves_stay_inside_every_condition_and_change_the_tree(name, arguments, model, pose, uploaded, rebuilt, kept_at_the_rule):
    scene = rb.make_scene(arguments)
    d = scene.desc
    assert (d.triangle_count, d.node_count, d.wide8_slot_count) == uploaded
    assert d.node_count > 64 and 0 < d.wide8_height <= 33      # the 8-wide search is the one an upload selects
    before = rb.description(scene)
    assert scene.move_model(model, **pose) is kept_at_the_rule      # the 1.5 rule, or a pair that parted: the host rebuilds
    d = scene.desc
    assert (d.node_count, d.wide8_slot_count) == rebuilt
    assert d.wide8_height <= 33 and d.bvh_max_depth <= 64
    assert scene.build_counts()["longest_median_range"] <= 64      # no range the device build declines
    after = rb.description(scene)
    assert {"nodes", "wide8_slots", "triangles", "order"} <= set(rb.differences(before, after))      # no new tree equals the old one
    # the topology kept as far as it can be, then rebuild(): the builder's own rebuild
    other = rb.make_scene(arguments)
    kept = other.move_model(model, rebuild_threshold=1e30, **pose)
    assert kept is (name != "atrium_parting_pair")      # a parted pair rebuilds whatever the threshold
    other.rebuild()
    assert rb.differences(after, rb.description(other)) == []
    if name == "cornell_far":
        assert d.wide8_height == 4 and d.bvh_max_depth == 11
    if name == "atrium_far":
        assert d.bvh_max_depth == 20


@pytest.mark.parametrize("name, arguments, model, pose, uploaded, rebuilt, kept_at_the_rule", rb.MOVES, ids=rb.MOVE_IDS)
def test_adopted_trees_leave_what_a_rebuild_leaves(name, arguments, model, pose, uploaded, rebuilt, kept_at_the_rule):
    a, b = rb.make_scene(arguments), rb.make_scene(arguments)
    assert a.move_model(model, **pose) is False      # moved and rebuilt on the host
    assert b.stage_model(model, **pose) is True      # the pose in the instances only
    assert b.adopt_trees(**trees_of(a)) is True
    assert rb.differences(rb.description(a), rb.description(b)) == []
    assert b.rebuild_counts() == dict(adopted=1, refused=0) and b.build_counts()["device_builds"] == 0 and b.collapse_counts()["device_collapses"] == 0
    # life afterwards: a later move and a later material edit on both
    assert a.move_model(model, rebuild_threshold=1e30, **rb.POSE) == b.move_model(model, rebuild_threshold=1e30, **rb.POSE)
    assert rb.differences(rb.description(a), rb.description(b)) == []
    which = "cornell" if arguments[0] == "cornell" else "atrium"
    assert a.update_materials(*mu.edit_of(a, which, "together")) and b.update_materials(*mu.edit_of(b, which, "together"))
    assert rb.differences(rb.description(a), rb.description(b)) == []


def test_adoption_without_a_move_reproduces_the_scene():
    a, b = rb.make_scene(rb.MOVES[0][1]), rb.make_scene(rb.MOVES[0][1])
    assert b.adopt_trees(**trees_of(a)) is True
    assert rb.differences(rb.description(a), rb.description(b)) == []


def test_refusals_leave_the_builder_untouched():
    arguments, model, pose = rb.MOVES[0][1], rb.MOVES[0][2], rb.MOVES[0][3]
    a, b = rb.make_scene(arguments), rb.make_scene(arguments)
    assert a.move_model(model, **pose) is False
    before = rb.description(b)
    good = trees_of(a)

    def refused(**changed):
        trees = dict(good)
        trees.update(changed)
        return b.adopt_trees(**trees) is False

    twice = good["order"].copy()
    twice[1] = twice[0]
    assert refused(order=twice)                                  # no permutation
    beyond = good["order"].copy()
    beyond[0] = len(beyond)
    assert refused(order=beyond)
    assert refused(order=good["order"][:-1])                     # counts that do not fit
    assert refused(nodes=np.zeros((0, 16), np.uint32))
    assert refused(nodes=np.concatenate([good["nodes"]] * 3))
    child = good["nodes"].copy()
    child[0, 12] = len(child)                                    # a child index out of range (HiprBvhNode::child[0])
    assert refused(nodes=child)
    leaf = good["nodes"].copy()
    inner = np.nonzero(leaf[:, 12].view(np.int32) < 0)[0][0]
    leaf[inner, 12] = np.uint32(~np.uint32((len(good["order"]) << 3) | 2))      # a leaf range past the triangles
    assert refused(nodes=leaf)
    slots = good["slots"].copy()
    is_node, _ = refit.decode_tree(slots)
    record = np.nonzero(~is_node)[0][0]
    slots[record, 12] = len(good["order"])                       # a record's triangle out of range (HiprLeaf8::triangle[0])
    assert refused(slots=slots)
    short = dict(good["wide8"], slot_count=len(good["slots"]) - 1)
    assert refused(slots=good["slots"][:-1], wide8=short)        # a child slot out of range
    assert rb.differences(before, rb.description(b)) == []
    assert b.rebuild_counts() == dict(adopted=0, refused=9)
    # ... and the builder still adopts the trees that fit
    assert b.stage_model(model, **pose) is True and b.adopt_trees(**good) is True
    assert rb.differences(rb.description(a), rb.description(b)) == []


def test_the_scene_the_device_build_declines(tmp_path):
    from bifrost3d_amd.host import Scene
    scene = Scene("file:" + rb.write_decline_obj(tmp_path / "decline.obj"))
    assert scene.build_counts()["longest_median_range"] == 300
    assert scene.desc.node_count > 64 and 0 < scene.desc.wide8_height <= 33
