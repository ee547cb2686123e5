"""hipr_set_scene_rigs / hipr_pose_scene_rigs without a GPU: the text of csrc/vertex_pose.h compiled for the host (tests/native/VertexPoseHost.hip) -- its restatement
of the octahedral encoder against the project's own, its chain against an independent float64 statement of linear-blend skinning with morph targets written here,
the exact cases, and the kernel's walk (the block table, blocks and threads backwards, both matrix paths) against Scene.posed_geometry, Scene.pose_rigs and the
staged path, byte for byte in every array the builder hands out -- and every refusal of SceneBuilder::set_rigs and pose_rigs."""
import ctypes as C

import numpy as np
import pytest

import vertex_pose_bindings as vp
import vertex_update_bindings as vu
from bifrost3d_amd import capi
from bifrost3d_amd.host import load_host_library
from test_vertex_update_on_host_cpu import assert_held_equals, by_instance_and_primitive

NEVER_REBUILD = 1e30


def project_encoder(normals):
    normals = np.ascontiguousarray(normals, np.float32)
    out = np.zeros((len(normals), 2), np.int16)
    load_host_library().hiprh_encode_octahedral(normals.ctypes.data_as(C.POINTER(C.c_float)), len(normals), out.ctypes.data_as(C.POINTER(C.c_short)))
    return out


def normalised32(normals):
    """n / sqrt((x x + y y) + z z) in float32, every operation rounded once: the header's normalisation."""
    n = np.ascontiguousarray(normals, np.float32)
    d = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    return (n / np.sqrt(d)[:, None]).astype(np.float32)


def decode64(codes):
    """OctahedralNormal::decode in float64."""
    f = codes.astype(np.float64)
    z = 32767.0 - np.abs(f[:, 0]) - np.abs(f[:, 1])
    t = np.maximum(-z, 0.0)
    n = np.stack([f[:, 0] + np.where(f[:, 0] >= 0, -t, t), f[:, 1] + np.where(f[:, 1] >= 0, -t, t), z], axis=1)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def angles(a, b):
    a, b = a / np.linalg.norm(a, axis=1, keepdims=True), b / np.linalg.norm(b, axis=1, keepdims=True)
    return 2.0 * np.arcsin(np.minimum(np.linalg.norm(a - b, axis=1) / 2.0, 1.0))


def test_the_restated_encoder_equals_the_projects_in_both_words():
    unit = lambda v: (np.asarray(v, np.float64) / np.linalg.norm(np.asarray(v, np.float64), axis=1, keepdims=True)).astype(np.float32)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    diagonals = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    ring = np.linspace(0.0, 2.0 * np.pi, 97)
    fold = np.stack([np.cos(ring), np.sin(ring), np.zeros_like(ring)], axis=1)
    below = fold + np.array([0.0, 0.0, -1e-7])
    minus_zero = fold.astype(np.float32) + np.array([0.0, 0.0, -0.0], np.float32)
    minus_zero[:, 2] = np.float32(-0.0)
    tiny = np.array([[1.0, 1e-30, 1e-30], [1e-30, -1.0, 1e-30], [1e-30, 1e-30, -1.0], [1.0, 1e-42, -1e-42], [-1e-42, 1.0, 1e-45], [1e-45, -1e-45, 1.0], [-1.0, 1e-39, -1e-30]], np.float32)
    random = unit(np.random.default_rng(2026).normal(size=(100000, 3)))
    normals = np.concatenate([unit(axes), unit(diagonals), unit(fold), unit(below), minus_zero, tiny, random]).astype(np.float32)
    ours, theirs = vp.encode(normals), project_encoder(normals)
    assert np.array_equal(ours, theirs), np.flatnonzero((ours != theirs).any(axis=1))[:10]


# ---- the independent statement: float64 linear-blend skinning with morph targets. It does not call the header. ----
def skinned64(rig, pose):
    """(positions, normals or None, the bound's sum per vertex: sum_k w_k (|M_k| |p| + |t_k|) with |p| = |rest| + sum_t |w_t| |dp_t|) in float64."""
    p = np.asarray(rig["rest_positions"], np.float64).copy()
    p_abs = np.abs(p)
    n = None if rig.get("rest_normals") is None else np.asarray(rig["rest_normals"], np.float64).copy()
    for t, w in enumerate(np.asarray(pose.get("weights", []), np.float64)):
        p += w * np.asarray(rig["target_positions"][t], np.float64)
        p_abs += abs(w) * np.abs(np.asarray(rig["target_positions"][t], np.float64))
        if n is not None and rig.get("target_normals") is not None:
            n += w * np.asarray(rig["target_normals"][t], np.float64)
    if rig.get("joints") is not None:
        m = np.asarray(pose["matrices"], np.float64)
        joints, weights = np.asarray(rig["joints"]).astype(int), np.asarray(rig["weights"], np.float64)
        blended = np.einsum("vk,vkrc->vrc", weights, m[joints])      # (v, 3, 4)
        magnitude = np.einsum("vk,vkrc->vrc", weights, np.abs(m[joints]))
        bound = np.einsum("vrc,vc->vr", magnitude[:, :, :3], p_abs) + magnitude[:, :, 3]
        p = np.einsum("vrc,vc->vr", blended[:, :, :3], p) + blended[:, :, 3]
        if n is not None:
            n = np.einsum("vrc,vc->vr", blended[:, :, :3], n)
    else:
        bound = p_abs
    return p, n, bound


@pytest.mark.parametrize("name", vp.CASE_IDS)
def test_the_chain_lies_within_its_roundings_of_float64_skinning(name):
    scene, info, rigs, steps = vp.case(name)
    for poses in steps:
        for pose in poses:
            rig = rigs[pose["rig"]]
            rows = scene.posed_geometry(rig, pose)
            assert rows is not None
            positions, normals, bound = skinned64(rig, pose)
            targets = 0 if rig.get("target_positions") is None else len(rig["target_positions"])
            roundings = int(vp.library().vertex_pose_host_roundings(targets))
            assert roundings == 2 * targets + 4 * 7 + 3      # the header's count, repeated: two per target, seven per slot, three sums between four slots
            error = np.abs(rows["position"].astype(np.float64) - positions)
            print(name, "largest position error over its bound:", float((error / np.maximum(roundings * 2.0 ** -24 * bound, 1e-300)).max()))
            assert (error <= roundings * 2.0 ** -24 * bound).all()
            if normals is None:
                assert not rows["oct_normal"].any()
                continue
            live = np.einsum("vc,vc->v", normals, normals) > 0.0      # a collapsed normal takes the rest normal's code: checked with the exact cases
            rounded = (normals[live] / np.linalg.norm(normals[live], axis=1, keepdims=True)).astype(np.float32)
            yardstick = angles(decode64(project_encoder(rounded)), normals[live]).max()
            ours = angles(decode64(rows["oct_normal"][live]), normals[live]).max()
            print(name, "largest normal angle:", float(ours), "the project's encoder on the float64 normals:", float(yardstick))
            assert ours <= 2.0 * yardstick


def test_exact_cases():
    scene, info = vp.make_scene(tube=True)
    rig = vp.tube_rig(info, 0, 289, 2)
    rest = rig["rest_positions"]
    rest_codes = project_encoder(normalised32(rig["rest_normals"]))
    identity = np.stack([vp.IDENTITY, vp.IDENTITY])
    for weights in ((1.0, 0.0, 0.0, 0.0), (0.5, 0.5, 0.0, 0.0)):
        rows = scene.posed_geometry(dict(rig, weights=np.tile(np.array(weights, np.float32), (289, 1))), dict(matrices=identity))
        assert np.array_equal(rows["position"].view(np.uint32), rest.view(np.uint32)), weights
        assert np.array_equal(rows["oct_normal"], rest_codes)
    # identity matrices and zero target weights: the targets are skipped
    morphed = dict(rig, target_positions=np.full((2, 289, 3), 0.25, np.float32), target_normals=np.full((2, 289, 3), 0.5, np.float32), weights=np.tile(np.array([1.0, 0.0, 0.0, 0.0], np.float32), (289, 1)))
    rows = scene.posed_geometry(morphed, dict(matrices=identity, weights=[0.0, 0.0]))
    assert np.array_equal(rows["position"].view(np.uint32), rest.view(np.uint32)) and np.array_equal(rows["oct_normal"], rest_codes)
    # a zero matrix on every joint: all positions at +0, every normal the rest normal's code
    rows = scene.posed_geometry(rig, dict(matrices=np.stack([vp.ZERO, vp.ZERO])))
    assert not rows["position"].view(np.uint32).any() and np.array_equal(rows["oct_normal"], rest_codes)
    # a slot of weight 0 may name any joint
    pose = dict(matrices=np.concatenate([vp.bend(2), np.full((3, 3, 4), 1e9, np.float32)]))
    wide = dict(rig, joint_count=5)
    expected = scene.posed_geometry(wide, pose)
    for spare in (0, 1, 4):
        joints = rig["joints"].copy()
        joints[:, 2:] = spare
        assert np.array_equal(scene.posed_geometry(dict(wide, joints=joints), pose), expected), spare


def held_after_walk(scene, rigs, poses, budget=None):
    """The builder's arrays after the kernel's walk: the posed pool, then the vertex update's host passes over the posed ranges (the continuation the device shares)."""
    held = vu.arrays_of(scene)
    pool, marks, posed = vp.walk(held["geometry"], scene.pooled_rigs(rigs), poses, budget)
    assert posed == sum(len(rigs[p["rig"]]["rest_positions"]) for p in poses)
    expected_marks = np.zeros(len(pool), bool)
    edits = []
    for p in poses:
        r = scene.pooled_rigs([rigs[p["rig"]]])[0]
        expected_marks[r["first"]:r["first"] + len(r["rest_positions"])] = True
        edits.append(dict(first=r["first"], geometry=pool[r["first"]:r["first"] + len(r["rest_positions"])].copy()))
    assert np.array_equal(marks.astype(bool), expected_marks)
    assert np.array_equal(pool[~expected_marks], held["geometry"][~expected_marks])      # no byte outside the posed ranges
    answer = vu.run_kernel_bodies(scene, held, edits)
    return held, pool, answer


@pytest.mark.parametrize("name", vp.CASE_IDS)
def test_the_kernels_walk_leaves_what_the_builder_leaves(name):
    scene, info, rigs, steps = vp.case(name)
    staged, _, _, _ = vp.case(name)
    budget = vp.lds_joints()
    assert name != "joints_above_the_lds_budget" or rigs[0]["joint_count"] == budget + 1
    for poses in steps:
        moved = vp.moved_count(scene, rigs, poses)
        held, pool, answer = held_after_walk(scene, rigs, poses)
        gathered, _, _ = vp.walk(vu.pool(scene, "geometry"), scene.pooled_rigs(rigs), poses, 0)      # the other matrix path: the same bytes
        assert np.array_equal(pool, gathered)
        for p in poses:      # against posed_geometry
            r = scene.pooled_rigs([rigs[p["rig"]]])[0]
            assert np.array_equal(pool[r["first"]:r["first"] + len(r["rest_positions"])], scene.posed_geometry(rigs[p["rig"]], p))
        kept = scene.pose_rigs(poses, NEVER_REBUILD)
        assert kept is (name != "zero_matrix_collapses_a_limb") and answer["moved"] == moved and answer["needs_rebuild"] == (not kept)
        if kept:
            assert_held_equals(held, scene, "against SceneBuilder::pose_rigs")
        else:      # the collapsed limb's triangles fall onto each other: a leaf record cannot be refitted, the builder rebuilt -- the pools and the corners still agree
            assert np.array_equal(held["geometry"], vu.pool(scene, "geometry"))
            assert np.array_equal(held["triangles"][np.lexsort((held["triangles"][:, 10], held["triangles"][:, 9]))], by_instance_and_primitive(scene))
        # the staged path: another pose first, then this one, then the catch-up -- it must equal this pose alone
        other = [dict(p, **({"matrices": np.asarray(p["matrices"]) * np.float32(0.5)} if p.get("matrices") is not None else {}),
                      **({"weights": np.asarray(p["weights"], np.float32) + np.float32(0.125)} if p.get("weights") is not None else {})) for p in poses]
        assert [p["rig"] for p in staged.stage_rig_poses(other)] == [p["rig"] for p in poses]
        assert staged.stage_rig_poses(poses) is not None
        assert staged.apply_staged(NEVER_REBUILD) is kept
        if kept:
            assert_held_equals(held, staged, "against stage_rig_poses twice + apply_staged_transforms")
        else:
            assert np.array_equal(held["geometry"], vu.pool(staged, "geometry")) and np.array_equal(by_instance_and_primitive(scene), by_instance_and_primitive(staged))


def test_a_budget_below_the_rigs_joints_takes_the_gather_and_gives_the_same_bytes():
    scene, info, rigs, steps = vp.case("box_worn_by_two_and_a_mirrored_twin_all_four_slots")
    pools = [vp.walk(vu.pool(scene, "geometry"), scene.pooled_rigs(rigs), steps[0], budget)[0] for budget in (0, 3, 4, vp.lds_joints(), vp.lds_capacity())]
    assert all(np.array_equal(pools[0], other) for other in pools[1:])
    assert vp.walk(vu.pool(scene, "geometry"), scene.pooled_rigs(rigs), steps[0], vp.lds_capacity() + 1)[2] == -3


def edit_inside_the_tube_rig(scene, info):
    """A vertex edit (mesh-relative) of 50 vertices in the middle of tube_257's rig, made without reading the builder's pools."""
    data = info["data"]["lace"]
    rows = scene.vertex_geometry(data["positions"][100:150] + np.float32(0.05), data["normals"][100:150])
    return dict(mesh=info["mesh"]["lace"], first=100, geometry=rows)


def assert_builders_equal(a, b, what):
    held_a, held_b = vu.arrays_of(a), vu.arrays_of(b)
    for k in held_a:
        assert np.array_equal(held_a[k], held_b[k]), (what, k)


def test_a_later_write_wins_over_a_staged_pose():
    """A staged pose is skinned BEFORE any later writer of the same vertices writes, never replayed over it by the catch-up: the device applied the pose long ago."""
    pose_a, pose_b = [dict(rig=0, matrices=vp.bend(2, 1.1))], [dict(rig=0, matrices=vp.bend(2, -0.4, seed=3))]
    # (1) stage_rig_poses(A), then stage_vertex_edits(E) inside the rig's range, then the catch-up: E over A, as update_vertices(E) after pose_rigs(A) leaves it
    scene, info, rigs, _ = vp.case("tube_257")
    reference, reference_info, _, _ = vp.case("tube_257")
    edit = edit_inside_the_tube_rig(scene, info)
    assert scene.stage_rig_poses(pose_a) is not None and scene.stage_vertex_edits([edit]) is not None and scene.apply_staged(NEVER_REBUILD) is True
    assert reference.pose_rigs(pose_a, NEVER_REBUILD) is True and reference.update_vertices([edit_inside_the_tube_rig(reference, reference_info)], NEVER_REBUILD) is True
    assert_builders_equal(scene, reference, "stage_rig_poses, stage_vertex_edits, catch-up")
    assert np.array_equal(vu.of_mesh(scene, info["mesh"]["lace"], "geometry")[100:150], edit["geometry"])
    # ... and through the whole host path of the vertex edit
    scene, info, rigs, _ = vp.case("tube_257")
    assert scene.stage_rig_poses(pose_a) is not None and scene.update_vertices([edit_inside_the_tube_rig(scene, info)], NEVER_REBUILD) is True
    assert_builders_equal(scene, reference, "stage_rig_poses, update_vertices")
    assert scene.apply_staged(NEVER_REBUILD) is True
    assert_builders_equal(scene, reference, "... and nothing is left to replay")
    # (2) stage_rig_poses(A), then the host path pose_rigs(B) on the same rig: B
    scene, info, rigs, _ = vp.case("tube_257")
    reference, _, _, _ = vp.case("tube_257")
    assert scene.stage_rig_poses(pose_a) is not None and scene.pose_rigs(pose_b, NEVER_REBUILD) is True and scene.apply_staged(NEVER_REBUILD) is True
    assert reference.pose_rigs(pose_b, NEVER_REBUILD) is True
    assert_builders_equal(scene, reference, "stage_rig_poses(A), pose_rigs(B)")


def refused_rigs(info, vertex_count_of_mesh=289):
    """Rig lists hipr_set_scene_rigs and SceneBuilder::set_rigs refuse, mesh-relative over the lace, each with what is wrong with it."""
    good = lambda **changes: dict(vp.tube_rig(info, 0, 16, 2), **changes)
    with_targets = lambda **changes: dict(vp.flag_rig(info, 0, 16, 1, True), **changes)

    def edited(rig, name, index, value):
        rig = dict(rig)
        rig[name] = np.array(rig[name], copy=True)
        rig[name][index] = value
        return rig
    return {
        "no vertices": [good(count=0)],
        "begins past the mesh": [good(first=vertex_count_of_mesh)],
        "reaches past the mesh": [good(first=vertex_count_of_mesh - 15)],
        "first + count wraps around 32 bits": [good(first=0xFFFFFFF8)],
        "two rigs overlap": [good(), dict(vp.tube_rig(info, 15, 16, 2))],
        "neither joints nor targets": [dict(vp.of_mesh(info, "lace", 0, 16))],
        "null rest positions": [good(rest_positions="null", count=16)],
        "null joints": [good(joints="null")],
        "null weights": [good(weights="null")],
        "null target positions": [with_targets(target_positions="null", target_count=1)],
        "more than 256 targets": [with_targets(target_count=257)],
        "a joint index at the joint count": [edited(good(), "joints", (3, 3), 2)],
        "a weight above 1": [edited(good(), "weights", (5, 0), 1.5)],
        "a negative weight": [edited(good(), "weights", (5, 0), -0.25)],
        "a weight that is not finite": [edited(good(), "weights", (5, 1), np.nan)],
        "four weights of 0": [edited(edited(good(), "weights", (7, 0), 0.0), "weights", (7, 1), 0.0)],
        "a rest position that is not finite": [edited(good(), "rest_positions", (2, 1), np.inf)],
        "a rest position above 2^30": [edited(good(), "rest_positions", (2, 1), 2.0 ** 31)],
        "a delta that is not finite": [edited(with_targets(), "target_positions", (0, 2, 1), np.nan)],
        "a normal delta above 2^30": [edited(with_targets(), "target_normals", (0, 2, 1), -2.0 ** 31)],
        "a rest normal that is not finite": [edited(good(), "rest_normals", (2, 1), np.nan)],
        "a rest normal of length 0": [edited(edited(edited(good(), "rest_normals", (2, 0), 0.0), "rest_normals", (2, 1), 0.0), "rest_normals", (2, 2), 0.0)],
        "a rest normal whose squared length underflows": [edited(edited(edited(good(), "rest_normals", (2, 0), 1e-30), "rest_normals", (2, 1), 0.0), "rest_normals", (2, 2), 0.0)],
    }


def refused_poses():
    """Pose lists refused over the rigs [tube_rig(0, 16, 2 joints), flag_rig(100, 16, 2 targets)]."""
    matrices, weights = vp.bend(2), np.array([0.5, 0.25], np.float32)
    bad = lambda value: np.where(np.arange(24).reshape(2, 3, 4) == 13, np.float32(value), matrices).astype(np.float32)
    return {
        "a rig that is not bound": [dict(rig=2, matrices=matrices)],
        "the same rig twice": [dict(rig=0, matrices=matrices), dict(rig=1, weights=weights), dict(rig=0, matrices=matrices)],
        "null matrices": [dict(rig=0)],
        "null target weights": [dict(rig=1)],
        "a matrix entry that is not finite": [dict(rig=0, matrices=bad(np.nan))],
        "a matrix entry above 2^30": [dict(rig=1, weights=weights), dict(rig=0, matrices=bad(-2.0 ** 31))],
        "a target weight that is not finite": [dict(rig=1, weights=[0.5, np.inf])],
        "a target weight above 2^10": [dict(rig=1, weights=[1025.0, 0.0])],
    }


def test_the_builder_refuses_what_the_device_refuses():
    scene, info = vp.make_scene(tube=True)
    before = vu.arrays_of(scene)
    for what, rigs in refused_rigs(info).items():
        assert scene.set_rigs(rigs) is False, what
        assert scene.pose_rigs([dict(rig=0, matrices=vp.bend(2))]) is None, what      # nothing was bound
    # the builder's own: a mesh it does not hold, normals that do not match the mesh's flags
    assert scene.set_rigs([dict(vp.tube_rig(info, 0, 16, 2), mesh=99)]) is False
    assert scene.set_rigs([{k: v for k, v in vp.tube_rig(info, 0, 16, 2).items() if k != "rest_normals"}]) is False
    rigs = [vp.tube_rig(info, 0, 16, 2), vp.flag_rig(info, 100, 16, 2)]
    assert scene.set_rigs(rigs) is True
    for what, poses in refused_poses().items():
        assert scene.pose_rigs(poses) is None, what
        assert scene.stage_rig_poses(poses) is None, what
        assert scene.apply_staged(NEVER_REBUILD) is True      # nothing was staged
    after = vu.arrays_of(scene)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    # an empty list of poses is served and changes nothing; an empty rig list removes the rigs
    assert scene.pose_rigs([]) is True and scene.set_rigs([]) is True and scene.pose_rigs([dict(rig=0, matrices=vp.bend(2))]) is None
    after = vu.arrays_of(scene)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    # a mesh added since the last build is not the device's yet; before the scene is built nothing is bound
    added = scene.add_mesh(**vu.mesh_data()["box"])
    assert scene.set_rigs([dict(vp.box_rig(info), mesh=added)]) is False
