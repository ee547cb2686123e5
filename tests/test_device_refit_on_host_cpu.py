"""The device refit of the 8-wide tree (csrc/wide8_refit.h, hipr_refit_scene_transforms) held to the host's refit WITHOUT a GPU: its record, box, grid and
quantisation routines are __host__ __device__ functions, compiled for the host by tests/native/DeviceRefitHost.hip, and must leave the bytes
SceneBuilder::update_model_transforms + refit_wide8 leave."""
import numpy as np
import pytest

import device_refit_bindings as refit
from bifrost3d_amd.host import Scene

POSE = dict(translation=(0.05, -0.30, 0.10), rotation=(0.0, float(np.sin(0.4)), 0.0, float(np.cos(0.4))), scale=0.3)      # test_refitted_scene_on_the_device_bit_exact's


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name, param0, param1, model", [("cornell", 1, 0, 6), ("cornell", 3, 0, 6), ("cornell", 12, 0, 6), ("atrium", 20000, 3, 10)])
def test_refit_routines_leave_the_bytes_of_the_host_refit(name, param0, param1, model):
    """After a move every triangle, every leaf record and every node slot is byte-identical to the host's, and so is the grid; the area is the f64 sum of the
    f32 half areas of the exact child boxes."""
    scene = Scene(name, param0=param0, param1=param1)
    before = scene.wide8_slots()
    moved = scene.model_pose(model, **POSE)
    assert len(moved) == 1
    ours = refit.refit_scene(scene, moved)
    assert np.array_equal(scene.wide8_slots(), before)                      # model_pose and the routines work on copies
    assert scene.move_model(model, rebuild_threshold=1e30, **POSE) is True      # the host's refit of the same pose, topology kept
    desc = scene.desc
    assert not ours["needs_rebuild"]
    assert np.array_equal(ours["triangles"], scene.triangles())
    theirs = scene.wide8_slots()
    assert not np.array_equal(theirs, before)                               # the move did change the tree
    different = np.nonzero((ours["slots"] != theirs).any(axis=1))[0]
    assert len(different) == 0, (len(different), different[:8], ours["slots"][different[:2]], theirs[different[:2]])
    assert np.array_equal(bits(ours["grid_min"]), bits(desc.wide8_grid_min[:])) and np.array_equal(bits(ours["grid_cell"]), bits(desc.wide8_grid_cell[:]))
    expected_area = refit.half_area_sum(refit.exact_boxes(theirs, scene.triangles()))
    assert abs(ours["area"] - expected_area) <= 1e-11 * expected_area
    # there and back: the refit is a function of the pose alone
    untouched = Scene(name, param0=param0, param1=param1)
    original = [(moved[0][0], np.array(untouched.desc.instances[moved[0][0]].object_to_world[:], np.float32))]
    back = refit.refit_scene(scene, original)      # `scene` is in the moved pose now; the original pose of the model is what an untouched scene holds
    assert np.array_equal(back["slots"], before) and np.array_equal(back["triangles"], untouched.triangles())


def test_a_parting_pair_of_the_atrium_is_reported_where_the_host_rebuilds():
    """Model 6 of the small atrium holds two object-space vertices that share a world position in the built pose and part under POSE: the host's refit_wide8 gives
    up and the scene builder rebuilds (move_model is False); the device's routines report needs_rebuild for the same move."""
    scene = Scene("atrium", param0=20000, param1=3)
    ours = refit.refit_scene(scene, scene.model_pose(6, **POSE))
    assert ours["needs_rebuild"]
    assert scene.move_model(6, rebuild_threshold=1e30, **POSE) is False


def test_a_constructed_pair_parts_on_the_host_and_in_the_device_routines(tmp_path):
    """Two object-space vertices one ulp apart that share a world position at scale 0.3 and part at scale 1 (device_refit_bindings.write_parting_pair_obj): the
    builder pairs their triangles in the small pose; for the move to scale 1 the host rebuilds -- the reference behaviour -- and the device's routines report it."""
    scene = refit.scene_with_a_parting_pair(tmp_path / "pair.obj")
    ours = refit.refit_scene(scene, scene.model_pose(1, **refit.LARGE_POSE))
    assert ours["needs_rebuild"]
    assert scene.move_model(1, rebuild_threshold=1e30, **refit.LARGE_POSE) is False


def synthetic_nodes(rng, count):
    """Random nodes and the corners the exponent search and the origin snap can stumble over."""
    boxes = np.zeros((count, 8, 6), np.float32)
    valid = np.zeros(count, np.uint32)
    grids = np.zeros((count, 6), np.float32)
    kind = rng.integers(0, 5, count)
    for i in range(count):
        children = int(rng.integers(1, 9))
        positions = rng.permutation(8)[:children]
        valid[i] = sum(1 << int(p) for p in positions)
        scale = np.float32(2.0 ** rng.integers(-20, 12))
        grid_min = (rng.uniform(-4, 4, 3) * scale).astype(np.float32)
        scene_extent = (rng.uniform(1, 64, 3) * scale).astype(np.float32)
        grid_cell = np.maximum(scene_extent / np.float32(2097151.0), np.float32(1e-30)).astype(np.float32)
        if kind[i] == 0:        # anywhere in the scene
            lo = grid_min + rng.uniform(0, 1, (children, 3)).astype(np.float32) * scene_extent
            size = rng.uniform(0, 1, (children, 3)).astype(np.float32) ** 4 * scene_extent * np.float32(rng.uniform(0.001, 1))
            hi = (lo + size).astype(np.float32)
        elif kind[i] == 1:      # extents of exactly 255 * 2^n from the node's origin (= grid_min: m = 0), and one ulp either way
            n = int(rng.integers(-24, 10))
            unit = np.float32(2.0 ** n)
            grid_min = (rng.integers(-64, 64, 3) * unit).astype(np.float32)
            reach = (grid_min + np.float32(255.0) * unit).astype(np.float32)
            step = int(rng.integers(-1, 2))
            if step:
                reach = np.nextafter(reach, np.float32(np.inf if step > 0 else -np.inf)).astype(np.float32)
            lo = np.tile(grid_min, (children, 1)) + (rng.integers(0, 200, (children, 3)) * unit).astype(np.float32)
            hi = np.minimum(lo + (rng.integers(0, 56, (children, 3)) * unit).astype(np.float32), reach).astype(np.float32)
            lo[0] = grid_min
            hi[0] = reach
            if rng.integers(0, 2):      # bounds off the 2^n lattice as well
                lo[1:] = np.nextafter(lo[1:], np.float32(np.inf))
                hi[1:] = np.minimum(np.nextafter(hi[1:], np.float32(-np.inf)), reach)
                lo[1:] = np.minimum(lo[1:], hi[1:])
        elif kind[i] == 2:      # zero extents: a flat or point-like node
            lo = grid_min + rng.uniform(0, 1, (children, 3)).astype(np.float32) * scene_extent
            hi = lo.copy()
            flat = rng.integers(0, 2, 3).astype(bool)
            lo[:, flat] = lo[0, flat]
            hi[:, flat] = lo[0, flat]
            hi[:, ~flat] += (rng.uniform(0, 0.1, (children, int((~flat).sum()))) * scene_extent[~flat]).astype(np.float32)
        else:                   # at and beyond the ends of the grid: the origin clamps to cell 0 or 2097151
            end = (grid_min + np.float32(2097151.0) * grid_cell).astype(np.float32)
            anchor = grid_min if kind[i] == 3 else end
            lo = anchor + (rng.uniform(-3, 3, (children, 3)) * grid_cell * np.float32(rng.choice([1.0, 1000.0]))).astype(np.float32)
            hi = (lo + rng.uniform(0, 1, (children, 3)).astype(np.float32) * scene_extent * np.float32(0.01)).astype(np.float32)
        lo, hi = lo.astype(np.float32), np.maximum(hi, lo).astype(np.float32)
        boxes[i, positions, :3], boxes[i, positions, 3:] = lo, hi
        grids[i, :3], grids[i, 3:] = grid_min, grid_cell
    return boxes, valid, grids


def test_quantisation_sweep_equals_the_hosts_quantise_node():
    """120 000 synthetic nodes -- random ones, extents that are exact powers of two times 255 and their neighbours one ulp either way, zero extents, boxes at the
    grid's ends -- give the node bytes of the host's quantise_node: the exponent search seeded from the extent's bits finds the exponent the host's log2 seed finds."""
    boxes, valid, grids = synthetic_nodes(np.random.default_rng(20), 120000)
    ours = refit.quantise_nodes(boxes, valid, grids, device=True)
    theirs = refit.quantise_nodes(boxes, valid, grids, device=False)
    assert theirs.any(axis=1).all()
    different = np.nonzero((ours != theirs).any(axis=1))[0]
    assert len(different) == 0, (len(different), different[:4], boxes[different[:1]], grids[different[:1]], ours[different[:1]], theirs[different[:1]])
    exponents = theirs[:, 2] & 0xFF
    assert len(np.unique(exponents)) > 20      # the sweep does reach many exponents


def test_a_pair_that_parts_is_reported_not_written():
    """A record whose second triangle no longer shares two bit-identical corners with the first is reported and left as stored."""
    p = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.25], [1.0, 1.0, 0.5], [0.0, 1.0, 0.125]], np.float32)
    triangles = np.zeros((2, 12), np.uint32)
    triangles[0, :9] = bits(p[[0, 1, 2]].reshape(-1))      # A = (a, b, c)
    triangles[1, :9] = bits(p[[2, 3, 0]].reshape(-1))      # B = (c, d, a): shares a and c
    triangles[:, 11] = 1 | 4
    stored = np.zeros(16, np.uint32)
    stored[12], stored[13] = 0, 1
    stored[14] = 1 << 8                                    # A is stored unrotated: its u is weight 1
    ok, record, box = refit.refit_leaf(triangles, stored)
    assert ok and record[13] == 1 and np.array_equal(record[:3], bits(p[0]))
    assert np.array_equal(record[9:12].view(np.float32), p[3] - p[0])      # e3 = d - a
    assert np.array_equal(box, np.concatenate([p.min(axis=0), p.max(axis=0)]))
    ok_again, same, _ = refit.refit_leaf(triangles, record)
    assert ok_again and np.array_equal(same, record)
    parted = triangles.copy()
    parted[1, 0:3] = bits(np.nextafter(p[2], np.float32(2.0)))      # B's copy of c moves by one ulp
    ok, untouched, _ = refit.refit_leaf(parted, record)
    assert not ok and np.array_equal(untouched, record)
