"""The device build of the BVH2 (csrc/bvh2_build.h, hipr_build_bvh2) held to the host builder WITHOUT a GPU: its routines are __host__ __device__ functions,
compiled for the host and walked level by level in the kernels' shape by tests/native/DeviceBuildHost.hip, and must leave the nodes (64 B each), the triangle order
and the depth of hiprh_bvh_build, byte for byte."""
import numpy as np
import pytest

import device_build_bindings as build
from bifrost3d_amd.host import Scene


def check(triangles, max_depth=62):
    ours = build.routines_build(triangles, max_depth)
    theirs = build.host_build(triangles, max_depth)
    assert ours["status"] == 0, ours["decline"]
    build.same_tree(ours, theirs)
    return ours, theirs


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8])
def test_single_leaf_and_first_split_sizes(n):
    ours, _ = check(build.random_triangles(n, seed=n))
    if n <= 3:
        assert len(ours["nodes"]) == 1 and ours["nodes"][0, 12] == ours["nodes"][0, 13] and ours["deepest"] == 1      # both children reference the leaf


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_a_thousand_random_triangles(seed):
    check(build.random_triangles(1000, seed))


def test_a_strip_along_one_axis():
    check(build.strip(257))


@pytest.mark.parametrize("negative_first", [False, True])
def test_signed_zeros_meeting_at_the_bounds(negative_first):
    triangles = build.signed_zeros(negative_first)
    ours, theirs = check(triangles)
    boxes = theirs["nodes"][:, :12]
    assert (boxes == 0x80000000).any() and (boxes == 0).any()      # both zeros do reach stored child boxes
    other, _ = check(build.signed_zeros(not negative_first))
    assert not np.array_equal(other["nodes"], ours["nodes"])        # ... and the order of appearance decides which


def test_a_cluster_of_identical_triangles_takes_a_short_median_range():
    triangles = build.with_cluster()
    _, theirs = check(triangles)
    assert theirs["median_splits"] >= 1 and 4 <= theirs["longest_median_range"] <= build.median_lane_limit()


def test_identical_triangles_decline():
    triangles = build.identical(300)
    ours = build.routines_build(triangles)
    assert ours["status"] == 1 and ours["decline"] == (0, 300)
    assert (ours["nodes"] == build.PATTERN).all() and (ours["order"] == build.PATTERN).all()
    assert build.host_build(triangles)["longest_median_range"] == 300


def test_a_depth_budget_that_forces_the_root_to_the_median_declines():
    triangles = build.random_triangles(4096, 11)
    ours = build.routines_build(triangles, max_depth=8)
    assert ours["status"] == 1 and ours["decline"] == (0, 4096)
    assert (ours["nodes"] == build.PATTERN).all() and (ours["order"] == build.PATTERN).all()
    assert build.host_build(triangles, 8)["longest_median_range"] == 4096


def test_a_depth_budget_met_by_short_ranges_only():
    """max_depth = 8 over 64 crowded triangles: the budget forces medians further down, where the ranges are short enough for a lane."""
    ours, theirs = check(build.skewed(64), max_depth=8)
    assert theirs["median_splits"] >= 2 and theirs["deepest"] == 8


def test_the_atrium_at_20k():
    check(Scene("atrium", param0=20000).triangles())


def test_300_000_random_triangles_against_the_hosts_threaded_path():
    check(build.random_triangles(300000, 21, size=0.004))      # above 2 * PARALLEL_RANGE: the host bins, partitions and builds subtrees on several threads


# param0 of the atrium is a triangle BUDGET: 260 000 with seed 1 is the project's 251 424-triangle atrium of the headline benchmark
@pytest.mark.parametrize("make, triangles", [(lambda: Scene("atrium", param0=20000), None), (lambda: Scene("atrium", param0=260000, param1=1), 251424), (lambda: Scene("material"), None),
                                             (lambda: Scene("glass"), None)], ids=["atrium_20k", "atrium_251k", "material", "glass"])
def test_no_scene_takes_a_median_range_longer_than_a_lane_sorts(make, triangles):
    """The condition that keeps the GPU tests from passing by declining: the host's own count of its median splits, per scene."""
    scene = make()
    if triangles is not None:
        assert scene.desc.triangle_count == triangles
    counts = scene.build_counts()
    assert counts["longest_median_range"] <= build.median_lane_limit(), counts


def test_the_routines_build_the_251k_atrium():
    """... and the routines do build the headline scene's triangles, not decline them."""
    scene = Scene("atrium", param0=260000, param1=1)
    assert scene.desc.triangle_count == 251424
    check(scene.triangles())
