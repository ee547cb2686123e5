"""The device's collapse of the BVH2 to the 8-wide tree (csrc/wide8_build.h, hipr_build_wide8) held to the host's build_wide8 WITHOUT a GPU: its routines are
__host__ __device__ functions, compiled for the host and walked in the kernels' shape (level lists and scans included) by tests/native/DeviceCollapseHost.hip, and
must leave the slots (64 B each), the height, the grid and the counters of build_wide8 (hiprh_bvh_wide8_*), byte for byte."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import device_collapse_bindings as collapse
from bifrost3d_amd.host import Scene

REPO = Path(__file__).resolve().parent.parent


def check(host):
    ours = collapse.routines_collapse(host["nodes"], host["triangles"], host["order"])
    assert ours["status"] == collapse.OK, ours.get("message")
    collapse.same_wide8(ours["wide8"], host["wide8"])
    return ours["wide8"]


@pytest.mark.parametrize("name", list(collapse.SETS))
def test_the_routines_collapse_to_the_hosts_tree(name):
    host = collapse.reference(name)
    ours = check(host)
    nodes, leaves, paired = ours["counts"]
    assert nodes + leaves == len(ours["slots"]) and nodes >= 1
    if name == "quad":
        assert (nodes, leaves, paired) == (1, 1, 1) and ours["height"] == 1        # the root holds a single record
    if name == "n1":
        assert host["nodes"][0, 12] == host["nodes"][0, 13] and (nodes, leaves, paired) == (1, 1, 0)      # the single-leaf root references its leaf twice
    if name == "grid16":
        assert paired > leaves // 2        # most records hold two triangles
    if name == "grid_two_instances":
        records = ours["slots"][_leaf_slots(ours["slots"])]
        both = records[records[:, 13] != 0xFFFFFFFF]
        instance = host["triangles"][host["order"]][:, 9]
        assert (instance[both[:, 12]] == instance[both[:, 13]]).all()        # no pairing across instances, though every triangle lies on its twin of the other one
        assert paired < collapse.reference("grid16")["wide8"]["counts"][2]
    if name == "grid_mixed_flags":
        flags = ours["slots"][_leaf_slots(ours["slots"])][:, 14] & 0xF
        assert all((flags & bit).any() for bit in (1, 2, 4, 8))
    if name == "n300000":
        assert len(host["triangles"]) >= 1 << 16        # the host's threaded path


def _leaf_slots(slots):
    """The slots that are leaf records: every slot no node's inner mask names, the root aside."""
    is_node = np.zeros(len(slots), bool)
    is_node[0] = True
    for i in range(len(slots)):      # children live in higher slots
        if not is_node[i]:
            continue
        base, valid, inner = int(slots[i, 3]) & 0xFFFFFF, int(slots[i, 3]) >> 24, (int(slots[i, 2]) >> 24) & 0xFF
        rank = 0
        for s in range(8):
            if valid >> s & 1:
                if inner >> s & 1:
                    is_node[base + rank] = True
                rank += 1
    return ~is_node


def test_the_signed_zero_sets_differ_in_their_trees():
    a, b = collapse.reference("zeros_negative_first")["wide8"], collapse.reference("zeros_positive_first")["wide8"]
    assert not np.array_equal(a["grid"], b["grid"]) or not np.array_equal(a["slots"], b["slots"])


@pytest.mark.parametrize("make", [lambda: Scene("atrium", param0=60000), lambda: Scene("material"), lambda: Scene("glass")], ids=["atrium_60k", "material", "glass"])
def test_the_routines_collapse_the_scenes(make):
    ours = check(collapse.host_collapse(make().triangles()))
    assert ours["counts"][2] > 0      # the scenes' meshes share edges


def test_the_hosts_tree_does_not_depend_on_its_thread_count():
    """The yardstick itself: HIPR_BVH_THREADS=1 and =16 give the host the same slots (a fresh process each: the builder reads the variable once)."""
    script = ("import sys, hashlib; sys.path.insert(0, sys.argv[1]); import device_collapse_bindings as c; w = c.host_collapse(c.SETS['n300000']())['wide8'];"
              "print(hashlib.sha256(w['slots'].tobytes() + w['grid'].tobytes()).hexdigest(), w['height'], w['counts'])")
    seen = []
    for threads in ("1", "16"):
        env = dict(os.environ, HIPR_BVH_THREADS=threads, PYTHONPATH=os.pathsep.join([str(REPO), os.environ.get("PYTHONPATH", "")]))
        seen.append(subprocess.run([sys.executable, "-c", script, str(REPO / "tests")], env=env, capture_output=True, text=True, check=True, cwd=REPO).stdout.strip())
    assert seen[0] == seen[1] and seen[0]


# ---- refusals: nothing is written ----
def untouched(answer):
    return (answer["slots"] == collapse.PATTERN).all() and (answer["result"] == collapse.PATTERN).all()


def test_a_slot_capacity_below_the_slots_needed_is_refused():
    host = collapse.reference("grid16")
    answer = collapse.routines_collapse(host["nodes"], host["triangles"], host["order"], slot_capacity=len(host["wide8"]["slots"]) - 1)
    assert answer["status"] == collapse.INVALID and untouched(answer), answer["message"]
    exact = collapse.routines_collapse(host["nodes"], host["triangles"], host["order"], slot_capacity=len(host["wide8"]["slots"]))
    assert exact["status"] == collapse.OK


@pytest.mark.parametrize("what", ["child_past_the_nodes", "leaf_past_the_triangles", "node_referenced_twice", "order_past_the_triangles", "empty"])
def test_malformed_input_is_refused(what):
    host = collapse.reference("n17")
    nodes, triangles, order = host["nodes"].copy(), host["triangles"], host["order"].copy()
    inner = next(i for i in range(len(nodes)) if np.int32(nodes[i, 12]) >= 0 or np.int32(nodes[i, 13]) >= 0)
    if what == "child_past_the_nodes":
        nodes[inner, 12 if np.int32(nodes[inner, 12]) >= 0 else 13] = len(nodes)
    elif what == "leaf_past_the_triangles":
        leaf = next((i, c) for i in range(len(nodes)) for c in (12, 13) if np.int32(nodes[i, c]) < 0)
        nodes[leaf] = np.uint32(~np.uint32(((len(triangles) - 1) << 3) | 2))      # three triangles from the last one on
    elif what == "node_referenced_twice":
        nodes[len(nodes) - 1, 12] = 0      # a cycle through the root
    elif what == "order_past_the_triangles":
        order[3] = len(triangles)
    elif what == "empty":
        nodes = nodes[:0]
    answer = collapse.routines_collapse(nodes if len(nodes) else np.zeros((0, 16), np.uint32), triangles, order)
    assert answer["status"] == collapse.INVALID and untouched(answer), answer


@pytest.mark.parametrize("where", ["corner", "child_box"])
def test_a_value_that_is_not_finite_is_refused(where):
    """An infinite bound would keep the quantisation's rounding loops going for ever."""
    host = collapse.reference("n17")
    nodes, triangles = host["nodes"].copy(), host["triangles"].copy()
    infinity = np.array([np.inf], np.float32).view(np.uint32)[0]
    if where == "corner":
        triangles[5, 4] = infinity
    else:
        nodes[1, 1] = infinity
    answer = collapse.routines_collapse(nodes, triangles, host["order"])
    assert answer["status"] == collapse.INVALID and untouched(answer) and "finite" in answer["message"]


def test_more_levels_than_a_walk_of_64_entries_allows_is_refused():
    """A chain of 65 inner nodes, each with a one-triangle leaf on the left: 65 levels."""
    levels = collapse.library().collapse_host_max_levels() + 1
    triangles = collapse.random_triangles(levels + 1, 5)
    nodes = np.zeros((levels, 16), np.uint32)
    for i in range(levels):
        nodes[i, 12] = np.uint32(~np.uint32(i << 3))
        nodes[i, 13] = i + 1 if i + 1 < levels else np.uint32(~np.uint32(levels << 3))
    answer = collapse.routines_collapse(nodes, triangles, None)
    assert answer["status"] == collapse.INVALID and untouched(answer) and "level" in answer["message"]
    shorter = collapse.routines_collapse(nodes[:levels - 1].copy(), triangles[:levels], None)      # its last node's right child is inner node 64: cut it to a leaf
    assert shorter["status"] == collapse.INVALID      # ... which is now a child index past the nodes
    nodes[levels - 2, 13] = np.uint32(~np.uint32((levels - 1) << 3))
    assert collapse.routines_collapse(nodes[:levels - 1].copy(), triangles[:levels], None)["status"] == collapse.OK      # 64 levels collapse


def test_leaves_out_of_triangle_order_decline():
    """Record numbers are scanned in the order of the leaves' first triangles; the walk asserts that this is the depth-first order and declines a tree where it is not."""
    host = collapse.reference("n17")
    nodes = host["nodes"].copy()
    nodes[0, [12, 13]] = nodes[0, [13, 12]]      # the root's children swapped (the boxes go unread by this check)
    answer = collapse.routines_collapse(nodes, host["triangles"], host["order"])
    assert answer["status"] == collapse.DECLINED and untouched(answer)


def test_the_walk_under_the_sanitizers():
    """`make sanitize-device-collapse`: the stand-alone program (tests/native/DeviceCollapseSanitize.cpp) walks grid16, fan and n4097 under ASan + UBSan on the CPU."""
    done = subprocess.run(["make", "-C", str(REPO / "bifrost3d_amd"), "sanitize-device-collapse"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "3 sets walked" in done.stdout
