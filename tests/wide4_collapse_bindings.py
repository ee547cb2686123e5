"""ctypes handle on tests/native/libwide4_collapse_host.so -- the routines of the device's 4-wide collapse (csrc/wide4_build.h) compiled for the host
(tests/native/Wide4CollapseHost.hip) -- the host's collapse behind hiprh_bvh_build / hiprh_wide4_collapse, and the BVH2s both suites collapse: the triangle sets of
device_collapse_bindings and synthetic node arrays that reach branches the sets do not. Test infrastructure: the library is built by bifrost3d_amd/Makefile and
loaded by tests only."""
import ctypes as C
import functools
from pathlib import Path

import numpy as np

from bifrost3d_amd import capi
from bifrost3d_amd.host import load_host_library
from device_build_bindings import PATTERN, random_triangles
from device_collapse_bindings import SETS

LIB_PATH = Path(__file__).resolve().parent / "native" / "libwide4_collapse_host.so"
_up, _vp = C.POINTER(C.c_uint32), C.c_void_p
_lib = None
OK, INVALID = 0, 1      # collapse_host_wide4's answers
EMPTY = 0x7FFFFFFF      # HIPR_WIDE_EMPTY
SMALL_BUDGET, LARGE_BUDGET = 32, 0xFFFF


def library():
    global _lib
    if _lib is None:
        assert LIB_PATH.exists(), f"{LIB_PATH} is missing: run __graft_entry__.build()"
        lib = C.CDLL(str(LIB_PATH))
        lib.collapse_host_wide4.argtypes = [_vp, C.c_uint32, C.c_uint32, _vp, C.c_uint32, _vp, _vp, C.c_char_p, C.c_uint32]
        lib.collapse_host_wide4_quantise.argtypes = [_vp, _vp, C.c_uint32, _vp]
        lib.collapse_host_wide4_quantise.restype = None
        _lib = lib
    return _lib


def _wide_of_handle(lib, handle) -> dict:
    count = lib.hiprh_bvh_wide_node_count(handle)
    wide = np.ctypeslib.as_array(C.cast(lib.hiprh_bvh_wide_nodes(handle), _up), shape=(count, 16)).copy()
    return dict(wide_nodes=wide, stack_entries=int(lib.hiprh_bvh_wide_stack_entries(handle)))


def host_trees(triangles, max_depth=62) -> dict:
    """The host's trees over `triangles` (hiprh_bvh_build): `triangles`, the BVH2 `nodes` (count, 16) and `order` as uint32 words, and the 4-wide tree: `wide_nodes`
    (count, 16) and `stack_entries`."""
    lib = load_host_library()
    triangles = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 12)
    handle = lib.hiprh_bvh_build(C.cast(triangles.ctypes.data, C.POINTER(capi.HiprTriangle)), len(triangles), max_depth)
    assert handle
    try:
        count = lib.hiprh_bvh_node_count(handle)
        nodes = np.ctypeslib.as_array(C.cast(lib.hiprh_bvh_nodes(handle), _up), shape=(count, 16)).copy()
        order = np.ctypeslib.as_array(C.cast(lib.hiprh_bvh_order(handle), _up), shape=(len(triangles),)).copy()
        return dict(triangles=triangles, nodes=nodes, order=order, **_wide_of_handle(lib, handle))
    finally:
        lib.hiprh_bvh_destroy(handle)


@functools.lru_cache(maxsize=None)
def reference(name) -> dict:
    """host_trees of a set of device_collapse_bindings.SETS, computed once per process and shared; callers leave it unchanged."""
    return host_trees(SETS[name]())


def threaded_set():
    """330 000 random triangles: more than 2^17 BVH2 nodes, from which the host's collapse runs its subtrees on threads."""
    return random_triangles(330000, 22, 0.004)


def host_collapse(nodes, threads=1) -> dict:
    """hiprh_wide4_collapse: the host's WideCollapse alone over a BVH2 (node 0 the root, parents before children): `wide_nodes`, `stack_entries`, and its counters:
    `did_not_fit` (nodes that stopped adopting because one more child did not fit the budget) and the root's `budget`."""
    lib = load_host_library()
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 16)
    counters = (C.c_uint * 2)()
    handle = lib.hiprh_wide4_collapse(nodes.ctypes.data, len(nodes), threads, counters)
    assert handle
    try:
        return dict(did_not_fit=int(counters[0]), budget=int(counters[1]), **_wide_of_handle(lib, handle))
    finally:
        lib.hiprh_bvh_destroy(handle)


def host_collapse_on_device(ctx, nodes, triangle_count):
    """hiprh_wide4_build_on_device: (status, dict of wide_nodes and stack_entries, or None)."""
    lib = load_host_library()
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 16)
    status = C.c_int(0)
    handle = lib.hiprh_wide4_build_on_device(ctx.handle, nodes.ctypes.data, len(nodes), triangle_count, C.byref(status))
    if not handle:
        return status.value, None
    try:
        return status.value, _wide_of_handle(lib, handle)
    finally:
        lib.hiprh_bvh_destroy(handle)


def routines_collapse(nodes, triangle_count, node_capacity=None) -> dict:
    """The device collapse's routines on the host (collapse_host_wide4). status OK: `wide_nodes`, `stack_entries` and the walk's counters `did_not_fit`, `budget`,
    `levels`, `need`; INVALID: `wide_nodes` and `result` still hold PATTERN."""
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 16)
    capacity = len(nodes) if node_capacity is None else node_capacity
    wide = np.full((max(capacity, 1), 16), PATTERN, np.uint32)
    raw = np.full(2, PATTERN, np.uint32)
    counters = np.zeros(4, np.uint32)
    message = C.create_string_buffer(256)
    status = library().collapse_host_wide4(nodes.ctypes.data, len(nodes), triangle_count, wide.ctypes.data, capacity, raw.ctypes.data, counters.ctypes.data, message, 256)
    assert status >= 0, "collapse_host_wide4: a collapse off its bounds"
    if status != OK:
        return dict(status=status, wide_nodes=wide, result=raw, message=message.value.decode())
    return dict(status=OK, wide_nodes=wide[:int(raw[0])].copy(), stack_entries=int(raw[1]), did_not_fit=int(counters[0]), budget=int(counters[1]), levels=int(counters[2]), need=int(counters[3]))


def same_wide4(ours, theirs):
    """Byte equality of the nodes (64 B each), with the first differing node named, then the stack entries."""
    assert ours["wide_nodes"].shape == theirs["wide_nodes"].shape, (ours["wide_nodes"].shape, theirs["wide_nodes"].shape)
    different = np.nonzero((ours["wide_nodes"] != theirs["wide_nodes"]).any(axis=1))[0]
    assert len(different) == 0, f"{len(different)} nodes differ, the first is node {different[0]}: {ours['wide_nodes'][different[0]]} against {theirs['wide_nodes'][different[0]]}"
    assert ours["stack_entries"] == theirs["stack_entries"], (ours["stack_entries"], theirs["stack_entries"])
    return True


def quantise_on_host(boxes, counts) -> np.ndarray:
    """quantise_children of host/BvhBuilder.cpp over groups of child boxes: boxes (g, 4, 6) f32 (lo xyz, hi xyz), counts (g,) in 1 .. 4 -> (g, 16) uint32 node words."""
    boxes, counts = np.ascontiguousarray(boxes, np.float32), np.ascontiguousarray(counts, np.uint32)
    out = np.full((len(counts), 16), PATTERN, np.uint32)
    load_host_library().hiprh_wide4_quantise_children(boxes.ctypes.data, counts.ctypes.data, len(counts), out.ctypes.data)
    return out


def quantise_by_the_routines(boxes, counts) -> np.ndarray:
    """w4_quantise of csrc/wide4_build.h over the same groups."""
    boxes, counts = np.ascontiguousarray(boxes, np.float32), np.ascontiguousarray(counts, np.uint32)
    out = np.full((len(counts), 16), PATTERN, np.uint32)
    library().collapse_host_wide4_quantise(boxes.ctypes.data, counts.ctypes.data, len(counts), out.ctypes.data)
    return out


# ---- synthetic BVH2 node arrays: the collapse reads nothing but nodes ----
def leaf(lo, hi):
    """A leaf of one triangle with the box [lo, hi]."""
    return ("leaf", np.array(lo, np.float32), np.array(hi, np.float32))


def inner(left, right):
    return ("inner", left, right)


def _box_of(tree):
    if tree[0] == "leaf":
        return tree[1], tree[2]
    (alo, ahi), (blo, bhi) = _box_of(tree[1]), _box_of(tree[2])
    return np.minimum(alo, blo), np.maximum(ahi, bhi)


def nodes_of(tree):
    """(nodes (n, 16) uint32, triangle count) of a nested inner() / leaf() description: node 0 the root, parents before children in depth-first order as the host
    builder stores them, leaves of one triangle each numbered in the order they are met, every child box the exact union of what lies below it."""
    assert tree[0] == "inner"
    nodes, triangles = [], [0]

    def place(t):
        index = len(nodes)
        nodes.append(np.zeros(16, np.uint32))
        words = np.zeros(16, np.uint32)
        boxes = np.zeros(12, np.float32)
        for c in (0, 1):
            child = t[1 + c]
            lo, hi = _box_of(child)
            boxes[4 * c:4 * c + 4] = (lo[0], hi[0], lo[1], hi[1])
            boxes[8 + 2 * c:10 + 2 * c] = (lo[2], hi[2])
            if child[0] == "leaf":
                words[12 + c] = np.uint32(~np.uint32(triangles[0] << 3))
                triangles[0] += 1
            else:
                words[12 + c] = place(child)
        words[:12] = boxes.view(np.uint32)
        nodes[index] = words
        return index

    place(tree)
    return np.stack(nodes), triangles[0]


def _cube(corner, size=1.0):
    corner = np.array(corner, np.float32)
    return leaf(corner, corner + np.float32(size))


def budget_binds(depth=30):
    """(a) A spine `depth` nodes deep whose every node has a two-leaf inner sibling with the larger box: binary_need = depth <= 32, so the budget is 32, yet every
    wide level adopts the sibling's leaves and the next spine node -- three entries held per two spine levels -- until what is left of the budget no longer covers
    the need of the spine below, and the adoption loop is left through `does not fit`."""
    def spine(i):
        size = 2.0 ** (depth - i)      # the siblings halve down the spine, all from the corner (0, 0, 0): sibling i is larger than the whole spine below it
        if i == depth - 1:
            return inner(_cube((0, 0, 0), 0.25), _cube((0.5, 0, 0), 0.25))
        sibling = inner(_cube((0, 0, 0), size), _cube((0, 0, 0), 0.75 * size))
        return inner(sibling, spine(i + 1))
    return nodes_of(spine(0))


def comb(depth=40):
    """(b) A comb: every node a leaf and the next node; binary_need = depth > 32 takes the 0xFFFF budget."""
    def tooth(i):
        x = float(i)
        if i == depth - 1:
            return inner(_cube((x, 0, 0)), _cube((x + 1, 0, 0)))
        return inner(_cube((x, 0, 0)), tooth(i + 1))
    return nodes_of(tooth(0))


def equal_areas():
    """(c) Root {A, B}, A the larger; A = {A1, A2}; A1, A2 and B are inner nodes over unit cubes set one apart: three candidates of EQUAL half area (5) once A is adopted,
    and room for one more adoption. The first (A1) must win: the node holds A1's two leaves, A2 and B."""
    def pair(x, y):
        return inner(_cube((x, y, 0)), _cube((x + 1, y, 0)))      # a 2 x 1 x 1 box: half area 5
    a = inner(pair(0, 0), pair(0, 4))
    return nodes_of(inner(a, pair(8, 0)))


def flat():
    """(d) Every box has z = 0.5 exactly: a zero-extent axis, the -126 exponent floor."""
    def tile(x, y):
        return leaf((x, y, 0.5), (x + 1, y + 1, 0.5))
    return nodes_of(inner(inner(inner(tile(0, 0), tile(1, 0)), inner(tile(0, 1), tile(1, 1))), inner(tile(4, 4), inner(tile(5, 4), tile(5, 5)))))


def exponent_seed_trees():
    """(e) Roots over two leaves whose union has an x extent of exactly 255 * 2^k, and one ulp either side, from an origin of 0, 1 and -3: [(name, nodes, triangles)]."""
    out = []
    for k in (-20, -3, 0, 7, 30):
        for origin in (0.0, 1.0, -3.0):
            exact = np.float32(origin) + np.float32(255.0 * 2.0 ** k)
            for name, hi in (("exact", exact), ("below", np.nextafter(exact, np.float32(-np.inf))), ("above", np.nextafter(exact, np.float32(np.inf)))):
                mid = np.float32(origin) + np.float32(100.0 * 2.0 ** k)
                tree = inner(leaf((origin, 0, 0), (mid, 1, 1)), leaf((mid, 0, 0), (hi, 1, 1)))
                out.append((f"k{k}_origin{origin:g}_{name}", *nodes_of(tree)))
    return out


SYNTHETIC = {"budget_binds": budget_binds, "comb": comb, "equal_areas": equal_areas, "flat": flat}


def random_box_groups(groups, seed=4):
    """Child-box groups for the exponent sweep: (boxes (g, 4, 6) f32, counts (g,)). Magnitudes from 2^-40 to 2^40, origins near and far from zero, and -- one group in
    four -- an axis whose union extent is 255 * 2^k or one ulp either side of it; one in eight has a zero-extent axis."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 5, groups).astype(np.uint32)
    scale = np.float32(2.0) ** rng.integers(-40, 41, (groups, 1, 1)).astype(np.float32)
    origin = (rng.uniform(-1, 1, (groups, 1, 3)) * 2.0 ** rng.integers(-40, 41, (groups, 1, 1))).astype(np.float32)
    a, b = rng.uniform(0, 1, (groups, 4, 3)), rng.uniform(0, 1, (groups, 4, 3))
    lo = (origin + np.minimum(a, b).astype(np.float32) * scale).astype(np.float32)
    hi = (origin + np.maximum(a, b).astype(np.float32) * scale).astype(np.float32)
    # the seeded corner cases: child 0 reaches from the union's low corner to low + 255 * 2^k (+- one ulp) on axis 0
    special = np.nonzero(rng.integers(0, 4, groups) == 0)[0]
    for g in special:
        low = lo[g, :counts[g], 0].min()
        k = int(rng.integers(-30, 31))
        top = np.float32(low + np.float32(255.0 * 2.0 ** k))
        top = [top, np.nextafter(top, np.float32(-np.inf)), np.nextafter(top, np.float32(np.inf))][int(rng.integers(0, 3))]
        if top > low:
            hi[g, :counts[g], 0] = np.minimum(hi[g, :counts[g], 0], top)
            lo[g, :counts[g], 0] = np.minimum(lo[g, :counts[g], 0], top)
            lo[g, 0, 0], hi[g, 0, 0] = low, top
    zero = np.nonzero(rng.integers(0, 8, groups) == 0)[0]
    hi[zero, :, 2] = lo[zero, :1, 2]
    lo[zero, :, 2] = lo[zero, :1, 2]
    boxes = np.concatenate([lo, hi], axis=2).astype(np.float32)
    assert np.isfinite(boxes).all() and (boxes[:, :, 3:] >= boxes[:, :, :3]).all()
    return boxes, counts
