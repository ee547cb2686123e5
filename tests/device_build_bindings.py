"""ctypes handle on tests/native/libdevice_build_host.so -- the routines of the device BVH2 build (csrc/bvh2_build.h) compiled for the host
(tests/native/DeviceBuildHost.hip) -- the host builder behind hiprh_bvh_build, and the triangle sets both suites build. Test infrastructure: the library is built
by bifrost3d_amd/Makefile and loaded by tests only."""
import ctypes as C
from pathlib import Path

import numpy as np

from bifrost3d_amd import capi
from bifrost3d_amd.host import load_host_library

LIB_PATH = Path(__file__).resolve().parent / "native" / "libdevice_build_host.so"
_up, _vp = C.POINTER(C.c_uint32), C.c_void_p
_lib = None
PATTERN = 0xA5A5A5A5      # what an output buffer holds before a build that must not write it


def library():
    global _lib
    if _lib is None:
        lib = C.CDLL(str(LIB_PATH))
        lib.build_host_bvh2.argtypes = [_vp, C.c_uint32, C.c_uint32, _vp, C.c_uint32, _up, _vp, _up, _up]
        lib.build_host_short_range.restype = C.c_uint
        lib.build_host_median_lane_limit.restype = C.c_uint
        _lib = lib
    return _lib


def median_lane_limit() -> int:
    return int(library().build_host_median_lane_limit())


def host_build(triangles, max_depth=62) -> dict:
    """The host builder (hiprh_bvh_build): nodes (count, 16) and order as uint32 words, the deepest leaf, and the test-only counters of its median splits."""
    lib = load_host_library()
    triangles = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 12)
    handle = lib.hiprh_bvh_build(C.cast(triangles.ctypes.data, C.POINTER(capi.HiprTriangle)), len(triangles), max_depth)
    assert handle
    try:
        return _from_handle(lib, handle, len(triangles))
    finally:
        lib.hiprh_bvh_destroy(handle)


def _from_handle(lib, handle, n) -> dict:
    count = lib.hiprh_bvh_node_count(handle)
    nodes = np.ctypeslib.as_array(C.cast(lib.hiprh_bvh_nodes(handle), _up), shape=(count, 16)).copy()
    order = np.ctypeslib.as_array(C.cast(lib.hiprh_bvh_order(handle), _up), shape=(n,)).copy()
    wide_count = lib.hiprh_bvh_wide_node_count(handle)
    wide = np.ctypeslib.as_array(C.cast(lib.hiprh_bvh_wide_nodes(handle), _up), shape=(wide_count, 16)).copy()
    return dict(nodes=nodes, order=order, deepest=lib.hiprh_bvh_max_depth(handle) - 1, wide_nodes=wide, median_splits=lib.hiprh_bvh_median_splits(handle),
                longest_median_range=lib.hiprh_bvh_longest_median_range(handle))


def host_build_on_device(ctx, triangles, max_depth=62):
    """hiprh_bvh_build_on_device: (status, dict as host_build or None)."""
    lib = load_host_library()
    triangles = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 12)
    status = C.c_int(0)
    handle = lib.hiprh_bvh_build_on_device(ctx.handle, C.cast(triangles.ctypes.data, C.POINTER(capi.HiprTriangle)), len(triangles), max_depth, C.byref(status))
    if not handle:
        return status.value, None
    try:
        return status.value, _from_handle(lib, handle, len(triangles))
    finally:
        lib.hiprh_bvh_destroy(handle)


def routines_build(triangles, max_depth=62) -> dict:
    """The device build's routines on the host (build_host_bvh2). status 0: built; 1: declined, `decline` = (begin, end), nodes and order still hold PATTERN."""
    triangles = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 12)
    n = len(triangles)
    nodes = np.full((max(n - 1, 1), 16), PATTERN, np.uint32)
    order = np.full(n, PATTERN, np.uint32)
    node_count, deepest, decline = C.c_uint32(0), C.c_uint32(0), (C.c_uint32 * 2)()
    status = library().build_host_bvh2(triangles.ctypes.data, n, max_depth, nodes.ctypes.data, len(nodes), C.byref(node_count), order.ctypes.data, C.byref(deepest), decline)
    assert status >= 0, "build_host_bvh2: bad argument or a build off its bounds"
    if status == 1:
        return dict(status=1, nodes=nodes, order=order, deepest=0, decline=(int(decline[0]), int(decline[1])))
    return dict(status=0, nodes=nodes[:node_count.value], order=order, deepest=int(deepest.value), decline=None)


def same_tree(ours, theirs):
    """Byte equality of nodes (64 B each), order and depth, with the first difference named."""
    assert ours["nodes"].shape == theirs["nodes"].shape, (ours["nodes"].shape, theirs["nodes"].shape)
    different = np.nonzero((ours["nodes"] != theirs["nodes"]).any(axis=1))[0]
    assert len(different) == 0, (len(different), different[:4], ours["nodes"][different[:1]], theirs["nodes"][different[:1]])
    assert np.array_equal(ours["order"], theirs["order"])
    assert ours["deepest"] == theirs["deepest"]
    return True


# ---- triangle sets: (n, 12) uint32 words of HiprTriangle ----
def pack(corners) -> np.ndarray:
    """`corners` (n, 3, 3) f32 -> triangles with instance 0, primitive k, flags opaque."""
    corners = np.ascontiguousarray(corners, np.float32)
    out = np.zeros((len(corners), 12), np.uint32)
    out[:, :9] = corners.reshape(-1, 9).view(np.uint32)
    out[:, 10] = np.arange(len(corners))
    out[:, 11] = 1
    return out


def random_triangles(n, seed, size=0.05):
    rng = np.random.default_rng(seed)
    centre = rng.uniform(0, 1, (n, 1, 3))
    return pack(centre + rng.uniform(-size, size, (n, 3, 3)))


def strip(n=257):
    """Triangles along x in the plane z = 0 whose centroids differ in x only: two centroid extents are zero."""
    x = np.arange(n, dtype=np.float32)[:, None]
    base = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 1.0, 0.0]], np.float32)
    corners = np.tile(base, (n, 1, 1))
    corners[:, :, 0] += 0.5 * x
    return pack(corners)


def signed_zeros(negative_first: bool):
    """Random triangles in [0, 1]^3 and [-1, 0]^3 of which many touch the planes x, y, z = 0 with a corner written as -0.0f or +0.0f: wherever a box bound is a
    zero, its sign is that of the first triangle in range order that reaches it. `negative_first` decides which sign appears first in the input."""
    rng = np.random.default_rng(5)
    n = 400
    corners = rng.uniform(0.05, 1, (n, 3, 3)).astype(np.float32)
    corners[n // 2:] *= -1
    touch = rng.integers(0, 3, n)
    zero = np.where((np.arange(n) % 2 == 0) == negative_first, np.float32(-0.0), np.float32(0.0))
    for k in range(n):
        corners[k, rng.integers(0, 3), touch[k]] = zero[k]
        if k % 5 == 0:      # some reach a second plane with the other zero
            corners[k, rng.integers(0, 3), (touch[k] + 1) % 3] = -zero[k]
    return pack(corners)


def with_cluster(n=500, copies=6, seed=9):
    """A random set with `copies` identical triangles in its midst: the cluster ends in a range of coincident centroids, a short median range."""
    triangles = random_triangles(n, seed)
    at = n // 3
    triangles[at:at + copies, :9] = triangles[at, :9]
    return triangles


def identical(n=300):
    return pack(np.tile(np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.5]], np.float32), (n, 1, 1)))


def skewed(n=64, seed=13):
    """Centres crowded towards one corner (u^8): the SAH peels off a few triangles per level, so under max_depth = 8 the depth budget forces medians on short ranges."""
    rng = np.random.default_rng(seed)
    return pack(rng.uniform(0, 1, (n, 1, 3)) ** 8 + rng.uniform(-1e-4, 1e-4, (n, 3, 3)))
