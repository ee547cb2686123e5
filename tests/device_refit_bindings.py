"""ctypes handle on tests/native/libdevice_refit_host.so: the routines of the device refit of the 8-wide tree (csrc/wide8_refit.h) compiled for the host
(tests/native/DeviceRefitHost.hip). Test infrastructure: built by bifrost3d_amd/Makefile, loaded by tests only."""
import ctypes as C
from pathlib import Path

import numpy as np

from bifrost3d_amd import capi
from bifrost3d_amd.host import load_host_library

LIB_PATH = Path(__file__).resolve().parent / "native" / "libdevice_refit_host.so"
_fp, _up, _vp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_void_p
_lib = None


def library():
    global _lib
    if _lib is None:
        lib = C.CDLL(str(LIB_PATH))
        lib.refit_host_scene.argtypes = [_vp, C.c_uint32, _vp, _up, _up, _vp, _vp, C.c_uint32, _fp, _fp, C.POINTER(C.c_double)]
        lib.refit_host_quantise_nodes.argtypes = [_fp, _up, _fp, _vp, C.c_uint32]
        lib.refit_host_quantise_nodes.restype = None
        lib.refit_host_leaf.argtypes = [_vp, _vp, _vp, _fp]
        _lib = lib
    return _lib


def _words(pointer, rows, words):
    return np.ctypeslib.as_array(C.cast(pointer, _up), shape=(rows, words)).copy()


def refit_scene(scene, moved):
    """The device refit's routines run on copies of the scene's arrays: `moved` = [(instance index, 3x4 matrix)] (Scene.model_pose). Returns what
    hipr_refit_scene_transforms leaves on the device and reports: triangles (n, 12) and slots (n, 16) as uint32 words, grid_min, grid_cell, area, needs_rebuild."""
    d = scene.desc
    triangles = _words(d.triangles, d.triangle_count, 12)
    slots = _words(d.wide8_slots, d.wide8_slot_count, 16)
    instances = _words(d.instances, d.instance_count, 20)
    flags = np.zeros(d.instance_count, np.uint32)
    for index, matrix in moved:
        instances[index, :12] = np.asarray(matrix, np.float32).reshape(12).view(np.uint32)
        flags[index] = 1
    grid_min, grid_cell, area = np.zeros(3, np.float32), np.zeros(3, np.float32), C.c_double()
    status = library().refit_host_scene(triangles.ctypes.data, d.triangle_count, instances.ctypes.data, flags.ctypes.data_as(_up), C.cast(d.indices, _up), C.cast(d.geometry, _vp),
                                        slots.ctypes.data, d.wide8_slot_count, grid_min.ctypes.data_as(_fp), grid_cell.ctypes.data_as(_fp), C.byref(area))
    assert status >= 0, "refit_host_scene: malformed tree"
    return dict(triangles=triangles, slots=slots, grid_min=grid_min, grid_cell=grid_cell, area=area.value, needs_rebuild=status == 1)


def quantise_nodes(boxes, valid, grids, device=True):
    """`boxes` (n, 8, 6) f32 child boxes (lo xyz, hi xyz), `valid` (n,) position masks, `grids` (n, 6) grid min xyz + cell xyz -> (n, 16) uint32 node words,
    by the device's restatement (`device`) or by the host builder's quantise_node."""
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 48)
    valid = np.ascontiguousarray(valid, np.uint32)
    grids = np.ascontiguousarray(grids, np.float32).reshape(-1, 6)
    out = np.zeros((len(boxes), 16), np.uint32)
    function = library().refit_host_quantise_nodes if device else load_host_library().hiprh_wide8_quantise_nodes
    function(boxes.ctypes.data_as(_fp), valid.ctypes.data_as(_up), grids.ctypes.data_as(_fp), out.ctypes.data, len(boxes))
    return out


def refit_leaf(triangles, stored):
    """One leaf record: `triangles` (n, 12) words, `stored` (16,) words -> (rebuilt?, record words -- the stored ones when not rebuilt --, exact box)."""
    triangles = np.ascontiguousarray(triangles, np.uint32)
    stored = np.ascontiguousarray(stored, np.uint32)
    out = stored.copy()
    box = np.zeros(6, np.float32)
    ok = library().refit_host_leaf(triangles.ctypes.data, stored.ctypes.data, out.ctypes.data, box.ctypes.data_as(_fp))
    return bool(ok), out, box


def decode_tree(slots):
    """Walks the 8-wide tree of (n, 16) slot words: (is_node mask, [(node slot, [child slots])] parents before children)."""
    is_node = np.zeros(len(slots), bool)
    is_node[0] = True
    nodes = []
    queue = [0]
    while queue:
        slot = queue.pop()
        word2, base_valid = int(slots[slot, 2]), int(slots[slot, 3])
        inner_mask, base, valid = word2 >> 24, base_valid & 0xFFFFFF, base_valid >> 24
        children, rank = [], 0
        for position in range(8):
            if not valid >> position & 1:
                continue
            child = base + rank
            rank += 1
            children.append(child)
            if inner_mask >> position & 1:
                is_node[child] = True
                queue.append(child)
        nodes.append((slot, children))
    return is_node, nodes


def exact_boxes(slots, triangles):
    """The exact box (lo xyz, hi xyz, f32) of every slot from the triangles its records name: what the area of hipr_refit_scene_transforms sums."""
    is_node, nodes = decode_tree(slots)
    corners = triangles[:, :9].view(np.float32).reshape(-1, 3, 3)
    boxes = np.zeros((len(slots), 6), np.float32)
    for slot in np.nonzero(~is_node)[0]:
        ids = [int(t) for t in slots[slot, 12:14] if t != 0xFFFFFFFF]
        points = corners[ids].reshape(-1, 3)
        boxes[slot, :3], boxes[slot, 3:] = points.min(axis=0), points.max(axis=0)
    for slot, children in sorted(nodes, key=lambda n: -n[0]):      # a child's slot is always greater than its parent's
        boxes[slot, :3], boxes[slot, 3:] = boxes[children, :3].min(axis=0), boxes[children, 3:].max(axis=0)
    return boxes


def half_area_sum(boxes):
    """Box::half_area per box in f32 as the builder writes it, over every slot but the root, summed in f64."""
    d = (boxes[1:, 3:] - boxes[1:, :3]).astype(np.float32)
    areas = (d[:, 0] * d[:, 1]).astype(np.float32) + (d[:, 1] * d[:, 2]).astype(np.float32)
    areas = (areas.astype(np.float32) + (d[:, 2] * d[:, 0]).astype(np.float32)).astype(np.float32)
    return float(areas.astype(np.float64).sum())


SMALL_POSE = dict(translation=(1.0, 0.0, 0.0), scale=0.3)      # the pose the parting pair's scene is built in
LARGE_POSE = dict(translation=(1.0, 0.0, 0.0), scale=1.0)      # ... and the pose in which the pair parts


def write_parting_pair_obj(path, filler=16):
    """Two triangles (a, b, c) and (a', c, d) whose corners a and a' are DISTINCT object-space vertices one ulp apart in x that round to one world position under
    SMALL_POSE (x * 0.3 + 1 in f32, SceneBuilder's expression) and part under LARGE_POSE, found by search; `filler`^2 loose triangles next to them make the scene
    large enough for the 8-wide search (more than 64 BVH2 nodes). A scene built in SMALL_POSE pairs the two triangles into one leaf record."""
    f32 = np.float32
    rng = np.random.default_rng(5)
    scale, shift = f32(SMALL_POSE["scale"]), f32(SMALL_POSE["translation"][0])
    for _ in range(100000):
        x = f32(rng.uniform(1.0, 2.0))
        neighbour = np.nextafter(x, f32(4.0))
        if f32(f32(scale * x) + shift) == f32(f32(scale * neighbour) + shift) and f32(x + f32(1.0)) != f32(neighbour + f32(1.0)):
            break
    else:
        raise AssertionError("no pair of neighbouring floats rounds together")
    lines = ["v %.9g 0 0" % x, "v 3 0 0.5", "v 3 1 0.25", "v %.9g 0 0" % neighbour, "v 1.5 1 0.125", "f 1 2 3", "f 4 3 5"]
    v = 5
    for i in range(filler):
        for j in range(filler):
            ox, oz = 5.0 + i, float(j)
            lines += ["v %.9g 0 %.9g" % (ox, oz), "v %.9g 0 %.9g" % (ox + 0.9, oz), "v %.9g 0.3 %.9g" % (ox, oz + 0.9), "f %d %d %d" % (v + 1, v + 2, v + 3)]
            v += 3
    Path(path).write_text("\n".join(lines) + "\n")
    return str(path)


def scene_with_a_parting_pair(path):
    """The scene of write_parting_pair_obj, rebuilt in SMALL_POSE (a move with a rebuild threshold nothing meets), with the pair in one record."""
    from bifrost3d_amd.host import Scene
    scene = Scene("file:" + write_parting_pair_obj(path))
    assert scene.move_model(1, rebuild_threshold=1e-9, **SMALL_POSE) is False      # rebuilt in the small pose
    slots, triangles = _words(scene.desc.wide8_slots, scene.desc.wide8_slot_count, 16), scene.triangles()
    is_node, _ = decode_tree(slots)
    pairs = [(int(triangles[slots[s, 12], 10]), int(triangles[slots[s, 13], 10])) for s in np.nonzero(~is_node)[0] if slots[s, 13] != 0xFFFFFFFF]
    assert pairs == [(0, 1)], pairs      # the builder did pair primitives 0 and 1, and nothing else
    return scene
