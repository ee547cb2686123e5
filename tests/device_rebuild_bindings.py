"""What the tests of the device rebuild of the resident scene's trees share (hipr_rebuild_scene_trees, SceneBuilder::adopt_rebuilt_trees): the three moves, every
array and scalar of a description as bytes, and the scene the BVH2 build declines."""
import ctypes as C
from pathlib import Path

import numpy as np

from bifrost3d_amd import capi

POSE = dict(translation=(0.05, -0.30, 0.10), rotation=(0.0, float(np.sin(0.4)), 0.0, float(np.cos(0.4))), scale=0.3)      # test_gpu_device_refit.py's
FAR = dict(translation=(3.0, 0.5, -2.0), rotation=(0.0, float(np.sin(0.4)), 0.0, float(np.cos(0.4))), scale=0.3)
FAR2 = dict(translation=(40.0, 10.0, -25.0), rotation=(0.0, 0.0, 0.0, 1.0), scale=1.0)

# (id, scene arguments, model, pose, the uploaded tree (triangles, nodes, slots), the rebuilt tree (nodes, slots), what the host's move_model at the 1.5 rule returns)
MOVES = [
    ("cornell_far", ("cornell", dict(param0=4)), 6, FAR, (184, 88, 113), (89, 112), False),
    ("atrium_far", ("atrium", dict(param0=20000, param1=3)), 10, FAR2, (17502, 8637, 10616), (8640, 10622), False),
    ("atrium_parting_pair", ("atrium", dict(param0=20000, param1=3)), 6, POSE, (17502, 8637, 10616), (8629, 10619), False),
]
MOVE_IDS = [m[0] for m in MOVES]


def make_scene(arguments):
    from bifrost3d_amd.host import Scene
    name, keywords = arguments
    return Scene(name, **keywords)


def words(pointer, count, width):
    if not count:
        return np.zeros((0, width), np.uint32)
    return np.ctypeslib.as_array(C.cast(pointer, C.POINTER(C.c_uint32)), shape=(count, width)).copy()


def description(scene) -> dict:
    """Every array and scalar of scene.desc, by name: arrays as uint32 words (bytes for the texels and the class of nothing), scalars as ints / bit patterns."""
    d = scene.desc
    out = dict(
        nodes=words(d.nodes, d.node_count, 16), triangles=words(d.triangles, d.triangle_count, 12), instances=words(d.instances, d.instance_count, 20),
        indices=words(d.indices, d.index_count, 1), geometry=words(d.geometry, d.vertex_count, 4), materials=words(d.materials, d.material_count, 16),
        lights=words(d.lights, d.light_count, 12), textures=words(d.textures, d.texture_count, 6), wide_nodes=words(d.wide_nodes, d.wide_node_count, C.sizeof(capi.HiprWideNode) // 4),
        wide8_slots=words(d.wide8_slots, d.wide8_slot_count, 16),
        texcoords=words(d.texcoords, d.vertex_count, 2) if d.texcoords else None, tints=words(d.tints, d.vertex_count, 1) if d.tints else None,
        emissions=words(d.emissions, d.vertex_count, 3) if d.emissions else None,
        texels=np.ctypeslib.as_array(d.texels, shape=(d.texel_bytes,)).copy() if d.texel_bytes else np.zeros(0, np.uint8),
        scalars=np.array([d.node_count, d.triangle_count, d.instance_count, d.index_count, d.vertex_count, d.material_count, d.light_count, d.texture_count, d.texel_bytes, d.bvh_max_depth,
                          d.wide_node_count, d.wide_stack_entries, d.wide8_slot_count, d.wide8_height, 1 if d.environment else 0], np.uint64),
        wide8_grid=np.array(list(d.wide8_grid_min[:]) + list(d.wide8_grid_cell[:]), np.float32).view(np.uint32),
        order=scene.order(),
    )
    return out


def differences(a: dict, b: dict) -> list:
    """The names of the entries of two description() dicts that differ in a byte."""
    assert a.keys() == b.keys()
    return [k for k in a if (a[k] is None) != (b[k] is None) or (a[k] is not None and (a[k].shape != b[k].shape or not np.array_equal(a[k], b[k])))]


def write_decline_obj(path, coincident=300, side=16):
    """`coincident` identical triangles (one centroid: a range that only the median path splits, and longer than the 64 a lane of the device build sorts) among
    side x side loose ones that make the scene large enough for the 8-wide search."""
    lines = ["v 0 0 0", "v 0.5 0 0", "v 0 0.5 0"] + ["f 1 2 3"] * coincident
    v = 3
    for i in range(side):
        for j in range(side):
            ox, oz = 2.0 + i, float(j)
            lines += ["v %.9g 0 %.9g" % (ox, oz), "v %.9g 0 %.9g" % (ox + 0.9, oz), "v %.9g 0.3 %.9g" % (ox, oz + 0.9), "f %d %d %d" % (v + 1, v + 2, v + 3)]
            v += 3
    Path(path).write_text("\n".join(lines) + "\n")
    return str(path)


# ---- the host build of the device rebuild's routines (tests/native/DeviceRebuildHost.hip) ----
LIB_PATH = Path(__file__).resolve().parent / "native" / "libdevice_rebuild_host.so"
REBUILT, CLAIMED_TWICE, BUILD_DECLINED, TOO_HIGH = 0, 1, 2, 3
PATTERN = 0xA5A5A5A5
_lib = None


def library():
    global _lib
    if _lib is None:
        assert LIB_PATH.exists(), f"{LIB_PATH} is missing: run __graft_entry__.build()"
        _lib = C.CDLL(str(LIB_PATH))
        vp = C.c_void_p
        _lib.rebuild_host_trees.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    return _lib


def routines_rebuild(resident, classes, instance_count, max_depth=62) -> dict:
    """rebuild_host_trees over copies of the resident triangles ((n, 12) words, in the old tree's order) and class bytes. `status` REBUILT: `triangles`, `classes`,
    `nodes`, `order`, `slots` and `result` (node_count, deepest, the eleven words of HiprWide8BuildResult); any other status: every array as it went in, the outputs
    still PATTERN."""
    triangles = np.ascontiguousarray(resident, np.uint32).reshape(-1, 12).copy()
    classes = np.ascontiguousarray(classes, np.uint8).copy()
    n = len(triangles)
    nodes, order, slots = np.full((max(n - 1, 1), 16), PATTERN, np.uint32), np.full(n, PATTERN, np.uint32), np.full((2 * n, 16), PATTERN, np.uint32)
    result = np.full(13, PATTERN, np.uint32)
    pointer = lambda a: C.c_void_p(a.ctypes.data)
    status = library().rebuild_host_trees(pointer(triangles), pointer(classes), n, instance_count, max_depth, pointer(nodes), pointer(order), pointer(slots), pointer(result))
    out = dict(status=status, triangles=triangles, classes=classes, nodes=nodes, order=order, slots=slots, result=result)
    if status == REBUILT:
        out.update(nodes=nodes[:int(result[0])], slots=slots[:int(result[2])])
    return out
