"""What the tests of hipr_edit_scene_instances share (SceneBuilder::remove_model / insert_model / adopt_edited_trees, csrc/instance_edit.h): the edits, each with the
counts the host builder gives for it, and the host build of the device's routines (tests/native/InstanceEditHost.hip)."""
import ctypes as C
from pathlib import Path

import numpy as np

import device_rebuild_bindings as rb
import material_update_bindings as mu
from bifrost3d_amd import capi

CORNELL = ("cornell", dict(param0=4))                                  # 184 triangles, 88 BVH2 nodes, 7 models
ATRIUM = ("atrium", dict(param0=20000, param1=3))                      # 17 502 triangles, 46 models; models 4, 10, 26, 32, 38 are coated
TEXTURED = ("atrium", dict(param0=20000, param1=3, textured=True))     # ... whose banners (models 41 - 46) are cut-outs through a coverage texture

Y = float(np.sin(0.4)), float(np.cos(0.4))
NEAR = dict(translation=(0.6, 0.4, -0.8), rotation=(0.0, Y[0], 0.0, Y[1]), scale=0.7)
ASIDE = dict(translation=(-1.5, 0.2, 1.1), rotation=(0.0, 0.0, 0.0, 1.0), scale=1.0)

# An edit is a list of operations in order: ("remove", model) or ("insert", position in the instance list, the model whose mesh is drawn again, material (None: that
# model's), pose, the new model's index). `prepare` operations are applied, with a rebuild(), BEFORE the scene is uploaded: they make the scene the edit starts from.
# (id, scene arguments, prepare, operations, the edited scene's (triangles, BVH2 nodes, 8-wide slots), its switches (all triangles opaque, any triangle coated))
EDITS = [
    ("cornell_remove_last", CORNELL, [], [("remove", 7)], (172, 83, 103), (True, False)),
    ("atrium_remove_one", ATRIUM, [], [("remove", 12)], (17208, 8481, 10467), (True, True)),
    ("atrium_append_copy", ATRIUM, [], [("insert", 1000, 6, None, NEAR, 101)], (17796, 8778, 10785), (True, True)),
    ("atrium_insert_middle", ATRIUM, [], [("insert", 20, 30, None, ASIDE, 102)], (17802, 8778, 10812), (True, True)),
    ("atrium_remove_two_add_one", ATRIUM, [], [("remove", 3), ("remove", 44), ("insert", 10, 42, None, ASIDE, 103)], (17172, 8477, 10349), (True, True)),
    ("textured_cutout_copy", TEXTURED, [], [("insert", 7, 41, None, NEAR, 104)], (18398, 9075, 11168), (False, True)),
    ("textured_remove_every_cutout", TEXTURED, [], [("remove", m) for m in range(41, 47)], (12126, 5963, 7342), (True, True)),
    ("atrium_first_coated", ATRIUM, [("remove", m) for m in (4, 10, 26, 32, 38)], [("insert", 3, 6, 11, NEAR, 105)], (16224, 8021, 9809), (True, True)),
]
EDIT_IDS = [e[0] for e in EDITS]
# The refusal: what is left of the Cornell box without its walls has at most 64 BVH2 nodes, and a fresh upload would trace it through another search.
TOO_SMALL = ("cornell_too_small", CORNELL, [], [("remove", m) for m in (1, 2, 3, 4)], None, None)


def apply(scene, operations):
    """The operations applied to a host scene's instance list; the triangles and the trees stay behind until rebuild() or adopt_edited_trees()."""
    for operation in operations:
        if operation[0] == "remove":
            assert scene.remove_model(operation[1])
        else:
            _, position, source, material, pose, model = operation
            info = scene.model_info(source)
            assert scene.insert_model(position, info["mesh"], info["material"] if material is None else material, model_index=model, **pose) == model


def prepared(arguments, prepare):
    """The scene an edit starts from."""
    scene = rb.make_scene(arguments)
    if prepare:
        apply(scene, prepare)
        scene.rebuild()
    return scene


def edited_on_the_host(arguments, prepare, operations):
    """The yardstick: the same operations followed by rebuild()."""
    scene = prepared(arguments, prepare)
    apply(scene, operations)
    scene.rebuild()
    return scene


def switches(scene):
    """(all triangles opaque, any triangle coated) of a host scene, as hipr_upload_scene derives them."""
    return bool((scene.triangles()[:, 11] & capi.TRIANGLE_OPAQUE).all()), bool(mu.derived_arrays(scene)[2].any())


# ---- the host build of the edit's routines (tests/native/InstanceEditHost.hip) ----
LIB_PATH = Path(__file__).resolve().parent / "native" / "libinstance_edit_host.so"
EDITED, CLAIMED, BUILD_DECLINED, TOO_HIGH, BAD_INDEX, TOO_FEW_NODES, NO_TRIANGLE = 0, 1, 2, 3, 4, 5, 6
PATTERN = rb.PATTERN
_lib = None


def library():
    global _lib
    if _lib is None:
        assert LIB_PATH.exists(), f"{LIB_PATH} is missing: run __graft_entry__.build()"
        _lib = C.CDLL(str(LIB_PATH))
        vp = C.c_void_p
        _lib.edit_host_scene.argtypes = [vp, vp, C.c_uint32, C.POINTER(capi.HiprSceneDesc), C.POINTER(capi.HiprInstanceEdit), C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp]
    return _lib


def routines_edit(resident, classes, pools, edits, max_depth=62) -> dict:
    """edit_host_scene over the resident triangles ((n, 12) words, in the old tree's order), their class bytes, the pools and old instances of the description `pools`
    and the list `edits` (a ctypes array of capi.HiprInstanceEdit). `status` EDITED: `triangles`, `classes`, `nodes`, `order`, `slots` cut to their counts and
    `result` (triangle count, node_count, deepest, the eleven words of HiprWide8BuildResult, all opaque, any coated); any other status: every output still PATTERN."""
    resident = np.ascontiguousarray(resident, np.uint32).reshape(-1, 12)
    classes = np.ascontiguousarray(classes, np.uint8)
    capacity = len(resident) + sum(int(e.primitive_count) for e in edits if e.source == capi.EDIT_NEW_INSTANCE)
    triangles, out_classes = np.full((capacity, 12), PATTERN, np.uint32), np.full(capacity, 0xA5, np.uint8)
    nodes, order, slots = np.full((max(capacity - 1, 1), 16), PATTERN, np.uint32), np.full(capacity, PATTERN, np.uint32), np.full((2 * capacity, 16), PATTERN, np.uint32)
    result = np.full(16, PATTERN, np.uint32)
    pointer = lambda a: C.c_void_p(a.ctypes.data)
    status = library().edit_host_scene(pointer(resident), pointer(classes), len(resident), C.byref(pools), edits, len(edits), max_depth, capacity, pointer(triangles), pointer(out_classes),
                                       pointer(nodes), pointer(order), pointer(slots), pointer(result))
    out = dict(status=status, triangles=triangles, classes=out_classes, nodes=nodes, order=order, slots=slots, result=result)
    if status == EDITED:
        n = int(result[0])
        out.update(triangles=triangles[:n], classes=out_classes[:n], order=order[:n], nodes=nodes[:int(result[1])], slots=slots[:int(result[3])])
    return out


def untouched(answer) -> bool:
    return ((answer["triangles"] == PATTERN).all() and (answer["classes"] == 0xA5).all() and (answer["nodes"] == PATTERN).all() and (answer["order"] == PATTERN).all()
            and (answer["slots"] == PATTERN).all() and (answer["result"] == PATTERN).all())


def wide8_of(result_words) -> capi.HiprWide8BuildResult:
    return capi.HiprWide8BuildResult.from_buffer_copy(np.ascontiguousarray(result_words[3:14], np.uint32).tobytes())
