"""What the tests of hipr_append_scene_pools share (SceneBuilder::staged_scene_growth, csrc/pool_growth.h): the cases -- models created over NEW meshes, materials and
textures, or drawn mirrored -- the pools of a host scene by name, the tails of a staged growth applied on the CPU, and the host build of the mirror routine
(tests/native/PoolGrowthHost.hip).

The yardstick of every case is SceneBuilder::add_mesh / add_material / add_texture, insert_model / remove_model and rebuild(), byte for byte."""
import ctypes as C
from pathlib import Path

import numpy as np

import device_rebuild_bindings as rb
import instance_edit_bindings as ie
from bifrost3d_amd import capi

CORNELL, ATRIUM, TEXTURED = ie.CORNELL, ie.ATRIUM, ie.TEXTURED      # 184 triangles and 88 BVH2 nodes; 17 502 triangles; ... with textures, a texcoords pool and cut-outs

# ---- the new meshes: tiny, made here ----
BOX_POSITIONS = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], np.float32)      # vertex 4 x + 2 y + z
BOX_NORMALS = (BOX_POSITIONS / np.sqrt(0.75)).astype(np.float32)
BOX_PRIMITIVES = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.uint32)      # 12 triangles, outward
QUAD_POSITIONS = np.array([[-0.5, -0.5, 0.0], [0.5, -0.5, 0.0], [0.5, 0.5, 0.0], [-0.5, 0.5, 0.0]], np.float32)
QUAD_NORMALS = np.array([[0.0, 0.0, -1.0]] * 4, np.float32)
QUAD_TEXCOORDS = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]], np.float32)
QUAD_PRIMITIVES = np.array([[0, 2, 1], [0, 3, 2]], np.uint32)      # 2 triangles, facing -z
MESHES = {
    "box": dict(positions=BOX_POSITIONS, primitives=BOX_PRIMITIVES, normals=BOX_NORMALS),
    "quad": dict(positions=QUAD_POSITIONS, primitives=QUAD_PRIMITIVES, normals=QUAD_NORMALS, texcoords=QUAD_TEXCOORDS),
    "tinted_box": dict(positions=BOX_POSITIONS, primitives=BOX_PRIMITIVES, normals=BOX_NORMALS, tints=np.array([0x40FF2010 + 0x01010100 * v for v in range(8)], np.uint32)),
    "glowing_box": dict(positions=BOX_POSITIONS, primitives=BOX_PRIMITIVES, normals=BOX_NORMALS, emission=np.array([[0.5 + 0.25 * v, 0.2, 1.0 - 0.1 * v] for v in range(8)], np.float32)),
}
# a 4 x 4 single-channel coverage image with texels above and below the cut-off of 0.5; a 4 x 4 RGBA8 sRGB tint image
COVERAGE_R8 = np.array([[255, 255, 0, 0], [255, 200, 40, 0], [0, 90, 160, 255], [0, 0, 255, 255]], np.uint8)
TINT_RGBA8 = np.array([[[40 * x + 30, 50 * y + 20, 255 - 30 * (x + y), 255 - 20 * x] for x in range(4)] for y in range(4)], np.uint8)
TEXTURES = {
    "coverage_r8": dict(pixels=COVERAGE_R8, width=4, height=4, texel_format=capi.TEXEL_R8, is_sRGB=False, linear=(False, False)),
    "tint_rgba8": dict(pixels=TINT_RGBA8, width=4, height=4, texel_format=capi.TEXEL_RGBA8, is_sRGB=True, linear=(True, True)),
}


def material(tint=(0.8, 0.7, 0.2), roughness=0.6, specularity=0.04, metallic=0.0, flags=0, coverage=1.0, coat=0.0, coat_roughness=0.0, tint_texture=0, coverage_texture=0) -> capi.HiprMaterial:
    """SceneBuilder::make_material with the fields the cases set; texture arguments are texture indices."""
    unorm16 = lambda v: int(min(max(v, 0.0), 1.0) * 65535.0 + 0.5)
    m = capi.HiprMaterial()
    m.flags, m.shading_model = flags, capi.SHADING_DEFAULT
    m.tint[:] = tint
    m.roughness, m.specularity, m.metallic, m.coverage = roughness, specularity, metallic, coverage
    m.tint_roughness_texture_ID, m.coverage_texture_ID = tint_texture, coverage_texture
    m.coat, m.coat_roughness = unorm16(coat), unorm16(coat_roughness)
    return m


MATERIALS = {
    "cutout_r8": lambda made: material(flags=capi.MATERIAL_THIN_WALLED | capi.MATERIAL_CUTOUT, coverage=0.5, coverage_texture=made["texture coverage_r8"]),
    "coated": lambda made: material(tint=(0.1, 0.3, 0.9), roughness=0.3, coat=1.0, coat_roughness=0.2),
    "tinted_rgba8": lambda made: material(tint=(1.0, 1.0, 1.0), tint_texture=made["texture tint_rgba8"]),
    "plain": lambda made: material(),
}

IN_THE_BOX = dict(translation=(-0.2, 0.1, -0.25), rotation=(0.0, ie.Y[0], 0.0, ie.Y[1]), scale=0.2)       # inside the Cornell box, in front of the camera
BESIDE_IT = dict(translation=(0.25, 0.15, -0.3), rotation=(0.0, 0.0, 0.0, 1.0), scale=0.25)
MIRRORED = dict(translation=(0.1, 0.2, -0.3), rotation=(0.0, ie.Y[0], 0.0, ie.Y[1]), scale=-0.7)      # a negative scale turns the mesh inside out: its mirrored index triples

# An operation: ("mesh", name of MESHES), ("texture", name of TEXTURES), ("material", name of MATERIALS), ("remove", model) or ("insert", position in the instance list,
# mesh, material, pose, the new model's index) with mesh = "new <name>" or the model whose mesh is drawn again, material = "new <name>", None (that model's) or an index.
# A case is a list of ROUNDS of operations: every round is one growth (append, edit, adopt), the second one after the adoption of the first.
# (id, scene arguments, rounds, the attribute pools (texcoords, tints, emissions) before and after, the switch all_triangles_opaque before and after)
CASES = [
    ("cornell_new_box", CORNELL, [[("mesh", "box"), ("insert", 1000, "new box", 4, IN_THE_BOX, 201)]], ((False, True, False), (False, True, False)), (True, True)),
    ("cornell_first_textured_quad", CORNELL, [[("texture", "coverage_r8"), ("material", "cutout_r8"), ("mesh", "quad"), ("insert", 1000, "new quad", "new cutout_r8", BESIDE_IT, 202)]],
     ((False, True, False), (True, True, False)), (True, False)),
    ("cornell_mirrored_copy", CORNELL, [[("insert", 2, 6, None, MIRRORED, 203)]], ((False, True, False), (False, True, False)), (True, True)),
    ("cornell_new_box_and_its_mirror", CORNELL, [[("mesh", "box"), ("insert", 1000, "new box", 4, IN_THE_BOX, 204), ("insert", 0, "new box", 5, dict(BESIDE_IT, scale=-0.25), 205)]],
     ((False, True, False), (False, True, False)), (True, True)),
    ("atrium_new_box_inserted_and_one_removed", ATRIUM, [[("material", "coated"), ("mesh", "box"), ("insert", 20, "new box", "new coated", ie.NEAR, 206), ("remove", 12)]],
     ((True, False, False), (True, False, False)), (True, True)),
    ("textured_new_quad_rgba8", TEXTURED, [[("texture", "tint_rgba8"), ("material", "tinted_rgba8"), ("mesh", "quad"), ("insert", 7, "new quad", "new tinted_rgba8", ie.NEAR, 207)]],
     ((True, False, False), (True, False, False)), (False, False)),
    # the Cornell box's own boxes carry tints: there the first round brings the tail of a resident pool and only the second an absent one ...
    ("cornell_first_tints_then_emission", CORNELL, [[("mesh", "tinted_box"), ("insert", 1000, "new tinted_box", 4, IN_THE_BOX, 208)],
                                                    [("mesh", "glowing_box"), ("material", "plain"), ("insert", 3, "new glowing_box", "new plain", BESIDE_IT, 209)]],
     ((False, True, False), (False, True, True)), (True, True)),
    # ... and in the atrium, which has neither, each round brings a pool that was absent
    ("atrium_first_tints_then_emission", ATRIUM, [[("mesh", "tinted_box"), ("insert", 1000, "new tinted_box", 3, ie.NEAR, 210)],
                                                  [("mesh", "glowing_box"), ("material", "plain"), ("insert", 5, "new glowing_box", "new plain", ie.ASIDE, 211)]],
     ((True, False, False), (True, True, True)), (True, True)),
]
CASE_IDS = [c[0] for c in CASES]


def case(name):
    return CASES[CASE_IDS.index(name)]


def apply(scene, operations, made=None) -> dict:
    """The operations applied to a host scene through its add_* calls and its instance list; the triangles and the trees stay behind until rebuild() or
    adopt_edited_trees(). `made`: the indices of what earlier rounds created, by "mesh <name>" / "texture <name>" / "material <name>"; returned with this round's."""
    made = dict(made or {})
    for operation in operations:
        kind = operation[0]
        if kind == "mesh":
            made["mesh " + operation[1]] = scene.add_mesh(**MESHES[operation[1]])
        elif kind == "texture":
            made["texture " + operation[1]] = scene.add_texture(**TEXTURES[operation[1]])
        elif kind == "material":
            made["material " + operation[1]] = scene.add_material(MATERIALS[operation[1]](made))
        elif kind == "remove":
            assert scene.remove_model(operation[1])
        else:
            _, position, mesh, chosen, pose, model = operation
            info = scene.model_info(mesh) if not isinstance(mesh, str) else None
            mesh_index = made["mesh " + mesh[4:]] if isinstance(mesh, str) else info["mesh"]
            material_index = made["material " + chosen[4:]] if isinstance(chosen, str) else (info["material"] if chosen is None else chosen)
            assert scene.insert_model(position, mesh_index, material_index, model_index=model, **pose) == model
    return made


def grown_on_the_host(arguments, rounds):
    """The yardstick: the same operations, each round followed by rebuild()."""
    scene, made = rb.make_scene(arguments), {}
    for operations in rounds:
        made = apply(scene, operations, made)
        scene.rebuild()
    return scene


POOLS = ("indices", "geometry", "texcoords", "tints", "emissions", "materials", "textures", "texels")


def pools(scene) -> dict:
    """The pools of a host scene's description by name, as words (the texels as bytes); an absent attribute pool has no rows."""
    d = rb.description(scene)
    absent = {"texcoords": np.zeros((0, 2), np.uint32), "tints": np.zeros((0, 1), np.uint32), "emissions": np.zeros((0, 3), np.uint32)}
    return {name: (d[name] if d[name] is not None else absent[name]) for name in POOLS}


def unequal_pools(a: dict, b: dict) -> list:
    return [name for name in POOLS if a[name].reshape(-1).shape != b[name].reshape(-1).shape or not np.array_equal(a[name].reshape(-1), b[name].reshape(-1))]


def words_at(pointer, count, width=1, dtype=np.uint32):
    if not count or not pointer:
        return np.zeros((0, width), dtype)
    return np.ctypeslib.as_array(C.cast(pointer, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(count, width)).copy()


def segments_of(growth) -> list:
    return [(growth.segments[k].mirrored_from, growth.segments[k].index_count) for k in range(growth.segment_count)]


def applied_on_the_cpu(old: dict, growth) -> dict:
    """What hipr_append_scene_pools makes of the pools `old` (a pools() dict) and the description `growth`, on the CPU: every tail behind its pool -- an attribute pool
    that was absent comes whole -- and the index segments through the host build of the mirror routine."""
    new = {}
    vertices = len(old["geometry"])
    new["geometry"] = np.concatenate([old["geometry"], words_at(growth.geometry, growth.vertex_count, 4)])
    for name, width, array, covered in (("texcoords", 2, growth.texcoords, growth.texcoord_vertices), ("tints", 1, growth.tints, growth.tint_vertices), ("emissions", 3, growth.emissions, growth.emission_vertices)):
        if len(old[name]):
            assert covered == growth.vertex_count, f"{name}: a resident pool takes its tail"
            new[name] = np.concatenate([old[name], words_at(array, covered, width)])
        else:
            assert covered in (0, vertices + growth.vertex_count), f"{name}: an absent pool comes whole or not at all"
            new[name] = words_at(array, covered, width)
    new["materials"] = np.concatenate([old["materials"], words_at(growth.materials, growth.material_count, 16)])
    new["textures"] = np.concatenate([old["textures"], words_at(growth.textures, growth.texture_count, 6)])
    new["texels"] = np.concatenate([old["texels"], words_at(growth.texels, growth.texel_bytes, 1, np.uint8).reshape(-1)])
    resident = old["indices"].reshape(-1)
    total = len(resident) + sum(count for _, count in segments_of(growth))
    pool = np.full(total, rb.PATTERN, np.uint32)
    pool[:len(resident)] = resident
    assert grow_host_indices(pool, len(resident), growth) == total
    new["indices"] = pool.reshape(-1, 1)
    return new


def description_with(scene, grown: dict):
    """A copy of scene.desc whose pools are `grown` (an applied_on_the_cpu dict): what the device holds between the append and the edit. Returns (desc, keep-alive)."""
    d = capi.HiprSceneDesc.from_buffer_copy(bytes(scene.desc))
    keep = {name: np.ascontiguousarray(grown[name]) for name in POOLS}
    pointer = lambda name, kind: keep[name].ctypes.data_as(C.POINTER(kind)) if len(keep[name]) else None
    d.indices, d.index_count = pointer("indices", C.c_uint32), len(keep["indices"])
    d.geometry, d.vertex_count = pointer("geometry", capi.HiprVertexGeometry), len(keep["geometry"])
    d.texcoords, d.tints, d.emissions = pointer("texcoords", C.c_float), pointer("tints", C.c_uint32), pointer("emissions", C.c_float)
    d.materials, d.material_count = pointer("materials", capi.HiprMaterial), len(keep["materials"])
    d.textures, d.texture_count = pointer("textures", capi.HiprTexture), len(keep["textures"])
    d.texels, d.texel_bytes = pointer("texels", C.c_uint8), len(keep["texels"])
    return d, keep


# ---- the host build of the mirror routine (tests/native/PoolGrowthHost.hip) ----
LIB_PATH = Path(__file__).resolve().parent / "native" / "libpool_growth_host.so"
_lib = None


def library():
    global _lib
    if _lib is None:
        assert LIB_PATH.exists(), f"{LIB_PATH} is missing: run __graft_entry__.build()"
        _lib = C.CDLL(str(LIB_PATH))
        _lib.mirror_host_triples.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
        _lib.mirror_host_triples.restype = C.c_uint32
        _lib.grow_host_indices.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(capi.HiprPoolGrowth)]
        _lib.grow_host_indices.restype = C.c_longlong
    return _lib


def mirror_host_triples(pool: np.ndarray, source: int, target: int, count: int) -> int:
    """One launch of k_mirror_triples walked on the host over `pool` (uint32 words, in place). Returns the threads that wrote."""
    assert pool.dtype == np.uint32 and pool.flags["C_CONTIGUOUS"] and 3 * (target + count) <= pool.size and 3 * (source + count) <= 3 * target
    return int(library().mirror_host_triples(C.c_void_p(pool.ctypes.data), source, target, count))


def grow_host_indices(pool: np.ndarray, resident: int, growth) -> int:
    """The index segments of `growth` applied to `pool` (room for the grown pool, the first `resident` words set). Returns the grown pool's words, -1 for a refusal."""
    return int(library().grow_host_indices(C.c_void_p(pool.ctypes.data), resident, pool.size, C.byref(growth)))


def mirrored(triples: np.ndarray) -> np.ndarray:
    """(a, b, c) -> (a, c, b), SceneBuilder::index_offset_for's copy."""
    return np.ascontiguousarray(triples.reshape(-1, 3)[:, [0, 2, 1]]).reshape(-1)


def mirror_only_growth(source_triple: int, count: int):
    """A description of nothing but one mirror segment. Returns (growth, keep-alive)."""
    segments = (capi.HiprIndexSegment * 1)(capi.HiprIndexSegment(source_triple, 3 * count))
    growth = capi.HiprPoolGrowth()
    growth.segments, growth.segment_count = segments, 1
    return growth, segments
