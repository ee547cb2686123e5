"""What the tests of hipr_update_scene_vertices share (csrc/vertex_update.h, SceneBuilder::update_vertices): the scene -- the Cornell box with walls of 4 x 4 quads
(the 8-wide tree exists) plus a lace banner of 16 x 16 cells (289 vertices) with a cut-out material, a box mesh worn by two models and by a mirrored third, a box with
tints and emissions, a quad with vertices no triangle references and a quad whose two triangles meet in coincident seam vertices -- the cases of vertex edits, the
counts made with numpy from the builder's indices, and ctypes access to the host build of the update's kernel bodies (tests/native/VertexUpdateHost.hip). Test
infrastructure: built by bifrost3d_amd/Makefile, loaded by tests only.

The yardstick of every case is SceneBuilder: update_vertices on the built scene, and a scene made anew from the edited mesh data."""
import ctypes as C
from pathlib import Path

import numpy as np

import material_update_bindings as mu
import pool_growth_bindings as pg
import texel_update_bindings as tu
from bifrost3d_amd import capi
from bifrost3d_amd.host import Scene

GEOMETRY = capi.vertex_geometry_dtype()
MESH_TEXCOORDS = 2      # HIPR_MESH_TEXCOORDS
SIZE = 32      # the coverage texture: solid but for a hole of 8 x 8 texels in its last corner
LACE_CELLS, LACE_COORDS = 16, (0.125, 0.5)      # texels 4 to 16: with the slack texel around a triangle's box, clear of the hole and of the seam it repeats across
# model indices
LACE, BOX_A, BOX_B, BOX_MIRRORED, GLOWING, LOOSE, SEAM = 202, 203, 204, 205, 206, 207, 208
POSES = {
    LACE: pg.BESIDE_IT, BOX_A: pg.IN_THE_BOX, BOX_B: dict(translation=(0.2, -0.3, 0.1), rotation=(0.0, 0.0, 0.0, 1.0), scale=0.15),
    BOX_MIRRORED: dict(translation=(-0.3, -0.3, -0.2), rotation=(0.0, 0.0, 0.0, 1.0), scale=-0.15), GLOWING: dict(translation=(0.0, -0.35, -0.3), rotation=(0.0, 0.0, 0.0, 1.0), scale=0.12),
    LOOSE: dict(translation=(-0.3, 0.2, 0.0), rotation=(0.0, 0.0, 0.0, 1.0), scale=0.2), SEAM: dict(translation=(0.3, 0.3, 0.1), rotation=(0.0, 0.0, 0.0, 1.0), scale=0.2),
}


def coverage_image():
    image = np.full((SIZE, SIZE), 255, np.uint8)
    image[24:, 24:] = 0
    return image


def mesh_data():
    """The meshes by name, as Scene.add_mesh takes them. The lace's texture coordinates keep to the image's solid part: every triangle is covered."""
    lace = tu.tessellated_quad(LACE_CELLS, LACE_COORDS)
    box = dict(positions=pg.BOX_POSITIONS.copy(), primitives=pg.BOX_PRIMITIVES, normals=pg.BOX_NORMALS.copy())
    glowing = dict(box, tints=np.array([0x40FF2010 + 0x01010100 * v for v in range(8)], np.uint32), emission=np.tile(np.array([0.5, 0.4, 0.1], np.float32), (8, 1)))
    loose = dict(positions=np.concatenate([pg.QUAD_POSITIONS, np.array([[2.0, 2.0, 0.0], [0.1, 0.2, 0.3], [-3.0, 0.0, 1.0]], np.float32)]), primitives=pg.QUAD_PRIMITIVES,
                 normals=np.tile(pg.QUAD_NORMALS[0], (7, 1)), texcoords=np.concatenate([np.float32(0.125) + pg.QUAD_TEXCOORDS * np.float32(0.375), np.zeros((3, 2), np.float32)]))
    seam = dict(positions=pg.QUAD_POSITIONS[[0, 2, 1, 0, 3, 2]], primitives=np.array([[0, 1, 2], [3, 4, 5]], np.uint32), normals=np.tile(pg.QUAD_NORMALS[0], (6, 1)))
    return dict(lace=lace, box=box, loose=loose, seam=seam, glowing=glowing)      # the glowing box last: the pool ends in vertices triangles read


def make_scene(meshes=None, lace_material="cutout"):
    """The scene built on the host. `meshes`: mesh data by name in place of mesh_data()'s (a builder made anew from edited data); lace_material: "cutout", or "plain"
    for a lace whose material leaves nothing to its texture. Returns (scene, info): the mesh indices by name, the materials, the mesh data as given."""
    meshes = dict(mesh_data(), **(meshes or {}))
    scene = Scene("cornell", param0=4)
    coverage = scene.add_texture(coverage_image(), SIZE, SIZE, capi.TEXEL_R8, linear=(False, False))
    cutout = scene.add_material(pg.material(flags=capi.MATERIAL_THIN_WALLED | capi.MATERIAL_CUTOUT, coverage=0.5, coverage_texture=coverage))
    plain = scene.add_material(pg.material())
    index = {name: scene.add_mesh(**data) for name, data in meshes.items()}
    for model, mesh, material in [(LACE, "lace", cutout if lace_material == "cutout" else plain), (BOX_A, "box", plain), (BOX_B, "box", plain), (BOX_MIRRORED, "box", plain), (GLOWING, "glowing", plain),
                                  (LOOSE, "loose", cutout), (SEAM, "seam", plain)]:
        assert scene.insert_model(1000, index[mesh], material, model_index=model, **POSES[model]) == model
    scene.rebuild()
    return scene, dict(mesh=index, cutout=cutout, plain=plain, data=meshes)


# ---- the pools and the counts, from the builder ----
def pool(scene, name):
    """A copy of a vertex pool of the builder's description: "geometry" as records, the others as rows of floats / words; None for an absent pool."""
    d = scene.desc
    pointer, dtype, width = dict(geometry=(d.geometry, np.uint32, 4), texcoords=(d.texcoords, np.float32, 2), tints=(d.tints, np.uint32, 1), emissions=(d.emissions, np.float32, 3))[name]
    if not pointer:
        return None
    rows = pg.words_at(pointer, d.vertex_count, width, dtype)
    return rows.view(GEOMETRY).reshape(-1) if name == "geometry" else rows


def of_mesh(scene, mesh, name):
    """The rows of mesh `mesh` in pool `name`."""
    r = scene.mesh_range(mesh)
    return pool(scene, name)[r["vertex_offset"]:r["vertex_offset"] + r["vertex_count"]].copy()


def pooled(scene, edits):
    """Mesh-relative edits in POOL coordinates, what Context.update_scene_vertices takes (Scene.stage_vertex_edits makes the same, and writes)."""
    return [dict({k: v for k, v in e.items() if k != "mesh"}, first=scene.mesh_range(e["mesh"])["vertex_offset"] + e["first"]) for e in edits]


def marked(scene, edits, name):
    """A flag per pool vertex: some edit carries attribute `name` for it."""
    marks = np.zeros(scene.desc.vertex_count, bool)
    for e in pooled(scene, edits):
        if e.get(name) is not None:
            count = len(np.ascontiguousarray(e[name]).reshape(-1).view(np.uint8)) // dict(geometry=16, texcoords=8)[name]
            marks[e["first"]:e["first"] + count] = True
    return marks


def corners_marked(scene, marks):
    """Per triangle of scene.triangles(): one of its three pool vertices -- through its instance's own index triple -- is marked."""
    triangles, instances, d = scene.triangles(), scene.instances_array(), scene.desc
    indices = pg.words_at(d.indices, d.index_count // 3, 3)
    instance, primitive = triangles[:, 9], triangles[:, 10]
    triples = indices[instances[instance, 12] + primitive] + instances[instance, 13][:, None]
    return marks[triples].any(axis=1)


def expected_counts(scene, info, edits):
    """moved_triangles and candidate_triangles, counted BEFORE the builder applies the edits (neither depends on values)."""
    triangles, instances = scene.triangles(), scene.instances_array()
    moved = int(corners_marked(scene, marked(scene, edits, "geometry")).sum())
    decides = (instances[:, 15] == info["cutout"]) & (instances[:, 16] & MESH_TEXCOORDS != 0)
    candidates = int((corners_marked(scene, marked(scene, edits, "texcoords")) & decides[triangles[:, 9]]).sum())
    return moved, candidates


# ---- the edits of the cases ----
def geometry_edit(scene, info, name, first, count, move=None, normals=None):
    """Vertices [first, first + count) of mesh `name` with their positions displaced by `move` (a vector, rows, or a function of the positions) and, `normals`, other
    normals (rows); what is not given stays as the pool holds it."""
    mesh = info["mesh"][name]
    records = of_mesh(scene, mesh, "geometry")[first:first + count]
    if move is not None:
        records["position"] = records["position"] + (move(records["position"]) if callable(move) else np.asarray(move, np.float32))
    if normals is not None:
        records = scene.vertex_geometry(records["position"], normals)
    return dict(mesh=mesh, first=first, geometry=records)


def wobble(seed, scale=0.02):
    return lambda positions: np.random.default_rng(seed).uniform(-scale, scale, positions.shape).astype(np.float32)


def onto_the_hole(scene, info, first, count):
    """Texture coordinates of `count` lace vertices from `first` on moved onto the hole of the coverage image."""
    return dict(mesh=info["mesh"]["lace"], first=first, texcoords=np.tile(np.array([0.875, 0.875], np.float32), (count, 1)))


def lace_texcoords(scene, info, first, count):
    return dict(mesh=info["mesh"]["lace"], first=first, texcoords=mesh_data()["lace"]["texcoords"][first:first + count])


def shifted_texcoords(scene, info, first, count, by=0.01):
    return dict(mesh=info["mesh"]["lace"], first=first, texcoords=mesh_data()["lace"]["texcoords"][first:first + count] + np.float32(by))


# ---- the cases: name -> function of (scene, info) returning the steps; a step = (the edits MESH-relative, as the builder takes them; the edits in POOL coordinates as the
#      device takes them, or None for pooled() of the former) ----
def _ranges(count):
    return lambda scene, info: [([geometry_edit(scene, info, "lace", 3, count, move=wobble(count))], None)]


def _first_and_last_vertex(scene, info):
    first = dict(_cornell_edit(scene, 2), tints=np.array([0x11223344, 0x55667788], np.uint32))
    last = geometry_edit(scene, info, "glowing", 6, 2, move=wobble(6))
    last.update(tints=np.array([0x80102030, 0x80405060], np.uint32), emissions=np.array([[1.0, 0.5, 0.25], [0.0, 2.0, 0.0]], np.float32))
    return [([first, last], None)]


def _cornell_edit(scene, count):
    """The first `count` vertices of the pool (mesh 0, a wall of the Cornell box) nudged."""
    records = of_mesh(scene, 0, "geometry")[:count]
    records["position"] = records["position"] + wobble(5, 0.005)(records["position"])
    return dict(mesh=0, first=0, geometry=records)


def _across_two_meshes(scene, info):
    box, loose = geometry_edit(scene, info, "box", 7, 1, move=(0.05, 0.0, 0.02)), geometry_edit(scene, info, "loose", 0, 1, move=(0.0, 0.04, 0.0))
    one = dict(first=scene.mesh_range(info["mesh"]["box"])["vertex_offset"] + 7, geometry=np.concatenate([box["geometry"], loose["geometry"]]))
    assert scene.mesh_range(info["mesh"]["loose"])["vertex_offset"] == one["first"] + 1
    return [([box, loose], [one])]


def _overlapping(scene, info):
    return [([geometry_edit(scene, info, "lace", 10, 30, move=wobble(7)), geometry_edit(scene, info, "lace", 30, 30, move=wobble(8)), geometry_edit(scene, info, "lace", 20, 5, move=wobble(9))], None)]


def _two_attributes(in_one):
    def steps(scene, info):
        geometry, texcoords = geometry_edit(scene, info, "lace", 0, 20, move=wobble(10)), shifted_texcoords(scene, info, 0, 20)
        return [([dict(geometry, texcoords=texcoords["texcoords"])] if in_one else [geometry, texcoords], None)]
    return steps


def _beyond_and_back(scene, info):
    out = geometry_edit(scene, info, "box", 0, 1, move=(0.0, -9.0, 0.0))
    back = dict(out, geometry=out["geometry"].copy())
    back["geometry"]["position"] = back["geometry"]["position"] + np.array([0.0, 8.5, 0.0], np.float32)      # inward again, not where it was
    return [([out], None), ([back], None)]


def _normals_only(scene, info):
    tilted = np.tile(np.array([0.6, 0.0, -0.8], np.float32), (289, 1))
    return [([geometry_edit(scene, info, "lace", 0, 289, normals=tilted)], None)]


def _tints_and_emissions(scene, info):
    tints, emissions = np.arange(8, dtype=np.uint32) * 0x01020304 + 0x80000000, np.random.default_rng(3).uniform(0.0, 2.0, (8, 3)).astype(np.float32)
    return [([dict(mesh=info["mesh"]["glowing"], first=0, tints=tints, emissions=emissions)], None), ([dict(mesh=info["mesh"]["box"], first=0, tints=tints), dict(mesh=info["mesh"]["box"], first=0, emissions=emissions)], None)]


CASES = {
    "range_1": _ranges(1), "range_63": _ranges(63), "range_64": _ranges(64), "range_65": _ranges(65), "range_257": _ranges(257),
    "first_and_last_vertex_of_the_pool": _first_and_last_vertex,
    "last_of_one_mesh_and_first_of_the_next_in_one_edit": _across_two_meshes,
    "overlapping_later_wins": _overlapping,
    "two_attributes_in_one_edit": _two_attributes(True), "two_attributes_in_two_edits": _two_attributes(False),
    "mesh_worn_by_two_and_a_mirrored_twin": lambda scene, info: [([geometry_edit(scene, info, "box", 0, 8, move=wobble(11, 0.1))], None)],
    "vertices_no_triangle_reads": lambda scene, info: [([geometry_edit(scene, info, "loose", 4, 3, move=(0.5, 0.5, 0.5))], None)],
    "identical_values": lambda scene, info: [([dict(geometry_edit(scene, info, "lace", 0, 289), texcoords=mesh_data()["lace"]["texcoords"])], None)],
    "beyond_the_bounds_and_inward_again": _beyond_and_back,
    "normals_only": _normals_only,
    "onto_the_hole_and_back": lambda scene, info: [([onto_the_hole(scene, info, 0, 3)], None), ([lace_texcoords(scene, info, 0, 3)], None)],
    "tints_and_emissions": _tints_and_emissions,
}
CASE_IDS = list(CASES)


# ---- the host build of the kernel bodies (tests/native/VertexUpdateHost.hip) ----
LIB_PATH = Path(__file__).resolve().parent / "native" / "libvertex_update_host.so"
_lib = None


def library():
    global _lib
    if _lib is None:
        assert LIB_PATH.exists(), f"{LIB_PATH} is missing: run __graft_entry__.build()"
        _lib = C.CDLL(str(LIB_PATH))
        vp, u32 = C.c_void_p, C.c_uint32
        _lib.vertex_update_host_scene.argtypes = [vp, u32, vp, u32, vp, vp, vp, vp, vp, vp, u32, vp, u32, vp, C.POINTER(capi.HiprVertexEdit), u32, vp, vp, vp, vp, u32, vp, vp, vp, vp]
        _lib.vertex_update_host_plan.argtypes = [C.POINTER(capi.HiprVertexEdit), u32, vp, u32, vp]
        _lib.vertex_update_host_plan.restype = u32
    return _lib


def arrays_of(scene):
    """Copies of what the passes rewrite or must leave alone, as the device holds them after an upload: the four pools, the triangles, the slots, the grid, and the
    trace and shading records as a pattern but for the words the flag pass writes (material_update_bindings.derived_arrays)."""
    trace, shade, classes = mu.derived_arrays(scene)
    d = scene.desc
    held = dict(triangles=scene.triangles(), trace=trace, shade=shade, classes=classes, slots=scene.wide8_slots(), grid_min=np.array(d.wide8_grid_min[:], np.float32),
                grid_cell=np.array(d.wide8_grid_cell[:], np.float32))
    held.update({name: pool(scene, name) for name in capi.VERTEX_ATTRIBUTES})
    return held


def run_kernel_bodies(scene, held, pool_edits):
    """The host build of the passes over `held` (an arrays_of dict, in place); the indices, instances, materials and textures come from `scene`, which a vertex edit
    leaves alone. Returns dict(needs_rebuild, all_opaque, decided, changed, moved, half_area)."""
    d = scene.desc
    array, keep = capi.vertex_edits(pool_edits)
    out, area = np.zeros(4, np.uint32), np.zeros(1, np.float64)
    pointer = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    address = lambda p: C.cast(p, C.c_void_p)
    status = library().vertex_update_host_scene(pointer(held["triangles"]), len(held["triangles"]), address(d.instances), d.instance_count, address(d.materials), address(d.indices),
                                                pointer(held["geometry"]), pointer(held["texcoords"]), pointer(held["tints"]), pointer(held["emissions"]), d.vertex_count, address(d.textures),
                                                d.texture_count, address(d.texels), array, len(pool_edits), pointer(held["trace"]), pointer(held["shade"]), pointer(held["classes"]),
                                                pointer(held["slots"]), len(held["slots"]), pointer(held["grid_min"]), pointer(held["grid_cell"]), pointer(area), pointer(out))
    assert status >= 0
    return dict(needs_rebuild=bool(status), all_opaque=bool(out[0]), decided=int(out[1]), changed=int(out[2]), moved=int(out[3]), half_area=float(area[0]))


def plan_of(pool_edits):
    """The disjoint segments the host makes of an edit list: rows of (first word, pool, destination word), and the word count."""
    array, keep = capi.vertex_edits(pool_edits)
    out, words = np.zeros((64, 3), np.uint64), np.zeros(1, np.uint64)
    count = library().vertex_update_host_plan(array, len(pool_edits), C.c_void_p(out.ctypes.data), len(out), C.c_void_p(words.ctypes.data))
    assert count <= len(out)
    return out[:count], int(words[0])
