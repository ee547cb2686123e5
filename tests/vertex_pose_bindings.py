"""What the tests of hipr_set_scene_rigs / hipr_pose_scene_rigs share (csrc/vertex_pose.h, SceneBuilder::set_rigs / pose_rigs): the rigs, made procedurally over
meshes of vertex_update_bindings.make_scene() -- a bending tube (the lace's 17 x 17 grid rolled up, skinned to joints along its length), a flag (the lace as it is,
with morph targets), the box worn by two models and a mirrored third, the seam quad, the first and the last mesh of the pool -- the poses of the cases, and ctypes
access to the host build of the pose kernel's body (tests/native/VertexPoseHost.hip). Test infrastructure: built by bifrost3d_amd/Makefile, loaded by tests only.

The yardstick of every case is SceneBuilder: pose_rigs on the built scene, posed_geometry, and stage_rig_poses with the catch-up."""
import ctypes as C
from pathlib import Path

import numpy as np

import pool_growth_bindings as pg
import vertex_update_bindings as vu
from bifrost3d_amd import capi

GEOMETRY = vu.GEOMETRY
CELLS = vu.LACE_CELLS      # the lace: (CELLS + 1)^2 = 289 vertices, vertex j * 17 + i
RANGES = (1, 63, 64, 65, 257)


# ---- meshes ----
def tube_mesh():
    """The lace's grid rolled into a tube around y: column i at the angle 2 pi (i mod 16) / 16 -- the last column lies on the first, bit for bit -- row j at the
    height j / 16 - 0.5. Normals radial. No negative zero among the coordinates (an identity pose must give the rest position back bit for bit)."""
    lace = vu.mesh_data()["lace"]
    i, j = np.meshgrid(np.arange(CELLS + 1), np.arange(CELLS + 1))
    angle = 2.0 * np.pi * (i.reshape(-1) % CELLS) / CELLS
    radial = np.stack([np.cos(angle), np.zeros_like(angle), np.sin(angle)], axis=1)
    positions = (0.2 * radial + np.stack([np.zeros_like(angle), j.reshape(-1) / CELLS - 0.5, np.zeros_like(angle)], axis=1)).astype(np.float32) + np.float32(0.0)
    return dict(lace, positions=positions, normals=radial.astype(np.float32) + np.float32(0.0))


def make_scene(tube=False, loose_without_normals=False):
    """vertex_update_bindings' scene; tube: the lace rolled up; loose_without_normals: the quad with spare vertices loses its normals."""
    meshes = {}
    if tube:
        meshes["lace"] = tube_mesh()
    if loose_without_normals:
        meshes["loose"] = {k: v for k, v in vu.mesh_data()["loose"].items() if k != "normals"}
    return vu.make_scene(meshes)


# ---- matrices ----
def matrix(axis=(0.0, 0.0, 1.0), angle=0.0, translation=(0.0, 0.0, 0.0), scale=1.0, pivot=(0.0, 0.0, 0.0)):
    """A 3 x 4 float32 matrix: rotation by `angle` about `axis` through `pivot`, scaled, then translated."""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = scale * (np.eye(3) + np.sin(angle) * k + (1.0 - np.cos(angle)) * k @ k)
    pivot = np.asarray(pivot, np.float64)
    return np.concatenate([r, (pivot - r @ pivot + np.asarray(translation, np.float64))[:, None]], axis=1).astype(np.float32)


IDENTITY = matrix()
ZERO = np.zeros((3, 4), np.float32)


# ---- rigs: dicts as capi.rig_descs takes them, with `mesh` and a MESH-relative `first` ----
def of_mesh(info, name, first, count):
    data = info["data"][name]
    rig = dict(mesh=info["mesh"][name], first=first, rest_positions=data["positions"][first:first + count].copy())
    if data.get("normals") is not None:
        rig["rest_normals"] = data["normals"][first:first + count].copy()
    return rig


def tube_rig(info, first, count, joints=2, spare_joint=None):
    """Vertices [first, first + count) of the tube skinned along its length: joint 0 holds the bottom, joint 1 the top, the weights follow the height -- a vertex of
    the bottom row names joint 1 with weight 0, one of the top row joint 0 -- slots 2 and 3 have weight 0 and name `spare_joint` (default: the last joint)."""
    rig = of_mesh(info, "lace", first, count)
    top = (rig["rest_positions"][:, 1] + np.float32(0.5)).astype(np.float32) if joints > 1 else np.zeros(count, np.float32)
    spare = joints - 1 if spare_joint is None else spare_joint
    rig["joints"] = np.tile(np.array([0, min(1, joints - 1), spare, spare], np.uint16), (count, 1))
    rig["weights"] = np.stack([np.float32(1.0) - top, top, np.zeros(count, np.float32), np.zeros(count, np.float32)], axis=1).astype(np.float32)
    rig["joint_count"] = joints
    return rig


def many_joint_rig(info, first, count, joints):
    """The tube with `joints` joints (above the kernel's LDS budget): vertex v is held by joints spread over the whole list, the last one included."""
    rig = of_mesh(info, "lace", first, count)
    v = np.arange(count)
    rig["joints"] = np.stack([(v * 4) % joints, np.full(count, joints - 1), (v * 7 + 1) % joints, np.zeros(count, int)], axis=1).astype(np.uint16)
    rig["weights"] = np.tile(np.array([0.5, 0.25, 0.25, 0.0], np.float32), (count, 1))
    rig["joint_count"] = joints
    return rig


def box_rig(info, name="box"):
    """All eight vertices of the box, all four slots used."""
    rig = of_mesh(info, name, 0, 8)
    rig["joints"] = np.tile(np.array([0, 1, 2, 3], np.uint16), (8, 1))
    rig["weights"] = np.tile(np.array([0.4, 0.3, 0.2, 0.1], np.float32), (8, 1))
    rig["joint_count"] = 4
    return rig


def flag_rig(info, first, count, targets, target_normals=False, joints=0, seed=1):
    """Vertices [first, first + count) of the flat lace with `targets` morph targets: ripples along z, seeded; target_normals: tilts of the normals with them."""
    rig = of_mesh(info, "lace", first, count)
    rng = np.random.default_rng(seed)
    if targets:
        rig["target_positions"] = (rng.uniform(-0.05, 0.05, (targets, count, 3)) * np.array([0.1, 0.1, 1.0])).astype(np.float32)
        if target_normals:
            rig["target_normals"] = rng.uniform(-0.3, 0.3, (targets, count, 3)).astype(np.float32)
    if joints:
        rig["joints"] = np.tile(np.array([0, joints - 1, 0, 0], np.uint16), (count, 1))
        rig["weights"] = np.tile(np.array([0.75, 0.25, 0.0, 0.0], np.float32), (count, 1))
        rig["joint_count"] = joints
    return rig


def bend(joints, angle=0.6, seed=0):
    """Matrices of a bend: joint 0 stays, the others turn about z through the tube's middle by `angle` and more, each a little shifted."""
    return np.stack([IDENTITY] + [matrix(angle=angle * (1.0 + 0.01 * k), translation=(0.01 * ((k * 7 + seed) % 5), 0.02, 0.0)) for k in range(1, joints)])[:joints]


def box_pose(seed):
    rng = np.random.default_rng(seed)
    return np.stack([matrix(axis=rng.uniform(-1, 1, 3), angle=rng.uniform(-0.5, 0.5), translation=rng.uniform(-0.1, 0.1, 3), scale=rng.uniform(0.8, 1.2)) for _ in range(4)])


# ---- the cases: name -> (make_scene's arguments, function of (scene, info) returning (rigs, steps)); a step = the poses of one call ----
def _tube(count):
    joints = 1 if count == 1 else 2
    return lambda scene, info: ([tube_rig(info, 3, count, joints)], [[dict(rig=0, matrices=bend(joints) if joints > 1 else np.stack([matrix(angle=0.3, translation=(0.0, 0.05, 0.0))]))]])


def _first_and_last(scene, info):
    wall = dict(mesh=0, first=0, rest_positions=vu.of_mesh(scene, 0, "geometry")["position"][:2].copy(), rest_normals=np.tile(np.array([0.0, 1.0, 0.0], np.float32), (2, 1)),
                joints=np.zeros((2, 4), np.uint16), weights=np.tile(np.array([1.0, 0.0, 0.0, 0.0], np.float32), (2, 1)), joint_count=1)
    last = of_mesh(info, "glowing", 6, 2)
    last.update(joints=np.zeros((2, 4), np.uint16), weights=np.tile(np.array([0.5, 0.5, 0.0, 0.0], np.float32), (2, 1)), joint_count=1)
    return [wall, last], [[dict(rig=1, matrices=np.stack([matrix(translation=(0.02, 0.03, -0.01))])), dict(rig=0, matrices=np.stack([matrix(translation=(0.0, 0.004, 0.0))]))]]


def _collapse(scene, info):
    return [tube_rig(info, 0, 289, 2)], [[dict(rig=0, matrices=np.stack([IDENTITY, ZERO]))]]


def _grow_and_shrink(scene, info):
    far = np.stack([matrix(translation=(0.0, -9.0, 0.0))] * 4)
    back = np.stack([matrix(translation=(0.0, -0.05, 0.0))] * 4)
    return [box_rig(info)], [[dict(rig=0, matrices=far)], [dict(rig=0, matrices=back)]]


CASES = {
    **{f"tube_{n}": (dict(tube=True), _tube(n)) for n in RANGES},
    "first_and_last_vertex_of_the_pool_two_rigs_in_one_call": (dict(), _first_and_last),
    "box_worn_by_two_and_a_mirrored_twin_all_four_slots": (dict(), lambda scene, info: ([box_rig(info)], [[dict(rig=0, matrices=box_pose(3))]])),
    "joints_above_the_lds_budget": (dict(tube=True), lambda scene, info: ([many_joint_rig(info, 100, 65, lds_joints() + 1)], [[dict(rig=0, matrices=bend(lds_joints() + 1, 0.002))]])),
    "flag_1_target": (dict(), lambda scene, info: ([flag_rig(info, 0, 289, 1)], [[dict(rig=0, weights=[0.75])]])),
    "flag_1_target_with_normals": (dict(), lambda scene, info: ([flag_rig(info, 5, 65, 1, True, seed=4)], [[dict(rig=0, weights=[-1.25])]])),
    "flag_3_targets": (dict(), lambda scene, info: ([flag_rig(info, 0, 257, 3, seed=5)], [[dict(rig=0, weights=[0.5, 1.5, -0.25])]])),
    "flag_3_targets_with_normals_one_skipped": (dict(), lambda scene, info: ([flag_rig(info, 20, 200, 3, True)], [[dict(rig=0, weights=[1.0, 0.0, -0.5])]])),
    "flag_targets_and_joints_beside_a_tube_free_rig": (dict(), lambda scene, info: ([flag_rig(info, 0, 100, 2, True, joints=2), flag_rig(info, 100, 189, 1, seed=2)],
                                                                                   [[dict(rig=0, matrices=bend(2, 0.2), weights=[0.5, 0.25]), dict(rig=1, weights=[1.0])]])),
    "mesh_without_normals": (dict(loose_without_normals=True), lambda scene, info: ([dict(of_mesh(info, "loose", 0, 7), target_positions=np.full((1, 7, 3), 0.01, np.float32))], [[dict(rig=0, weights=[2.0])]])),
    "zero_matrix_collapses_a_limb": (dict(tube=True), _collapse),
    "bounds_grow_and_shrink_back": (dict(), _grow_and_shrink),
}
CASE_IDS = list(CASES)


def case(name):
    """(scene, info, rigs, steps) of a case, the rigs bound in the builder."""
    arguments, make = CASES[name]
    scene, info = make_scene(**arguments)
    rigs, steps = make(scene, info)
    assert scene.set_rigs(rigs) is True, name
    return scene, info, rigs, steps


def moved_count(scene, rigs, poses):
    """Triangles that read a vertex of a posed rig, from the builder's arrays."""
    marks = np.zeros(scene.desc.vertex_count, bool)
    for p in poses:
        r = scene.pooled_rigs([rigs[p["rig"]]])[0]
        marks[r["first"]:r["first"] + len(r["rest_positions"])] = True
    return int(vu.corners_marked(scene, marks).sum())


def as_vertex_edits(scene, rigs, poses):
    """The poses as POOL-coordinate geometry edits of hipr_update_scene_vertices, through Scene.posed_geometry."""
    return [dict(first=scene.pooled_rigs([rigs[p["rig"]]])[0]["first"], geometry=scene.posed_geometry(rigs[p["rig"]], p)) for p in poses]


# ---- the host build of the pose kernel's body (tests/native/VertexPoseHost.hip) ----
LIB_PATH = Path(__file__).resolve().parent / "native" / "libvertex_pose_host.so"
_lib = None


def library():
    global _lib
    if _lib is None:
        assert LIB_PATH.exists(), f"{LIB_PATH} is missing: run __graft_entry__.build()"
        _lib = C.CDLL(str(LIB_PATH))
        vp, u32 = C.c_void_p, C.c_uint32
        _lib.vertex_pose_host_walk.argtypes = [C.POINTER(capi.HiprRigDesc), u32, C.POINTER(capi.HiprRigPose), u32, u32, vp, vp, u32]
        _lib.vertex_pose_host_walk.restype = C.c_longlong
        _lib.vertex_pose_host_encode.argtypes = [vp, u32, vp]
        _lib.vertex_pose_host_roundings.argtypes = [u32]
        _lib.vertex_pose_host_roundings.restype = u32
        _lib.vertex_pose_host_lds_joints.restype = u32
        _lib.vertex_pose_host_lds_capacity.restype = u32
    return _lib


def lds_joints():
    """The LDS budget in joints that ships."""
    return int(library().vertex_pose_host_lds_joints())


def lds_capacity():
    """The joints the kernel's LDS array holds: the largest budget that can be set."""
    return int(library().vertex_pose_host_lds_capacity())


def walk(geometry, pooled_rigs, poses, budget=None):
    """The kernel's walk over a copy of the geometry pool (records): returns (the pool afterwards, the marks, the vertices posed -- negative: refused)."""
    geometry = np.ascontiguousarray(geometry).copy()
    marks = np.zeros(len(geometry), np.uint8)
    rigs, keep_rigs = capi.rig_descs(pooled_rigs)
    array, keep_poses = capi.rig_poses(poses)
    posed = library().vertex_pose_host_walk(rigs, len(pooled_rigs), array, len(poses), lds_joints() if budget is None else budget, C.c_void_p(geometry.ctypes.data), C.c_void_p(marks.ctypes.data), len(geometry))
    return geometry, marks, int(posed)


def encode(normals):
    """The header's restatement of encode_precise on (n, 3) float32 normals: (n, 2) int16."""
    normals = np.ascontiguousarray(normals, np.float32)
    out = np.zeros((len(normals), 2), np.int16)
    library().vertex_pose_host_encode(C.c_void_p(normals.ctypes.data), len(normals), C.c_void_p(out.ctypes.data))
    return out
