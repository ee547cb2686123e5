"""ctypes mirror of include/hiprenderer_c.h and loader for the C-ABI shared library.

Python here is plumbing for tests, bench.py and the multi-GPU driver only: it holds no
rendering logic. The library must have been built (``__graft_entry__.build()``); loading
fails loudly otherwise -- there is no CPU fallback for the product path.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("HIPR_LIBRARY", PKG_DIR / "csrc" / "libhiprenderer.so"))   # HIPR_LIBRARY: A/B builds of the kernels
HIPR_ARITHMETIC_FAST, HIPR_ARITHMETIC_EXACT = 0, 1      # hipr_set_arithmetic: the two builds of the shade unit inside the library
HOST_LIB_PATH = Path(os.environ.get("HIPR_HOST_LIBRARY", PKG_DIR / "host" / "libhiprenderer_host.so"))   # HIPR_HOST_LIBRARY: A/B builds of the host side (BVH builder)
TABLES_PATH = PKG_DIR / "data" / "HIPRenderer" / "shading_tables.bin"

HIPR_OK = 0

c_f = C.c_float
c_u32 = C.c_uint32
c_i32 = C.c_int32
c_u16 = C.c_uint16
c_u8 = C.c_uint8
c_u64 = C.c_uint64


class HiprMaterial(C.Structure):
    _fields_ = [("flags", c_u16), ("shading_model", c_u16), ("tint", c_f * 3),
                ("roughness", c_f), ("tint_roughness_texture_ID", c_i32), ("roughness_texture_ID", c_i32), ("specularity", c_f),
                ("metallic", c_f), ("metallic_texture_ID", c_i32), ("coverage", c_f), ("coverage_texture_ID", c_i32),
                ("emission", c_f * 3), ("coat", c_u16), ("coat_roughness", c_u16)]


class HiprLight(C.Structure):
    _fields_ = [("data", c_f * 11), ("flags", c_u32)]


class HiprVertexGeometry(C.Structure):
    _fields_ = [("position", c_f * 3), ("oct_normal", C.c_int16 * 2)]


class HiprInstance(C.Structure):
    _fields_ = [("object_to_world", c_f * 12), ("index_offset", c_u32), ("vertex_offset", c_u32),
                ("instance_id", c_i32), ("material_index", c_i32), ("mesh_flags", c_u32), ("_pad", c_u32 * 3)]


class HiprTriangle(C.Structure):
    _fields_ = [("v0", c_f * 3), ("v1", c_f * 3), ("v2", c_f * 3),
                ("instance_index", c_u32), ("primitive_index", c_u32), ("flags", c_u32)]


class HiprBvhNode(C.Structure):
    _fields_ = [("c0xy", c_f * 4), ("c1xy", c_f * 4), ("cz", c_f * 4), ("child", c_i32 * 2), ("_pad", c_u32 * 2)]


class HiprTexture(C.Structure):
    _fields_ = [("width", c_u32), ("height", c_u32), ("texel_offset", c_u64), ("format", c_u8),
                ("wrap_u", c_u8), ("wrap_v", c_u8), ("filter", c_u8), ("is_sRGB", c_u8), ("_pad", c_u8 * 3)]


class HiprWideNode(C.Structure):
    _fields_ = [("origin", c_f * 3), ("exponents", c_u32), ("qlo", c_u32 * 3), ("qhi", c_u32 * 3), ("_pad", c_u32 * 2), ("child", c_i32 * 4)]


class HiprLightSample(C.Structure):
    _fields_ = [("radiance", c_f * 3), ("PDF", c_f), ("direction_to_light", c_f * 3), ("distance", c_f)]


class HiprEnvironment(C.Structure):
    _fields_ = [("environment_map_ID", c_i32), ("pdf_width", c_u32), ("pdf_height", c_u32), ("per_pixel_PDF", C.POINTER(c_f)),
                ("samples", C.POINTER(HiprLightSample)), ("sample_count", c_u32)]


class HiprSceneDesc(C.Structure):
    _fields_ = [("nodes", C.POINTER(HiprBvhNode)), ("node_count", c_u32),
                ("triangles", C.POINTER(HiprTriangle)), ("triangle_count", c_u32),
                ("instances", C.POINTER(HiprInstance)), ("instance_count", c_u32),
                ("indices", C.POINTER(c_u32)), ("index_count", c_u32),
                ("geometry", C.POINTER(HiprVertexGeometry)), ("vertex_count", c_u32),
                ("texcoords", C.POINTER(c_f)), ("tints", C.POINTER(c_u32)), ("emissions", C.POINTER(c_f)),
                ("materials", C.POINTER(HiprMaterial)), ("material_count", c_u32),
                ("lights", C.POINTER(HiprLight)), ("light_count", c_u32),
                ("textures", C.POINTER(HiprTexture)), ("texture_count", c_u32),
                ("texels", C.POINTER(c_u8)), ("texel_bytes", c_u64),
                ("bvh_max_depth", c_u32),
                ("wide_nodes", C.POINTER(HiprWideNode)), ("wide_node_count", c_u32), ("wide_stack_entries", c_u32),
                ("environment", C.POINTER(HiprEnvironment)),
                ("wide8_slots", C.POINTER(c_u32 * 16)), ("wide8_slot_count", c_u32), ("wide8_height", c_u32),
                ("wide8_grid_min", c_f * 3), ("wide8_grid_cell", c_f * 3)]


class HiprSceneState(C.Structure):
    _fields_ = [("environment_tint", c_f * 3), ("next_event_sample_count", c_i32)]


class HiprCameraState(C.Structure):
    _fields_ = [("view_to_world_rotation", c_f * 9), ("inverse_projection_matrix", c_f * 16),
                ("inverse_view_projection_matrix", c_f * 16), ("accumulations", c_u32),
                ("max_bounce_count", c_u32), ("path_regularization_PDF_scale", c_f), ("path_regularization_scale_decay", c_f)]


class HiprTables(C.Structure):
    _fields_ = [("ggx_with_fresnel_rho", C.POINTER(c_f)), ("ggx_rho", C.POINTER(c_f)),
                ("dielectric_light_rho", C.POINTER(c_f)), ("dielectric_dense_rho", C.POINTER(c_f)),
                ("ggx_alpha_from_max_PDF", C.POINTER(c_f))]


class HiprFrameDesc(C.Structure):
    _fields_ = [("width", c_u32), ("height", c_u32), ("tile_phase", c_u32), ("tile_stride", c_u32), ("samples_per_pass", c_u32)]


class HiprCounters(C.Structure):
    _fields_ = [("camera_rays", c_u64), ("closest_rays", c_u64), ("shadow_rays", c_u64), ("shaded_hits", c_u64),
                ("closest_nodes", c_u64), ("closest_triangles", c_u64), ("shadow_nodes", c_u64), ("shadow_triangles", c_u64),
                ("iterations", c_u64)]


class HiprInstanceTransform(C.Structure):
    _fields_ = [("instance_index", c_u32), ("object_to_world", c_f * 12)]


class HiprWide8BuildResult(C.Structure):
    _fields_ = [("slot_count", c_u32), ("height", c_u32), ("grid_min", c_f * 3), ("grid_cell", c_f * 3), ("node_count", c_u32), ("leaf_count", c_u32), ("paired_leaves", c_u32)]


class HiprWide4BuildResult(C.Structure):
    _fields_ = [("node_count", c_u32), ("stack_entries", c_u32)]


class HiprSceneRebuildResult(C.Structure):
    _fields_ = [("node_count", c_u32), ("deepest", c_u32), ("wide8", HiprWide8BuildResult), ("half_area", C.c_double)]


EDIT_NEW_INSTANCE = 0xFFFFFFFF


class HiprInstanceEdit(C.Structure):
    _fields_ = [("source", c_u32), ("primitive_count", c_u32), ("instance", HiprInstance)]


class HiprSceneEditResult(C.Structure):
    _fields_ = [("triangle_count", c_u32), ("instance_count", c_u32), ("node_count", c_u32), ("deepest", c_u32), ("wide8", HiprWide8BuildResult), ("_pad", c_u32), ("half_area", C.c_double)]


SEGMENT_FROM_HOST = 0xFFFFFFFF


class HiprIndexSegment(C.Structure):
    _fields_ = [("mirrored_from", c_u32), ("index_count", c_u32)]


class HiprPoolGrowth(C.Structure):
    _fields_ = [("geometry", C.POINTER(HiprVertexGeometry)), ("texcoords", C.POINTER(c_f)), ("tints", C.POINTER(c_u32)), ("emissions", C.POINTER(c_f)), ("indices", C.POINTER(c_u32)),
                ("segments", C.POINTER(HiprIndexSegment)), ("materials", C.POINTER(HiprMaterial)), ("textures", C.POINTER(HiprTexture)), ("texels", C.POINTER(c_u8)), ("texel_bytes", c_u64),
                ("vertex_count", c_u32), ("texcoord_vertices", c_u32), ("tint_vertices", c_u32), ("emission_vertices", c_u32),
                ("index_count", c_u32), ("segment_count", c_u32), ("material_count", c_u32), ("texture_count", c_u32)]


class HiprEnvironmentBuild(C.Structure):
    _fields_ = [("environment_map_ID", c_i32), ("row_sines", C.POINTER(c_f)), ("pdf_height", c_u32), ("srgb_decode", C.POINTER(c_f)), ("draw_points", C.POINTER(c_f)), ("sample_count", c_u32)]


class HiprLightingResult(C.Structure):
    _fields_ = [("pdf_width", c_u32), ("pdf_height", c_u32), ("sample_count", c_u32), ("importance_sampling_disabled", c_u32), ("light_count", c_u32), ("switches", c_u32)]


ENVIRONMENT_KEEP, ENVIRONMENT_REMOVE, ENVIRONMENT_BUILD = 0, 1, 2
SWITCH_TEXTURES, SWITCH_ENVIRONMENT = 1, 2
LIGHT_NONE, LIGHT_SPHERE, LIGHT_DIRECTIONAL, LIGHT_ENVIRONMENT, LIGHT_PRESAMPLED_ENVIRONMENT, LIGHT_SPOT, LIGHT_TYPE_MASK = 0, 1, 2, 3, 4, 5, 7


class HiprTexelEdit(C.Structure):
    _fields_ = [("texture_index", c_u32), ("x", c_u32), ("y", c_u32), ("width", c_u32), ("height", c_u32), ("texels", C.c_void_p), ("row_pitch_bytes", c_u64)]


class HiprTexelUpdateResult(C.Structure):
    _fields_ = [("candidate_triangles", c_u32), ("changed_triangles", c_u32), ("all_triangles_opaque", c_u32), ("environment_stale", c_u32)]


def texel_edits(edits):
    """(texture index, x, y, pixels) tuples -- `pixels` a C-contiguous array of (height, width[, channels]) texels in the texture's resident format, or
    (texture index, x, y, width, height, pixels, row pitch in bytes) with the rows of `pixels` a pitch apart -- as the HiprTexelEdit array of hipr_update_scene_texels
    (one spare element: never a null array). Returns (array, keep-alive): the array points into the arrays of keep-alive."""
    import numpy as np
    edits = list(edits)
    array, keep = (HiprTexelEdit * max(len(edits), 1))(), []
    for k, edit in enumerate(edits):
        if len(edit) == 4:
            texture, x, y, pixels = edit
            pixels = np.ascontiguousarray(pixels)
            height, width, pitch = pixels.shape[0], pixels.shape[1], pixels.strides[0]
        else:
            texture, x, y, width, height, pixels, pitch = edit
            pixels = np.ascontiguousarray(pixels) if pixels is not None else None
        keep.append(pixels)
        array[k] = HiprTexelEdit(int(texture), int(x), int(y), int(width), int(height), pixels.ctypes.data if pixels is not None else None, int(pitch))
    return array, keep


class HiprRefitResult(C.Structure):
    _fields_ = [("needs_rebuild", c_i32), ("child_half_area", C.c_double), ("uploaded_half_area", C.c_double), ("grid_min", c_f * 3), ("grid_cell", c_f * 3)]


class HiprMaterialUpdate(C.Structure):
    _fields_ = [("material_index", c_u32), ("material", HiprMaterial)]


class HiprInstanceMaterial(C.Structure):
    _fields_ = [("instance_index", c_u32), ("material_index", c_i32)]


def material_updates(materials):
    """(material index, HiprMaterial) pairs as the HiprMaterialUpdate array of hipr_update_scene_materials (one spare element: never a null array)."""
    materials = list(materials)
    array = (HiprMaterialUpdate * max(len(materials), 1))()
    for k, (index, material) in enumerate(materials):
        array[k].material_index = int(index)
        C.memmove(C.byref(array[k].material), C.byref(material), C.sizeof(HiprMaterial))
    return array


def instance_materials(assignments):
    """(instance index, material index) pairs as the HiprInstanceMaterial array of hipr_update_scene_materials."""
    assignments = list(assignments)
    array = (HiprInstanceMaterial * max(len(assignments), 1))()
    for k, (instance, material) in enumerate(assignments):
        array[k].instance_index = int(instance)
        array[k].material_index = int(material)
    return array


HIPR_ERROR_INVALID_ARGUMENT, HIPR_ERROR_NOT_READY, HIPR_ERROR_UNSUPPORTED = -1, -5, -6
SCENE_BUFFER_TRIANGLES, SCENE_BUFFER_WIDE8_SLOTS, SCENE_BUFFER_TRACE_TRIANGLES, SCENE_BUFFER_SHADE_TRIANGLES, SCENE_BUFFER_TRIANGLE_CLASS, SCENE_BUFFER_MATERIALS, SCENE_BUFFER_INSTANCES = 0, 1, 2, 3, 4, 5, 6
SCENE_BUFFER_NODES = 7      # the BVH2; not among SCENE_BUFFERS, which lists what every writer of the resident scene is held to
TEXEL_R8, TEXEL_RGBA8, TEXEL_R32F, TEXEL_RGBA32F = 1, 4, 17, 20
# the pools hipr_append_scene_pools grows; not among SCENE_BUFFERS either: tests of the growth keep a tuple of their own
SCENE_BUFFER_INDICES, SCENE_BUFFER_GEOMETRY, SCENE_BUFFER_TEXCOORDS, SCENE_BUFFER_TINTS, SCENE_BUFFER_EMISSIONS, SCENE_BUFFER_TEXTURES, SCENE_BUFFER_TEXELS = 8, 9, 10, 11, 12, 13, 14
# what hipr_update_scene_lighting writes: the lights, the environment's PDF image and its samples
SCENE_BUFFER_LIGHTS, SCENE_BUFFER_ENVIRONMENT_PDF, SCENE_BUFFER_ENVIRONMENT_SAMPLES = 15, 16, 17
SCENE_BUFFERS = (SCENE_BUFFER_TRIANGLES, SCENE_BUFFER_WIDE8_SLOTS, SCENE_BUFFER_TRACE_TRIANGLES, SCENE_BUFFER_SHADE_TRIANGLES, SCENE_BUFFER_TRIANGLE_CLASS, SCENE_BUFFER_MATERIALS, SCENE_BUFFER_INSTANCES)
TRACE_BVH2, TRACE_WIDE_PERSISTENT, TRACE_EXHAUSTIVE, TRACE_WIDE8_PERSISTENT = 0, 1, 2, 3
SHADING_DEFAULT, SHADING_DIFFUSE, SHADING_TRANSMISSIVE = 0, 1, 2
MATERIAL_THIN_WALLED, MATERIAL_CUTOUT = 1, 2
TRIANGLE_OPAQUE, TRIANGLE_ONE_SIDED = 1, 4
ENTRY_PATH_TRACING, ENTRY_DEPTH, ENTRY_ALBEDO, ENTRY_TINT, ENTRY_ROUGHNESS, ENTRY_SHADING_NORMAL, ENTRY_PRIMITIVE_ID, ENTRY_DENOISER_ALBEDO = 0, 3, 4, 5, 6, 7, 8, 9
HIPR_KERNEL_NAMES = ("generate", "trace_closest", "shade", "trace_shadow", "accumulate")


class HiprKernelTimes(C.Structure):
    _fields_ = [("milliseconds", C.c_double * 5), ("launches", c_u64 * 5)]


assert C.sizeof(HiprMaterial) == 64 and C.sizeof(HiprLight) == 48 and C.sizeof(HiprVertexGeometry) == 16
assert C.sizeof(HiprTexture) == 24 and C.sizeof(HiprCameraState) == 180 and C.sizeof(HiprTriangle) == 48 and C.sizeof(HiprBvhNode) == 64 and C.sizeof(HiprInstance) == 80
assert C.sizeof(HiprInstanceEdit) == 88 and C.sizeof(HiprSceneEditResult) == 72
assert C.sizeof(HiprIndexSegment) == 8 and C.sizeof(HiprPoolGrowth) == 112
assert C.sizeof(HiprEnvironmentBuild) == 48 and C.sizeof(HiprLightingResult) == 24 and C.sizeof(HiprLightSample) == 32
assert C.sizeof(HiprTexelEdit) == 40 and C.sizeof(HiprTexelUpdateResult) == 16


class HiprVertexEdit(C.Structure):
    _fields_ = [("first_vertex", c_u32), ("vertex_count", c_u32), ("geometry", C.c_void_p), ("texcoords", C.c_void_p), ("tints", C.c_void_p), ("emissions", C.c_void_p)]


class HiprVertexUpdateResult(C.Structure):
    _fields_ = [("refit", HiprRefitResult), ("moved_triangles", c_u32), ("candidate_triangles", c_u32), ("changed_triangles", c_u32), ("all_triangles_opaque", c_u32)]


assert C.sizeof(HiprVertexEdit) == 40 and C.sizeof(HiprVertexUpdateResult) == 64

VERTEX_ATTRIBUTES = ("geometry", "texcoords", "tints", "emissions")


def vertex_geometry_dtype():
    """HiprVertexGeometry as a numpy record: the position and the octahedral normal, 16 bytes."""
    import numpy as np
    return np.dtype([("position", "<f4", (3,)), ("oct_normal", "<i2", (2,))])


def vertex_edits(edits):
    """Dicts of `first` (a vertex of the RESIDENT pools) and any of `geometry` (records of vertex_geometry_dtype(), or raw (n, 4) words), `texcoords` (n, 2) float32,
    `tints` (n,) uint32 and `emissions` (n, 3) float32 -- `count` in place of the arrays' length for a call that is to be refused -- as the HiprVertexEdit array of
    hipr_update_scene_vertices (one spare element: never a null array). Returns (array, keep-alive): the array points into the arrays of keep-alive."""
    import numpy as np
    edits = list(edits)
    array, keep = (HiprVertexEdit * max(len(edits), 1))(), []
    kinds = dict(geometry=(None, 16), texcoords=(np.float32, 8), tints=(np.uint32, 4), emissions=(np.float32, 12))
    for k, edit in enumerate(edits):
        pointers, count = [], None
        for name in VERTEX_ATTRIBUTES:
            values = edit.get(name)
            if values is None:
                pointers.append(None)
                continue
            dtype, size = kinds[name]
            values = np.ascontiguousarray(values) if dtype is None else np.ascontiguousarray(values, dtype)
            assert values.nbytes % size == 0, name
            count = values.nbytes // size if count is None else count
            assert values.nbytes // size == count, "the arrays of one edit describe the same vertices"
            keep.append(values)
            pointers.append(values.ctypes.data)
        array[k] = HiprVertexEdit(int(edit["first"]), int(edit.get("count", count or 0)), *pointers)
    return array, keep or [None]


class HiprRigDesc(C.Structure):
    _fields_ = [("first_vertex", c_u32), ("vertex_count", c_u32), ("joint_count", c_u32), ("target_count", c_u32), ("rest_positions", C.c_void_p), ("rest_normals", C.c_void_p),
                ("joints", C.c_void_p), ("weights", C.c_void_p), ("target_positions", C.c_void_p), ("target_normals", C.c_void_p)]


class HiprRigPose(C.Structure):
    _fields_ = [("rig", c_u32), ("reserved", c_u32), ("joint_matrices", C.c_void_p), ("target_weights", C.c_void_p)]


assert C.sizeof(HiprRigDesc) == 64 and C.sizeof(HiprRigPose) == 24

RIG_ARRAYS = ("rest_positions", "rest_normals", "joints", "weights", "target_positions", "target_normals")


def rig_descs(rigs):
    """Dicts of `first` (a vertex of the RESIDENT pools; MESH-relative for Scene.set_rigs), `rest_positions` (n, 3) float32 and any of `rest_normals` (n, 3), `joints`
    (n, 4) uint16 with `weights` (n, 4) float32, `target_positions` (t, n, 3) float32 and `target_normals` (t, n, 3) as the HiprRigDesc array of hipr_set_scene_rigs
    (one spare element: never a null array). `joint_count` defaults to the largest index + 1, `target_count` to the targets given, `count` to the rest positions'
    length; each can be given for a call that is to be refused, and an array given as the string "null" stays a null pointer whatever the counts say. Returns
    (array, keep-alive)."""
    import numpy as np
    rigs = list(rigs)
    array, keep = (HiprRigDesc * max(len(rigs), 1))(), []
    kinds = dict(rest_positions=np.float32, rest_normals=np.float32, joints=np.uint16, weights=np.float32, target_positions=np.float32, target_normals=np.float32)
    for k, rig in enumerate(rigs):
        held = {}
        for name in RIG_ARRAYS:
            values = rig.get(name)
            if values is None or isinstance(values, str):
                held[name] = None
                continue
            held[name] = np.ascontiguousarray(values, kinds[name])
            keep.append(held[name])
        positions, joints, targets = held["rest_positions"], held["joints"], held["target_positions"]
        count = int(rig.get("count", 0 if positions is None else positions.size // 3))
        joint_count = int(rig.get("joint_count", 0 if joints is None or not joints.size else int(joints.max()) + 1))
        target_count = int(rig.get("target_count", 0 if targets is None or not count else targets.size // (3 * count)))
        array[k] = HiprRigDesc(int(rig["first"]), count, joint_count, target_count, *[None if held[name] is None else held[name].ctypes.data for name in RIG_ARRAYS])
    return array, keep or [None]


def rig_poses(poses):
    """Dicts of `rig` (an index into the bound set) and any of `matrices` (joint_count, 3, 4) float32 and `weights` (target_count,) float32 as the HiprRigPose array
    of hipr_pose_scene_rigs (one spare element). Returns (array, keep-alive)."""
    import numpy as np
    poses = list(poses)
    array, keep = (HiprRigPose * max(len(poses), 1))(), []
    for k, pose in enumerate(poses):
        pointers = []
        for name in ("matrices", "weights"):
            values = pose.get(name)
            if values is None:
                pointers.append(None)
                continue
            values = np.ascontiguousarray(values, np.float32)
            keep.append(values)
            pointers.append(values.ctypes.data)
        array[k] = HiprRigPose(int(pose["rig"]), 0, *pointers)
    return array, keep or [None]

# Every symbol include/hiprenderer_c.h declares; tests check the library exports all of them.
C_ABI_SYMBOLS = (
    "hipr_create", "hipr_destroy", "hipr_last_error", "hipr_device_count", "hipr_set_stream",
    "hipr_upload_tables", "hipr_upload_scene", "hipr_validate_scene", "hipr_update_scene_geometry", "hipr_group_update_scene_geometry", "hipr_refit_scene_transforms", "hipr_group_refit_scene_transforms", "hipr_update_scene_materials", "hipr_group_update_scene_materials", "hipr_build_bvh2", "hipr_group_build_bvh2", "hipr_debug_build_times", "hipr_build_wide8", "hipr_group_build_wide8", "hipr_debug_collapse_times", "hipr_build_wide4", "hipr_group_build_wide4", "hipr_debug_collapse4_times", "hipr_rebuild_scene_trees", "hipr_group_rebuild_scene_trees", "hipr_edit_scene_instances", "hipr_group_edit_scene_instances", "hipr_append_scene_pools", "hipr_group_append_scene_pools", "hipr_update_scene_lighting", "hipr_group_update_scene_lighting", "hipr_debug_lighting_times", "hipr_update_scene_texels", "hipr_group_update_scene_texels", "hipr_debug_texel_update_times", "hipr_update_scene_vertices", "hipr_group_update_scene_vertices", "hipr_debug_vertex_update_times", "hipr_set_scene_rigs", "hipr_group_set_scene_rigs", "hipr_pose_scene_rigs", "hipr_group_pose_scene_rigs", "hipr_debug_vertex_pose_times", "hipr_debug_set_pose_lds_joints", "hipr_debug_scene_buffer_bytes", "hipr_debug_append_times", "hipr_debug_rebuild_times", "hipr_debug_read_scene_buffer", "hipr_set_scene_state", "hipr_set_entry_point", "hipr_use_scratch_accumulation",
    "hipr_set_frame", "hipr_owned_pixel_count",
    "hipr_render_pass", "hipr_set_samples_per_pass", "hipr_trace_pass", "hipr_accumulate_samples", "hipr_read_accumulation", "hipr_scatter_tiles", "hipr_synchronize", "hipr_get_counters",
    "hipr_device_malloc", "hipr_device_free", "hipr_device_memset", "hipr_copy_to_host", "hipr_present_flipped",
    "hipr_reset_counters", "hipr_set_wavefront_count", "hipr_get_wavefront_count", "hipr_get_trace_variant", "hipr_set_trace_variant", "hipr_set_pass_pipelining", "hipr_set_backface_culling", "hipr_set_arithmetic", "hipr_get_arithmetic", "hipr_set_instrumentation", "hipr_reset_timers", "hipr_get_kernel_times",
    "hipr_group_create", "hipr_group_destroy", "hipr_group_size", "hipr_group_context", "hipr_group_gather_description", "hipr_group_upload_tables", "hipr_group_upload_scene",
    "hipr_group_set_scene_state", "hipr_group_set_entry_point", "hipr_group_use_scratch_accumulation", "hipr_group_set_frame", "hipr_group_set_samples_per_pass",
    "hipr_group_trace_pass", "hipr_group_accumulate_samples", "hipr_group_read_accumulation", "hipr_group_get_counters",
    "hipr_debug_shading", "hipr_debug_shade", "hipr_debug_light", "hipr_debug_math", "hipr_debug_generate", "hipr_debug_sobol", "hipr_debug_valu_issue_rates", "hipr_debug_sample_offsets", "hipr_debug_trace_closest", "hipr_debug_trace_shadow", "hipr_debug_trace_fused", "hipr_debug_trace_hinted", "hipr_debug_classify_hits",
)


class HiprError(RuntimeError):
    pass


_lib = None


def load_library(path: os.PathLike | None = None) -> C.CDLL:
    """Loads libhiprenderer.so. Raises (never falls back) when the HIP extension is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else LIB_PATH
    if not p.exists():
        raise HiprError(f"{p} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()')")
    try:
        # PyTorch-ROCm bundles its own libamdhip64; a process that loads the system runtime first and torch second
        # ends up with two HIP runtimes and torch then reports "No HIP GPUs are available". Loading torch first makes
        # this library bind to the runtime torch uses (device memory, streams and RCCL come from torch).
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(str(p))
    vp = C.c_void_p
    lib.hipr_last_error.restype = C.c_char_p
    lib.hipr_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.hipr_destroy.argtypes = [vp]
    lib.hipr_set_stream.argtypes = [vp, vp]
    lib.hipr_upload_tables.argtypes = [vp, C.POINTER(HiprTables)]
    lib.hipr_upload_scene.argtypes = [vp, C.POINTER(HiprSceneDesc)]
    lib.hipr_validate_scene.argtypes = [C.POINTER(HiprSceneDesc)]
    lib.hipr_update_scene_geometry.argtypes = [vp, C.POINTER(HiprSceneDesc)]
    lib.hipr_group_update_scene_geometry.argtypes = [vp, C.POINTER(HiprSceneDesc)]
    lib.hipr_refit_scene_transforms.argtypes = [vp, C.POINTER(HiprInstanceTransform), c_u32, C.POINTER(HiprLight), c_u32, C.POINTER(HiprRefitResult)]
    lib.hipr_group_refit_scene_transforms.argtypes = [vp, C.POINTER(HiprInstanceTransform), c_u32, C.POINTER(HiprLight), c_u32, C.POINTER(HiprRefitResult)]
    lib.hipr_update_scene_materials.argtypes = [vp, C.POINTER(HiprMaterialUpdate), c_u32, C.POINTER(HiprInstanceMaterial), c_u32]
    lib.hipr_group_update_scene_materials.argtypes = [vp, C.POINTER(HiprMaterialUpdate), c_u32, C.POINTER(HiprInstanceMaterial), c_u32]
    lib.hipr_build_bvh2.argtypes = [vp, C.POINTER(HiprTriangle), c_u32, c_u32, C.POINTER(HiprBvhNode), c_u32, C.POINTER(c_u32), C.POINTER(c_u32), C.POINTER(c_u32)]
    lib.hipr_group_build_bvh2.argtypes = [vp, C.POINTER(HiprTriangle), c_u32, c_u32, C.POINTER(HiprBvhNode), c_u32, C.POINTER(c_u32), C.POINTER(c_u32), C.POINTER(c_u32)]
    lib.hipr_debug_build_times.argtypes = [vp, C.POINTER(C.c_double)]
    lib.hipr_build_wide8.argtypes = [vp, C.POINTER(HiprBvhNode), c_u32, C.POINTER(HiprTriangle), C.POINTER(c_u32), c_u32, vp, c_u32, C.POINTER(HiprWide8BuildResult)]
    lib.hipr_group_build_wide8.argtypes = [vp, C.POINTER(HiprBvhNode), c_u32, C.POINTER(HiprTriangle), C.POINTER(c_u32), c_u32, vp, c_u32, C.POINTER(HiprWide8BuildResult)]
    lib.hipr_debug_collapse_times.argtypes = [vp, C.POINTER(C.c_double)]
    lib.hipr_build_wide4.argtypes = [vp, C.POINTER(HiprBvhNode), c_u32, c_u32, vp, c_u32, C.POINTER(HiprWide4BuildResult)]
    lib.hipr_group_build_wide4.argtypes = [vp, C.POINTER(HiprBvhNode), c_u32, c_u32, vp, c_u32, C.POINTER(HiprWide4BuildResult)]
    lib.hipr_debug_collapse4_times.argtypes = [vp, C.POINTER(C.c_double)]
    lib.hipr_rebuild_scene_trees.argtypes = [vp, c_u32, vp, c_u32, vp, vp, c_u32, C.POINTER(HiprSceneRebuildResult)]
    lib.hipr_group_rebuild_scene_trees.argtypes = [vp, c_u32, vp, c_u32, vp, vp, c_u32, C.POINTER(HiprSceneRebuildResult)]
    lib.hipr_edit_scene_instances.argtypes = [vp, C.POINTER(HiprInstanceEdit), c_u32, c_u32, vp, c_u32, vp, c_u32, vp, c_u32, C.POINTER(HiprSceneEditResult)]
    lib.hipr_group_edit_scene_instances.argtypes = [vp, C.POINTER(HiprInstanceEdit), c_u32, c_u32, vp, c_u32, vp, c_u32, vp, c_u32, C.POINTER(HiprSceneEditResult)]
    lib.hipr_append_scene_pools.argtypes = [vp, C.POINTER(HiprPoolGrowth)]
    lib.hipr_group_append_scene_pools.argtypes = [vp, C.POINTER(HiprPoolGrowth)]
    lighting = [C.POINTER(HiprLight), c_u32, C.c_int, C.POINTER(HiprEnvironmentBuild), C.POINTER(c_f), c_u64, C.POINTER(HiprLightSample), c_u32, C.POINTER(HiprLightingResult)]
    lib.hipr_update_scene_lighting.argtypes = [vp] + lighting
    lib.hipr_group_update_scene_lighting.argtypes = [vp] + lighting
    lib.hipr_debug_lighting_times.argtypes = [vp, C.POINTER(C.c_double)]
    lib.hipr_update_scene_texels.argtypes = [vp, C.POINTER(HiprTexelEdit), c_u32, C.POINTER(HiprTexelUpdateResult)]
    lib.hipr_group_update_scene_texels.argtypes = [vp, C.POINTER(HiprTexelEdit), c_u32, C.POINTER(HiprTexelUpdateResult)]
    lib.hipr_debug_texel_update_times.argtypes = [vp, C.POINTER(C.c_double)]
    lib.hipr_update_scene_vertices.argtypes = [vp, C.POINTER(HiprVertexEdit), c_u32, C.POINTER(HiprVertexUpdateResult)]
    lib.hipr_group_update_scene_vertices.argtypes = [vp, C.POINTER(HiprVertexEdit), c_u32, C.POINTER(HiprVertexUpdateResult)]
    lib.hipr_debug_vertex_update_times.argtypes = [vp, C.POINTER(C.c_double)]
    lib.hipr_set_scene_rigs.argtypes = [vp, C.POINTER(HiprRigDesc), c_u32]
    lib.hipr_group_set_scene_rigs.argtypes = [vp, C.POINTER(HiprRigDesc), c_u32]
    lib.hipr_pose_scene_rigs.argtypes = [vp, C.POINTER(HiprRigPose), c_u32, C.POINTER(HiprVertexUpdateResult)]
    lib.hipr_group_pose_scene_rigs.argtypes = [vp, C.POINTER(HiprRigPose), c_u32, C.POINTER(HiprVertexUpdateResult)]
    lib.hipr_debug_vertex_pose_times.argtypes = [vp, C.POINTER(C.c_double)]
    lib.hipr_debug_set_pose_lds_joints.argtypes = [vp, c_u32]
    lib.hipr_debug_scene_buffer_bytes.argtypes = [vp, C.c_int, C.POINTER(c_u64)]
    lib.hipr_debug_append_times.argtypes = [vp, C.POINTER(C.c_double)]
    lib.hipr_debug_rebuild_times.argtypes = [vp, C.POINTER(C.c_double)]
    lib.hipr_debug_read_scene_buffer.argtypes = [vp, C.c_int, vp, c_u64]
    lib.hipr_set_scene_state.argtypes = [vp, C.POINTER(HiprSceneState)]
    lib.hipr_set_entry_point.argtypes = [vp, C.c_int]
    lib.hipr_use_scratch_accumulation.argtypes = [vp, C.c_int]
    lib.hipr_set_frame.argtypes = [vp, C.POINTER(HiprFrameDesc)]
    lib.hipr_owned_pixel_count.argtypes = [vp, C.POINTER(c_u32)]
    lib.hipr_render_pass.argtypes = [vp, C.POINTER(HiprCameraState), vp, c_u32, C.c_int]
    lib.hipr_set_samples_per_pass.argtypes = [vp, c_u32]
    lib.hipr_trace_pass.argtypes = [vp, C.POINTER(HiprCameraState)]
    lib.hipr_accumulate_samples.argtypes = [vp, c_u32, c_u32, c_u32, vp, c_u32, C.c_int]
    lib.hipr_read_accumulation.argtypes = [vp, C.POINTER(C.c_double), c_u64]
    lib.hipr_scatter_tiles.argtypes = [vp, vp, c_u64, c_u32, c_u32, c_u32, vp, c_u32]
    lib.hipr_synchronize.argtypes = [vp]
    lib.hipr_get_counters.argtypes = [vp, C.POINTER(HiprCounters)]
    lib.hipr_reset_counters.argtypes = [vp]
    lib.hipr_set_instrumentation.argtypes = [vp, C.c_int]
    lib.hipr_set_arithmetic.argtypes = [vp, C.c_int]
    lib.hipr_get_arithmetic.argtypes = [vp]
    lib.hipr_debug_math.argtypes = [vp, C.c_int, c_u32, C.POINTER(c_f), C.POINTER(c_f), C.POINTER(c_f)]
    lib.hipr_reset_timers.argtypes = [vp]
    lib.hipr_get_kernel_times.argtypes = [vp, C.POINTER(HiprKernelTimes)]
    lib.hipr_debug_generate.argtypes = [vp, C.POINTER(HiprCameraState), c_u32, C.POINTER(c_f), C.POINTER(c_f), C.POINTER(c_u32)]
    lib.hipr_debug_sobol.argtypes = [vp, C.POINTER(c_u32), c_u32, C.POINTER(c_u32)]
    lib.hipr_debug_valu_issue_rates.argtypes = [vp, C.POINTER(C.c_double)]
    lib.hipr_group_create.argtypes = [C.POINTER(C.c_int), c_u32, C.POINTER(vp)]
    lib.hipr_group_destroy.argtypes = [vp]
    lib.hipr_group_size.argtypes = [vp]; lib.hipr_group_size.restype = c_u32
    lib.hipr_group_context.argtypes = [vp, c_u32]; lib.hipr_group_context.restype = vp
    lib.hipr_group_gather_description.argtypes = [vp]; lib.hipr_group_gather_description.restype = C.c_char_p
    lib.hipr_group_upload_tables.argtypes = [vp, C.POINTER(HiprTables)]
    lib.hipr_group_upload_scene.argtypes = [vp, C.POINTER(HiprSceneDesc)]
    lib.hipr_group_set_scene_state.argtypes = [vp, C.POINTER(HiprSceneState)]
    lib.hipr_group_set_entry_point.argtypes = [vp, C.c_int]
    lib.hipr_group_use_scratch_accumulation.argtypes = [vp, C.c_int]
    lib.hipr_group_set_frame.argtypes = [vp, c_u32, c_u32, c_u32]
    lib.hipr_group_set_samples_per_pass.argtypes = [vp, c_u32]
    lib.hipr_group_trace_pass.argtypes = [vp, C.POINTER(HiprCameraState)]
    lib.hipr_group_accumulate_samples.argtypes = [vp, c_u32, c_u32, c_u32, vp, c_u32, C.c_int]
    lib.hipr_group_read_accumulation.argtypes = [vp, C.POINTER(C.c_double), c_u64]
    lib.hipr_group_get_counters.argtypes = [vp, C.POINTER(HiprCounters)]
    lib.hipr_debug_sample_offsets.argtypes = [vp, C.POINTER(c_f)]
    lib.hipr_debug_trace_closest.argtypes = [vp, C.POINTER(c_f), C.POINTER(c_u32), c_u32, C.POINTER(c_f)]
    lib.hipr_debug_trace_shadow.argtypes = [vp, C.POINTER(c_f), c_u32, C.POINTER(c_f)]
    lib.hipr_debug_trace_fused.argtypes = [vp, C.POINTER(c_f), C.POINTER(c_u32), c_u32, C.POINTER(c_f), c_u32, C.POINTER(c_f), C.POINTER(c_f)]
    lib.hipr_debug_trace_hinted.argtypes = [vp, C.c_int, C.POINTER(c_f), C.POINTER(c_u32), c_u32, C.POINTER(c_f), c_u32, C.POINTER(c_u32), c_u32, C.POINTER(c_f), C.POINTER(c_f), C.POINTER(c_u32)]
    lib.hipr_debug_classify_hits.argtypes = [vp, C.POINTER(c_f), c_u32, C.c_int, c_u32, C.POINTER(c_u32)]
    if path is None:
        _lib = lib
    return lib


def check(lib: C.CDLL, status: int, what: str = "") -> None:
    if status != HIPR_OK:
        msg = lib.hipr_last_error()
        raise HiprError(f"{what} failed with status {status}: {msg.decode() if msg else ''}")


def load_tables():
    """Returns the five f32 tables of data/HIPRenderer/shading_tables.bin as numpy arrays (base, full, light, dense, alpha)."""
    import numpy as np
    raw = TABLES_PATH.read_bytes()
    if raw[:8] != b"HIPRTBL1":
        raise HiprError("bad shading table file")
    counts = np.frombuffer(raw[8:28], dtype="<u4")
    data = np.frombuffer(raw[28:], dtype="<f4")
    out, o = [], 0
    for n in counts:
        out.append(np.ascontiguousarray(data[o:o + int(n)]))
        o += int(n)
    return tuple(out)
