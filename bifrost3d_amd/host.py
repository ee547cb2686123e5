"""ctypes wrapper of host/libhiprenderer_host.so (scene construction, BVH build). These entry points need no GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

_lib = None


def load_host_library() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not capi.HOST_LIB_PATH.exists():
        raise capi.HiprError(f"{capi.HOST_LIB_PATH} is missing: run __graft_entry__.build()")
    capi.load_library()   # the host library links libhiprenderer.so (HIPRenderer::Renderer drives the C-ABI); keeps the torch-first load order
    lib = C.CDLL(str(capi.HOST_LIB_PATH))
    vp = C.c_void_p
    lib.hiprh_scene_create.argtypes = [C.c_char_p, C.c_uint, C.c_uint, C.c_uint]
    lib.hiprh_scene_create.restype = vp
    lib.hiprh_scene_load.argtypes = [C.c_char_p, C.c_uint]
    lib.hiprh_scene_load.restype = vp
    lib.hiprh_png_load.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_ubyte), C.c_size_t]
    lib.hiprh_png_load.restype = C.c_size_t
    lib.hiprh_make_camera.argtypes = [C.POINTER(C.c_float), C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.POINTER(capi.HiprCameraState)]
    lib.hiprh_scene_move_model.argtypes = [vp, C.c_uint, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_double]
    lib.hiprh_scene_model_pose.argtypes = [vp, C.c_uint, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_uint), C.POINTER(C.c_float), C.c_uint]
    lib.hiprh_scene_update_materials.argtypes = [vp, C.POINTER(capi.HiprMaterialUpdate), C.c_uint, C.POINTER(capi.HiprInstanceMaterial), C.c_uint]
    lib.hiprh_scene_update_texels.argtypes = [vp, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint, vp, C.c_ulonglong, C.POINTER(C.c_int)]
    lib.hiprh_scene_update_vertices.argtypes = [vp, C.POINTER(C.c_uint), C.POINTER(capi.HiprVertexEdit), C.c_uint, C.c_double]
    lib.hiprh_scene_stage_vertex_edits.argtypes = [vp, C.POINTER(C.c_uint), C.POINTER(capi.HiprVertexEdit), C.c_uint, C.POINTER(capi.HiprVertexEdit)]
    lib.hiprh_scene_apply_staged.argtypes = [vp, C.c_double]
    lib.hiprh_vertex_geometry.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint, vp]
    lib.hiprh_scene_mesh_range.argtypes = [vp, C.c_uint, C.POINTER(C.c_uint)]
    lib.hiprh_scene_set_rigs.argtypes = [vp, C.POINTER(C.c_uint), C.POINTER(capi.HiprRigDesc), C.c_uint]
    lib.hiprh_scene_pose_rigs.argtypes = [vp, C.POINTER(capi.HiprRigPose), C.c_uint, C.c_double]
    lib.hiprh_scene_stage_rig_poses.argtypes = [vp, C.POINTER(capi.HiprRigPose), C.c_uint, C.POINTER(capi.HiprRigPose)]
    lib.hiprh_posed_geometry.argtypes = [C.POINTER(capi.HiprRigDesc), C.POINTER(capi.HiprRigPose), vp]
    lib.hiprh_scene_rebuild.argtypes = [vp]
    lib.hiprh_scene_stage_model.argtypes = [vp, C.c_uint, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float]
    lib.hiprh_scene_adopt_trees.argtypes = [vp, vp, C.c_uint, vp, C.c_uint, vp, C.POINTER(capi.HiprWide8BuildResult)]
    lib.hiprh_scene_order.argtypes = [vp, C.POINTER(C.c_uint)]
    lib.hiprh_scene_order.restype = C.POINTER(C.c_uint)
    lib.hiprh_scene_rebuild_counts.argtypes = [vp, C.POINTER(C.c_uint)]
    lib.hiprh_scene_remove_model.argtypes = [vp, C.c_uint]
    lib.hiprh_scene_insert_model.argtypes = [vp, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_uint]
    lib.hiprh_scene_insert_model.restype = C.c_uint
    lib.hiprh_scene_model_info.argtypes = [vp, C.c_uint, C.POINTER(C.c_uint)]
    lib.hiprh_scene_staged_edits.argtypes = [vp, C.POINTER(capi.HiprInstanceEdit), C.c_uint]
    lib.hiprh_scene_adopt_edited_trees.argtypes = [vp, vp, C.c_uint, vp, C.c_uint, C.c_uint, vp, C.POINTER(capi.HiprWide8BuildResult)]
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint)
    lib.hiprh_scene_add_mesh.argtypes = [vp, fp, fp, fp, up, fp, C.c_uint, up, C.c_uint]
    lib.hiprh_scene_add_material.argtypes = [vp, C.POINTER(capi.HiprMaterial)]
    lib.hiprh_scene_add_texture.argtypes = [vp, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.POINTER(C.c_ubyte), C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.hiprh_scene_add_environment.argtypes = [vp, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.POINTER(C.c_ubyte), C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint]
    lib.hiprh_scene_add_light.argtypes = [vp, C.POINTER(capi.HiprLight)]
    lib.hiprh_scene_set_lights.argtypes = [vp, C.POINTER(capi.HiprLight), C.c_uint]
    lib.hiprh_scene_lights.argtypes = [vp, C.POINTER(C.c_uint)]
    lib.hiprh_scene_lights.restype = C.POINTER(capi.HiprLight)
    lib.hiprh_scene_staged_environment_build.argtypes = [vp, C.c_uint, C.c_uint, C.POINTER(capi.HiprEnvironmentBuild)]
    lib.hiprh_scene_adopt_lighting.argtypes = [vp, C.POINTER(capi.HiprLight), C.c_uint, C.c_int, C.c_uint, C.POINTER(capi.HiprLightingResult), C.POINTER(C.c_float), C.POINTER(capi.HiprLightSample)]
    lib.hiprh_scene_staged_growth.argtypes = [vp, C.POINTER(capi.HiprPoolGrowth), C.POINTER(capi.HiprInstanceEdit), C.c_uint]
    lib.hiprh_scene_materials.argtypes = [vp, C.POINTER(C.c_uint)]
    lib.hiprh_scene_materials.restype = C.POINTER(capi.HiprMaterial)
    lib.hiprh_scene_instances.argtypes = [vp, C.POINTER(C.c_uint)]
    lib.hiprh_scene_instances.restype = C.POINTER(capi.HiprInstance)
    lib.hiprh_wide8_quantise_nodes.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_uint), C.POINTER(C.c_float), vp, C.c_uint]
    lib.hiprh_wide8_quantise_nodes.restype = None
    lib.hiprh_scene_destroy.argtypes = [vp]
    lib.hiprh_scene_desc.argtypes = [vp]
    lib.hiprh_scene_desc.restype = C.POINTER(capi.HiprSceneDesc)
    lib.hiprh_scene_state.argtypes = [vp, C.POINTER(capi.HiprSceneState)]
    lib.hiprh_scene_camera.argtypes = [vp, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_float, C.POINTER(capi.HiprCameraState)]
    lib.hiprh_bvh_build.argtypes = [C.POINTER(capi.HiprTriangle), C.c_uint, C.c_uint]
    lib.hiprh_bvh_build.restype = vp
    lib.hiprh_bvh_build_on_device.argtypes = [vp, C.POINTER(capi.HiprTriangle), C.c_uint, C.c_uint, C.POINTER(C.c_int)]
    lib.hiprh_bvh_build_on_device.restype = vp
    lib.hiprh_bvh_median_splits.argtypes = [vp]; lib.hiprh_bvh_median_splits.restype = C.c_uint
    lib.hiprh_bvh_longest_median_range.argtypes = [vp]; lib.hiprh_bvh_longest_median_range.restype = C.c_uint
    lib.hiprh_scene_use_device_builder.argtypes = [vp, vp]
    lib.hiprh_scene_build_counts.argtypes = [vp, C.POINTER(C.c_uint)]
    lib.hiprh_scene_collapse_counts.argtypes = [vp, C.POINTER(C.c_uint)]
    lib.hiprh_bvh_node_count.argtypes = [vp]; lib.hiprh_bvh_node_count.restype = C.c_uint
    lib.hiprh_bvh_max_depth.argtypes = [vp]; lib.hiprh_bvh_max_depth.restype = C.c_uint
    lib.hiprh_bvh_nodes.argtypes = [vp]; lib.hiprh_bvh_nodes.restype = C.POINTER(capi.HiprBvhNode)
    lib.hiprh_bvh_order.argtypes = [vp]; lib.hiprh_bvh_order.restype = C.POINTER(C.c_uint)
    lib.hiprh_bvh_wide_node_count.argtypes = [vp]; lib.hiprh_bvh_wide_node_count.restype = C.c_uint
    lib.hiprh_bvh_wide_stack_entries.argtypes = [vp]; lib.hiprh_bvh_wide_stack_entries.restype = C.c_uint
    lib.hiprh_bvh_wide_nodes.argtypes = [vp]; lib.hiprh_bvh_wide_nodes.restype = C.POINTER(capi.HiprWideNode)
    lib.hiprh_bvh_wide8_slots.argtypes = [vp]; lib.hiprh_bvh_wide8_slots.restype = vp
    lib.hiprh_bvh_wide8_slot_count.argtypes = [vp]; lib.hiprh_bvh_wide8_slot_count.restype = C.c_uint
    lib.hiprh_bvh_wide8_height.argtypes = [vp]; lib.hiprh_bvh_wide8_height.restype = C.c_uint
    lib.hiprh_bvh_wide8_grid.argtypes = [vp, C.POINTER(C.c_float)]; lib.hiprh_bvh_wide8_grid.restype = None
    lib.hiprh_bvh_wide8_counts.argtypes = [vp, C.POINTER(C.c_uint)]; lib.hiprh_bvh_wide8_counts.restype = None
    lib.hiprh_wide8_build_on_device.argtypes = [vp, vp, C.c_uint, vp, vp, C.c_uint, C.POINTER(C.c_int)]
    lib.hiprh_wide8_build_on_device.restype = vp
    lib.hiprh_wide4_build_on_device.argtypes = [vp, vp, C.c_uint, C.c_uint, C.POINTER(C.c_int)]
    lib.hiprh_wide4_build_on_device.restype = vp
    lib.hiprh_wide4_collapse.argtypes = [vp, C.c_uint, C.c_uint, C.POINTER(C.c_uint)]
    lib.hiprh_wide4_collapse.restype = vp
    lib.hiprh_wide4_quantise_children.argtypes = [vp, vp, C.c_uint, vp]; lib.hiprh_wide4_quantise_children.restype = None
    lib.hiprh_scene_wide4_collapse_counts.argtypes = [vp, C.POINTER(C.c_uint)]
    lib.hiprh_scene_set_test_wide4_source.argtypes = [vp, C.c_int]
    lib.hiprh_scene_use_device_wide4.argtypes = [vp, vp]
    lib.hiprh_pmjbn_samples.argtypes = [C.POINTER(C.c_float), C.c_uint, C.c_uint]
    lib.hiprh_bvh_destroy.argtypes = [vp]
    lib.hiprh_renderer_bench.argtypes = [C.c_char_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_double)]
    lib.hiprh_encode_octahedral.argtypes = [C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_short)]
    _lib = lib
    return lib


def load_png(path: str, flip: bool = False) -> np.ndarray:
    """Decode a PNG with the host library's decoder into (height, width, channels) uint8; rows top-down unless `flip`."""
    lib = load_host_library()
    w, h, c = C.c_uint(), C.c_uint(), C.c_uint()
    size = lib.hiprh_png_load(path.encode(), int(flip), C.byref(w), C.byref(h), C.byref(c), None, 0)
    if size == 0:
        raise capi.HiprError(f"could not decode '{path}'")
    out = np.empty(size, dtype=np.uint8)
    lib.hiprh_png_load(path.encode(), int(flip), None, None, None, out.ctypes.data_as(C.POINTER(C.c_ubyte)), size)
    return out.reshape(h.value, w.value, c.value)


def make_camera(width: int, height: int, position=(0.0, 0.0, 0.0), rotation=(0.0, 0.0, 0.0, 1.0), field_of_view=np.pi / 4, near=0.1, far=100.0, orthographic=None,
                accumulations: int = 0, max_bounce_count: int = 4) -> capi.HiprCameraState:
    """Camera state for a free camera: perspective (field of view, near, far) or orthographic=(width, height, depth)."""
    lib = load_host_library()
    ortho = orthographic if orthographic is not None else (1.0, 1.0, 1000.0)
    params = np.array(list(position) + list(rotation) + [field_of_view, near, far, 1.0 if orthographic is not None else 0.0] + list(ortho), np.float32)
    cam = capi.HiprCameraState()
    if lib.hiprh_make_camera(params.ctypes.data_as(C.POINTER(C.c_float)), width, height, accumulations, max_bounce_count, C.byref(cam)) != 0:
        raise capi.HiprError("hiprh_make_camera failed")
    return cam


class Scene:
    """A flattened scene owned by the C++ host library (what handle_updates() would hand to hipr_upload_scene)."""

    def __init__(self, name: str, diffuse_only: bool = False, param0: int = 0, param1: int = 0, environment: bool = False, coat: bool = False, spot: bool = False, textured: bool = False,
                 device_builder=None):
        """`device_builder`: a renderer.Context whose device builds the BVH2 of this scene (hipr_build_bvh2) and collapses it to the 8-wide tree (hipr_build_wide8, unless
        HIPR_DEVICE_COLLAPSE=0) and, with HIPR_DEVICE_COLLAPSE4=1, to the 4-wide tree (hipr_build_wide4) -- the scene is rebuilt through it at once, and so is every later rebuild; where the device declines a stage, the host builds the same
        tree and build_counts() / collapse_counts() say so."""
        self.lib = load_host_library()
        if name.startswith("file:"):    # a model file set up the way SimpleViewer sets up its command-line scene
            self.handle = self.lib.hiprh_scene_load(name[5:].encode(), 1 if diffuse_only else 0)
            if not self.handle:
                raise capi.HiprError(f"could not load '{name[5:]}'")
        else:
            self.handle = self.lib.hiprh_scene_create(name.encode(), (1 if diffuse_only else 0) | (2 if environment else 0) | (4 if coat else 0) | (8 if spot else 0) | (16 if textured else 0), param0, param1)
            if not self.handle:
                raise capi.HiprError(f"unknown scene '{name}'")
        self.name = name
        self._device_builder = None
        if device_builder is not None:
            self.use_device_builder(device_builder)

    def use_device_builder(self, context) -> bool:
        """Installs (None: removes) the context's device build as the BVH2 stage and rebuilds through it. True when the device built the tree, False when the host did."""
        if context is not None and not context.handle:
            raise capi.HiprError("use_device_builder: the context is closed")
        if self._device_builder is not None:
            self._device_builder.forget_built_scene(self)
        self._device_builder = context      # the scene's builds call into the context: keep it alive ...
        if context is not None:
            context.remember_built_scene(self)      # ... and have its close() take the source out of this scene first, so that a later rebuild() is the host's
        status = self.lib.hiprh_scene_use_device_builder(self.handle, context.handle if context is not None else None)
        if status < 0:
            raise capi.HiprError("hiprh_scene_use_device_builder failed")
        return status == 1

    def build_counts(self) -> dict:
        out = (C.c_uint * 3)()
        self.lib.hiprh_scene_build_counts(self.handle, out)
        return dict(device_builds=int(out[0]), declined_builds=int(out[1]), longest_median_range=int(out[2]))

    def wide4_collapse_counts(self) -> dict:
        """Tree builds, adoptions included, whose 4-wide tree the device collapsed, and those where it was asked and the host collapsed instead."""
        out = (C.c_uint * 2)()
        self.lib.hiprh_scene_wide4_collapse_counts(self.handle, out)
        return dict(device_collapses=int(out[0]), declined_collapses=int(out[1]))

    def use_device_wide4(self, context) -> None:
        """Installs (None: removes) the context's hipr_build_wide4 as the 4-wide collapse of this scene's later builds and adoptions, whatever HIPR_DEVICE_COLLAPSE4 says.
        Nothing is rebuilt here. Context.close() takes it out again, with the other sources."""
        if context is not None and not context.handle:
            raise capi.HiprError("use_device_wide4: the context is closed")
        if context is not None:
            context.remember_built_scene(self)
        if self.lib.hiprh_scene_use_device_wide4(self.handle, context.handle if context is not None else None) < 0:
            raise capi.HiprError("hiprh_scene_use_device_wide4 failed")

    def collapse_counts(self) -> dict:
        """Builds whose 8-wide tree the device collapsed, and builds where it was asked and the host collapsed instead."""
        out = (C.c_uint * 2)()
        self.lib.hiprh_scene_collapse_counts(self.handle, out)
        return dict(device_collapses=int(out[0]), declined_collapses=int(out[1]))

    def __del__(self):
        if getattr(self, "handle", None):
            self.lib.hiprh_scene_destroy(self.handle)
            self.handle = None

    @property
    def desc(self) -> capi.HiprSceneDesc:
        return self.lib.hiprh_scene_desc(self.handle).contents

    @property
    def state(self) -> capi.HiprSceneState:
        s = capi.HiprSceneState()
        self.lib.hiprh_scene_state(self.handle, C.byref(s))
        return s

    def camera(self, width: int, height: int, accumulations: int = 0, max_bounce_count: int = -1, pdf_scale: float = 0.5, scale_decay: float = 0.0) -> capi.HiprCameraState:
        cam = capi.HiprCameraState()
        if self.lib.hiprh_scene_camera(self.handle, width, height, accumulations, max_bounce_count, pdf_scale, C.byref(cam)) != 0:
            raise capi.HiprError("hiprh_scene_camera failed")
        cam.path_regularization_scale_decay = scale_decay
        return cam

    def move_model(self, model_index: int, translation, rotation=(0.0, 0.0, 0.0, 1.0), scale: float = 1.0, rebuild_threshold: float = 0.0) -> bool:
        """Transform-only update (BVH refit). True when the topology was kept, False when the scene builder rebuilt the tree."""
        t = (C.c_float * 3)(*translation)
        r = (C.c_float * 4)(*rotation)
        status = self.lib.hiprh_scene_move_model(self.handle, model_index, t, r, scale, rebuild_threshold)
        if status < 0:
            raise capi.HiprError("hiprh_scene_move_model failed")
        return status == 1

    def model_pose(self, model_index: int, translation, rotation=(0.0, 0.0, 0.0, 1.0), scale: float = 1.0) -> list:
        """[(instance index, 3x4 object-to-world matrix)] of the model under the pose, for Context.refit_scene_transforms; the scene itself is not touched."""
        t = (C.c_float * 3)(*translation)
        r = (C.c_float * 4)(*rotation)
        count = self.lib.hiprh_scene_model_pose(self.handle, model_index, t, r, scale, None, None, 0)
        if count < 0:
            raise capi.HiprError("hiprh_scene_model_pose failed")
        indices = np.zeros(max(count, 1), np.uint32)
        matrices = np.zeros((max(count, 1), 3, 4), np.float32)
        self.lib.hiprh_scene_model_pose(self.handle, model_index, t, r, scale, indices.ctypes.data_as(C.POINTER(C.c_uint)), matrices.ctypes.data_as(C.POINTER(C.c_float)), count)
        return [(int(indices[k]), matrices[k].copy()) for k in range(count)]

    def update_materials(self, materials=(), assignments=()) -> bool:
        """Material-only update WITHOUT a rebuild (SceneBuilder::update_materials): `materials` is a sequence of (material index, capi.HiprMaterial), `assignments` one
        of (instance index, material index) -- what Context.update_scene_materials takes. False, with nothing done, when an index is out of range."""
        materials, assignments = list(materials), list(assignments)
        status = self.lib.hiprh_scene_update_materials(self.handle, capi.material_updates(materials), len(materials), capi.instance_materials(assignments), len(assignments))
        if status < 0:
            raise capi.HiprError("hiprh_scene_update_materials failed")
        return status == 1

    def update_texels(self, edits) -> bool:
        """Pixel edits WITHOUT a rebuild (SceneBuilder::update_texels), in order: `edits` as capi.texel_edits takes them -- what Context.update_scene_texels takes. False as
        soon as one is refused (where the device call would refuse); the ones before it stay applied. `environment_stale` says afterwards whether the environment's
        PDF image and samples lag behind an edit of its map."""
        array, keep = capi.texel_edits(edits)
        stale = C.c_int(0)
        for k in range(len(keep)):
            e = array[k]
            status = self.lib.hiprh_scene_update_texels(self.handle, e.texture_index, e.x, e.y, e.width, e.height, e.texels, e.row_pitch_bytes, C.byref(stale))
            if status < 0:
                raise capi.HiprError("hiprh_scene_update_texels failed")
            self.environment_stale = bool(stale.value)
            if status != 1:
                return False
        return True

    def _mesh_vertex_edits(self, edits):
        edits = list(edits)
        array, keep = capi.vertex_edits(edits)
        return edits, array, keep, (C.c_uint * max(len(edits), 1))(*[int(e["mesh"]) for e in edits])

    def update_vertices(self, edits, rebuild_threshold: float = 0.0):
        """Vertex edits WITHOUT a rebuild (SceneBuilder::update_vertices, the whole host path): `edits` as capi.vertex_edits takes them, each with a `mesh` and its
        `first` MESH-relative. True when the topology was kept, False when the builder rebuilt the scene, None when the edits were refused (nothing touched)."""
        edits, array, keep, meshes = self._mesh_vertex_edits(edits)
        status = self.lib.hiprh_scene_update_vertices(self.handle, meshes, array, len(edits), rebuild_threshold)
        if status == -1:
            raise capi.HiprError("hiprh_scene_update_vertices failed")
        return None if status == -2 else status == 1

    def stage_vertex_edits(self, edits):
        """SceneBuilder::stage_vertex_edits: the pools and the flags are written, the triangles and the trees stay behind -- `desc` must not be read until
        apply_staged(), rebuild() or an adoption has caught up. Returns the edits in POOL coordinates, what Context.update_scene_vertices takes, or None when they
        were refused (nothing touched)."""
        edits, array, keep, meshes = self._mesh_vertex_edits(edits)
        pooled = (capi.HiprVertexEdit * max(len(edits), 1))()
        status = self.lib.hiprh_scene_stage_vertex_edits(self.handle, meshes, array, len(edits), pooled)
        if status < 0:
            raise capi.HiprError("hiprh_scene_stage_vertex_edits failed")
        if status != 1:
            return None
        return [dict({name: e[name] for name in capi.VERTEX_ATTRIBUTES if e.get(name) is not None}, first=int(pooled[k].first_vertex)) for k, e in enumerate(edits)]

    def apply_staged(self, rebuild_threshold: float = 0.0) -> bool:
        """SceneBuilder::apply_staged_transforms: everything staged reaches the triangles and the trees. True when the topology was kept, False after a rebuild."""
        status = self.lib.hiprh_scene_apply_staged(self.handle, rebuild_threshold)
        if status < 0:
            raise capi.HiprError("hiprh_scene_apply_staged failed")
        return status == 1

    def vertex_geometry(self, positions, normals=None) -> np.ndarray:
        """Positions (n, 3) and normals (n, 3; None: a mesh without) packed as the geometry pool holds them (SceneBuilder::vertex_geometry): records of
        capi.vertex_geometry_dtype()."""
        positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        normals = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(len(positions), 3)
        out = np.zeros(len(positions), capi.vertex_geometry_dtype())
        floats = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
        if self.lib.hiprh_vertex_geometry(floats(positions), floats(normals), len(positions), C.c_void_p(out.ctypes.data)) != 0:
            raise capi.HiprError("hiprh_vertex_geometry failed")
        return out

    def set_rigs(self, rigs) -> bool:
        """SceneBuilder::set_rigs: the builder's rig set replaced. `rigs` as capi.rig_descs takes them, each with a `mesh` and its `first` MESH-relative. False when
        they were refused (nothing touched)."""
        rigs = list(rigs)
        array, keep = capi.rig_descs(rigs)
        status = self.lib.hiprh_scene_set_rigs(self.handle, (C.c_uint * max(len(rigs), 1))(*[int(r["mesh"]) for r in rigs]), array, len(rigs))
        if status < 0:
            raise capi.HiprError("hiprh_scene_set_rigs failed")
        return status == 1

    def pooled_rigs(self, rigs):
        """Mesh-relative rigs in POOL coordinates, what Context.set_scene_rigs takes."""
        return [dict({k: v for k, v in r.items() if k != "mesh"}, first=self.mesh_range(r["mesh"])["vertex_offset"] + r["first"]) for r in rigs]

    def pose_rigs(self, poses, rebuild_threshold: float = 0.0):
        """SceneBuilder::pose_rigs, the whole host path: `poses` as capi.rig_poses takes them. True when the topology was kept, False when the builder rebuilt the
        scene, None when the poses were refused (nothing touched)."""
        poses = list(poses)
        array, keep = capi.rig_poses(poses)
        status = self.lib.hiprh_scene_pose_rigs(self.handle, array, len(poses), rebuild_threshold)
        if status == -1:
            raise capi.HiprError("hiprh_scene_pose_rigs failed")
        return None if status == -2 else status == 1

    def stage_rig_poses(self, poses):
        """SceneBuilder::stage_rig_poses: the latest pose of each rig recorded and its instances marked as staged, nothing skinned -- `desc` must not be read until
        apply_staged(), rebuild() or an adoption has caught up. Returns the poses as Context.pose_scene_rigs takes them, or None when they were refused."""
        poses = list(poses)
        array, keep = capi.rig_poses(poses)
        pooled = (capi.HiprRigPose * max(len(poses), 1))()
        status = self.lib.hiprh_scene_stage_rig_poses(self.handle, array, len(poses), pooled)
        if status < 0:
            raise capi.HiprError("hiprh_scene_stage_rig_poses failed")
        if status != 1:
            return None
        return [dict(p, rig=int(pooled[k].rig)) for k, p in enumerate(poses)]

    def posed_geometry(self, rig, pose):
        """SceneBuilder::posed_geometry: the rows of one rig (a capi.rig_descs dict; `first` is not read) under one pose (a capi.rig_poses dict; `rig` is not read) as
        records of capi.vertex_geometry_dtype(), or None when the rig or the pose is refused."""
        rigs, keep_rig = capi.rig_descs([dict(rig, first=0)])
        poses, keep_pose = capi.rig_poses([dict(pose, rig=0)])
        out = np.zeros(max(int(rigs[0].vertex_count), 1), capi.vertex_geometry_dtype())
        status = self.lib.hiprh_posed_geometry(rigs, poses, C.c_void_p(out.ctypes.data))
        if status < 0:
            raise capi.HiprError("hiprh_posed_geometry failed")
        return out[:int(rigs[0].vertex_count)] if status == 1 else None

    def mesh_range(self, mesh: int) -> dict:
        """Where a mesh lies in the pools: vertex_offset, vertex_count, index_offset (in triples), primitive_count, flags."""
        out = (C.c_uint * 5)()
        if self.lib.hiprh_scene_mesh_range(self.handle, mesh, out) != 1:
            raise capi.HiprError(f"the scene has no mesh {mesh}")
        return dict(vertex_offset=int(out[0]), vertex_count=int(out[1]), index_offset=int(out[2]), primitive_count=int(out[3]), flags=int(out[4]))

    def rebuild(self):
        """A fresh build (triangle flags, BVH2, 4-wide and 8-wide trees) over the instances and materials as they stand."""
        if self.lib.hiprh_scene_rebuild(self.handle) != 0:
            raise capi.HiprError("hiprh_scene_rebuild failed")

    def stage_model(self, model_index: int, translation, rotation=(0.0, 0.0, 0.0, 1.0), scale: float = 1.0) -> bool:
        """SceneBuilder::stage_model_transforms: the pose is recorded in the instances only; `desc` must not be read until adopt_trees, move_model or rebuild has caught
        up. False when the pose turns an instance inside out."""
        status = self.lib.hiprh_scene_stage_model(self.handle, model_index, (C.c_float * 3)(*translation), (C.c_float * 4)(*rotation), scale)
        if status < 0:
            raise capi.HiprError("hiprh_scene_stage_model failed")
        return status == 1

    def adopt_trees(self, nodes: np.ndarray, order: np.ndarray, deepest: int, slots: np.ndarray, wide8) -> bool:
        """SceneBuilder::adopt_rebuilt_trees: the trees Context.rebuild_scene_trees made -- `nodes` (n, 16) uint32, `order`, `deepest`, `slots` (s, 16) uint32, `wide8` a
        capi.HiprWide8BuildResult or the dict build_wide8 returns -- taken over in place of a rebuild. False, with nothing touched, when they do not fit the scene."""
        nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 16)
        order = np.ascontiguousarray(order, np.uint32)
        slots = np.ascontiguousarray(slots, np.uint32).reshape(-1, 16)
        if isinstance(wide8, dict):
            wide8 = capi.HiprWide8BuildResult(wide8["slot_count"], wide8["height"], (C.c_float * 3)(*[float(v) for v in wide8["grid_min"]]), (C.c_float * 3)(*[float(v) for v in wide8["grid_cell"]]),
                                              wide8["node_count"], wide8["leaf_count"], wide8["paired_leaves"])
        if len(order) != self.desc_triangle_count() or wide8.slot_count != len(slots):
            order_pointer = None      # lengths that do not fit are the library's to refuse: it reads none of the arrays then
        else:
            order_pointer = C.c_void_p(order.ctypes.data)
        status = self.lib.hiprh_scene_adopt_trees(self.handle, C.c_void_p(nodes.ctypes.data), len(nodes), order_pointer, int(deepest), C.c_void_p(slots.ctypes.data), C.byref(wide8))
        if status < 0:
            raise capi.HiprError("hiprh_scene_adopt_trees failed")
        return status == 1

    def remove_model(self, model_index: int) -> bool:
        """SceneBuilder::remove_model: the model leaves the instance list; `desc` must not be read until rebuild() or adopt_edited_trees() has caught up. False when
        the scene has no such model."""
        status = self.lib.hiprh_scene_remove_model(self.handle, model_index)
        if status < 0:
            raise capi.HiprError("hiprh_scene_remove_model failed")
        return status == 1

    def insert_model(self, position: int, mesh: int, material: int, translation, rotation=(0.0, 0.0, 0.0, 1.0), scale: float = 1.0, model_index: int = 0) -> int:
        """SceneBuilder::insert_model: a model of a mesh and a material the scene holds at `position` of the instance list (past the end: appended). Returns the model
        index used; `desc` must not be read until rebuild() or adopt_edited_trees() has caught up."""
        used = self.lib.hiprh_scene_insert_model(self.handle, position, mesh, material, (C.c_float * 3)(*translation), (C.c_float * 4)(*rotation), scale, model_index)
        if used == 0:
            raise capi.HiprError("hiprh_scene_insert_model failed")
        return int(used)

    def model_info(self, model_index: int) -> dict:
        """The mesh, the material and the place in the instance list of a model's first instance."""
        out = (C.c_uint * 3)()
        if self.lib.hiprh_scene_model_info(self.handle, model_index, out) != 1:
            raise capi.HiprError(f"the scene has no model {model_index}")
        return dict(mesh=int(out[0]), material=int(out[1]), position=int(out[2]))

    def staged_instance_edits(self):
        """SceneBuilder::staged_instance_edits: the ctypes array of capi.HiprInstanceEdit Context.edit_scene_instances takes for the edits since the last build, or None
        when they are not the device's to apply (a pool has grown, a transform is staged as well)."""
        count = self.lib.hiprh_scene_staged_edits(self.handle, None, 0)
        if count == -2:
            return None
        if count < 0:
            raise capi.HiprError("hiprh_scene_staged_edits failed")
        edits = (capi.HiprInstanceEdit * count)()
        self.lib.hiprh_scene_staged_edits(self.handle, edits, count)
        return edits

    def add_mesh(self, positions, primitives, normals=None, texcoords=None, tints=None, emission=None) -> int:
        """SceneBuilder::add_mesh: `positions` (vertices, 3), `primitives` (triangles, 3) vertex indices; optional, one per vertex: `normals` (.., 3), `texcoords` (.., 2),
        `tints` (..,) uint32 (tint rgb, roughness), `emission` (.., 3). Returns the mesh index. After a build the pools lead the description until rebuild() or an
        adoption has caught up (staged_scene_growth)."""
        positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        primitives = np.ascontiguousarray(primitives, np.uint32).reshape(-1, 3)
        per_vertex = lambda a, dtype, width: None if a is None else np.ascontiguousarray(a, dtype).reshape(len(positions), width)
        normals, texcoords, tints, emission = per_vertex(normals, np.float32, 3), per_vertex(texcoords, np.float32, 2), per_vertex(tints, np.uint32, 1), per_vertex(emission, np.float32, 3)
        floats = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
        words = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint))
        mesh = self.lib.hiprh_scene_add_mesh(self.handle, floats(positions), floats(normals), floats(texcoords), words(tints), floats(emission), len(positions), words(primitives), len(primitives))
        if mesh < 0:
            raise capi.HiprError("hiprh_scene_add_mesh failed")
        return int(mesh)

    def add_material(self, material: capi.HiprMaterial) -> int:
        """SceneBuilder::add_material. Returns the material index."""
        index = self.lib.hiprh_scene_add_material(self.handle, C.byref(material))
        if index < 0:
            raise capi.HiprError("hiprh_scene_add_material failed")
        return int(index)

    def add_texture(self, pixels: np.ndarray, width: int, height: int, texel_format: int, is_sRGB: bool = False, repeat=(True, True), linear=(True, True)) -> int:
        """SceneBuilder::add_texture: `pixels` are the width x height texels of `texel_format` (capi.TEXEL_*) as bytes. Returns the texture index."""
        pixels = np.ascontiguousarray(pixels).view(np.uint8).reshape(-1)
        index = self.lib.hiprh_scene_add_texture(self.handle, width, height, texel_format, int(is_sRGB), pixels.ctypes.data_as(C.POINTER(C.c_ubyte)), pixels.nbytes, int(repeat[0]), int(repeat[1]),
                                                 int(linear[0]), int(linear[1]))
        if index < 0:
            raise capi.HiprError("hiprh_scene_add_texture failed")
        return int(index)

    def add_environment(self, pixels: np.ndarray, width: int, height: int, texel_format: int, is_sRGB: bool = False, repeat=(True, False), linear=(True, True), sample_count: int = 1024) -> int:
        """The scene given an environment from raw pixels through the HOST path: InfiniteAreaLight + presample_environment over the image, SceneBuilder::add_texture +
        set_environment. `pixels` are the width x height texels of `texel_format` (capi.TEXEL_RGBA8 or TEXEL_RGBA32F); `linear` = (magnification, minification).
        Returns the texture index; rebuild() before the description is read."""
        pixels = np.ascontiguousarray(pixels).view(np.uint8).reshape(-1)
        index = self.lib.hiprh_scene_add_environment(self.handle, width, height, texel_format, int(is_sRGB), pixels.ctypes.data_as(C.POINTER(C.c_ubyte)), pixels.nbytes, int(repeat[0]), int(repeat[1]),
                                                     int(linear[0]), int(linear[1]), sample_count)
        if index < 0:
            raise capi.HiprError("hiprh_scene_add_environment failed")
        return int(index)

    def add_light(self, light: capi.HiprLight) -> None:
        """SceneBuilder::add_light (the host path): rebuild() before the description is read."""
        if self.lib.hiprh_scene_add_light(self.handle, C.byref(light)) != 1:
            raise capi.HiprError("hiprh_scene_add_light failed")

    def lights(self) -> list:
        """Copies of the builder's lights, the presampled environment's (last) included."""
        count = C.c_uint()
        pointer = self.lib.hiprh_scene_lights(self.handle, C.byref(count))
        return [capi.HiprLight.from_buffer_copy(bytes(pointer[k])) for k in range(count.value)]

    def set_lights(self, lights) -> bool:
        """SceneBuilder::set_lights: the light list of a built scene replaced in place, any count and types, the environment's light kept last."""
        lights = list(lights)
        status = self.lib.hiprh_scene_set_lights(self.handle, (capi.HiprLight * max(len(lights), 1))(*lights), len(lights))
        if status < 0:
            raise capi.HiprError("hiprh_scene_set_lights failed")
        return status == 1

    def staged_environment_build(self, texture_index: int, sample_count: int):
        """SceneBuilder::staged_environment_build: the capi.HiprEnvironmentBuild Context.update_scene_lighting takes to build the environment of `texture_index` on the
        device, or None for a texture the scene does not hold. Its pointers hold until the next call of this method."""
        build = capi.HiprEnvironmentBuild()
        status = self.lib.hiprh_scene_staged_environment_build(self.handle, texture_index, sample_count, C.byref(build))
        if status < 0:
            raise capi.HiprError("hiprh_scene_staged_environment_build failed")
        return build if status == 1 else None

    def adopt_lighting(self, lights, action: int, texture_index: int = 0, updated: dict | None = None) -> bool:
        """SceneBuilder::adopt_lighting: the outcome of Context.update_scene_lighting (`updated`, its dict) taken over without a rebuild."""
        lights = list(lights)
        result = updated["result"] if updated else capi.HiprLightingResult()
        pdf = updated["per_pixel_PDF"] if updated and action == capi.ENVIRONMENT_BUILD else None
        samples = updated["samples"] if updated and action == capi.ENVIRONMENT_BUILD else None
        status = self.lib.hiprh_scene_adopt_lighting(self.handle, (capi.HiprLight * max(len(lights), 1))(*lights), len(lights), action, texture_index, C.byref(result),
                                                     pdf.ctypes.data_as(C.POINTER(C.c_float)) if pdf is not None else None,
                                                     C.cast(samples.ctypes.data, C.POINTER(capi.HiprLightSample)) if samples is not None else None)
        if status < 0:
            raise capi.HiprError("hiprh_scene_adopt_lighting failed")
        return status == 1

    def staged_scene_growth(self):
        """SceneBuilder::staged_scene_growth: (capi.HiprPoolGrowth, ctypes array of capi.HiprInstanceEdit) for everything since the last build or adoption -- what
        Context.append_scene_pools and Context.edit_scene_instances take, in that order -- or None when it is not the device's to apply (nothing built, a transform
        staged, an environment set since). The growth's pointers hold until the next call of this method and the next add_* call."""
        growth = capi.HiprPoolGrowth()
        count = self.lib.hiprh_scene_staged_growth(self.handle, C.byref(growth), None, 0)
        if count == -2:
            return None
        if count < 0:
            raise capi.HiprError("hiprh_scene_staged_growth failed")
        edits = (capi.HiprInstanceEdit * count)()
        self.lib.hiprh_scene_staged_growth(self.handle, C.byref(growth), edits, count)
        return growth, edits

    def adopt_edited_trees(self, nodes: np.ndarray, order: np.ndarray, deepest: int, slots: np.ndarray, wide8) -> bool:
        """SceneBuilder::adopt_edited_trees: the trees Context.edit_scene_instances made of the edited instance list taken over in place of a rebuild; arguments as
        adopt_trees'. False, with nothing touched, when they do not fit the scene."""
        nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 16)
        order = np.ascontiguousarray(order, np.uint32)
        slots = np.ascontiguousarray(slots, np.uint32).reshape(-1, 16)
        if isinstance(wide8, dict):
            wide8 = capi.HiprWide8BuildResult(wide8["slot_count"], wide8["height"], (C.c_float * 3)(*[float(v) for v in wide8["grid_min"]]), (C.c_float * 3)(*[float(v) for v in wide8["grid_cell"]]),
                                              wide8["node_count"], wide8["leaf_count"], wide8["paired_leaves"])
        slots_pointer = C.c_void_p(slots.ctypes.data) if wide8.slot_count == len(slots) else None      # a length that does not fit is the library's to refuse
        status = self.lib.hiprh_scene_adopt_edited_trees(self.handle, C.c_void_p(nodes.ctypes.data), len(nodes), C.c_void_p(order.ctypes.data), len(order), int(deepest), slots_pointer, C.byref(wide8))
        if status < 0:
            raise capi.HiprError("hiprh_scene_adopt_edited_trees failed")
        return status == 1

    def desc_triangle_count(self) -> int:
        return len(self.order())

    def order(self) -> np.ndarray:
        """The builder's current order: order()[k] is the position, in the order the builder flattens in, of the triangle desc.triangles[k]."""
        count = C.c_uint()
        pointer = self.lib.hiprh_scene_order(self.handle, C.byref(count))
        return np.ctypeslib.as_array(pointer, shape=(count.value,)).astype(np.uint32) if count.value else np.zeros(0, np.uint32)

    def rebuild_counts(self) -> dict:
        out = (C.c_uint * 2)()
        self.lib.hiprh_scene_rebuild_counts(self.handle, out)
        return dict(adopted=int(out[0]), refused=int(out[1]))

    def materials(self) -> list:
        """Copies of the scene's materials (capi.HiprMaterial), slot 0 the invalid material."""
        count = C.c_uint()
        pointer = self.lib.hiprh_scene_materials(self.handle, C.byref(count))
        out = []
        for k in range(count.value):
            m = capi.HiprMaterial()
            C.memmove(C.byref(m), C.byref(pointer[k]), C.sizeof(capi.HiprMaterial))
            out.append(m)
        return out

    def materials_array(self) -> np.ndarray:
        count = C.c_uint()
        pointer = self.lib.hiprh_scene_materials(self.handle, C.byref(count))
        return np.ctypeslib.as_array(C.cast(pointer, C.POINTER(C.c_uint32)), shape=(count.value, 16)).copy()

    def instances_array(self) -> np.ndarray:
        count = C.c_uint()
        pointer = self.lib.hiprh_scene_instances(self.handle, C.byref(count))
        return np.ctypeslib.as_array(C.cast(pointer, C.POINTER(C.c_uint32)), shape=(count.value, 20)).copy()

    def wide8_slots(self) -> np.ndarray:
        d = self.desc
        return np.ctypeslib.as_array(C.cast(d.wide8_slots, C.POINTER(C.c_uint32)), shape=(d.wide8_slot_count, 16)).copy()

    def triangles(self) -> np.ndarray:
        d = self.desc
        return np.ctypeslib.as_array(C.cast(d.triangles, C.POINTER(C.c_uint32)), shape=(d.triangle_count, 12)).copy()

    def nodes(self) -> np.ndarray:
        d = self.desc
        return np.ctypeslib.as_array(C.cast(d.nodes, C.POINTER(C.c_uint32)), shape=(d.node_count, 16)).copy()


def renderer_bench(target_triangles: int, width: int, height: int, warmup_calls: int, calls: int, max_batch: int) -> dict:
    """Times `calls` HIPRenderer::Renderer::render() calls on the atrium built in the Bifrost managers (the plugin path end to end)."""
    lib = load_host_library()
    out = (C.c_double * 3)()
    status = lib.hiprh_renderer_bench(str(capi.TABLES_PATH.parent.parent).encode(), target_triangles, width, height, warmup_calls, calls, max_batch, out)
    if status != 0:
        raise capi.HiprError(f"hiprh_renderer_bench failed with status {status}")
    return {"milliseconds": out[0], "accumulations": int(out[1]), "triangles": int(out[2]), "calls": calls, "max_batch": max_batch}
