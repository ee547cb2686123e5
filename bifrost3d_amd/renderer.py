"""Thin Python handle on a HiprContext (include/hiprenderer_c.h). Plumbing only; fails loudly without the HIP library."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi


class Context:
    def __init__(self, device_id: int = 0, library=None, arithmetic=None):
        """`library`: another build of libhiprenderer.so (A/B builds of the kernels); the product library by default.
        `arithmetic`: "fast" / "exact" (or capi.HIPR_ARITHMETIC_*): hipr_set_arithmetic; None keeps the library's default (fast, or what HIPR_ARITHMETIC says)."""
        self.lib = capi.load_library(library)
        self.device_id = device_id
        self.handle = C.c_void_p()
        capi.check(self.lib, self.lib.hipr_create(device_id, C.byref(self.handle)), "hipr_create")
        if arithmetic is not None:
            self.set_arithmetic(arithmetic)
        self._tables = capi.load_tables()
        t = capi.HiprTables(*[a.ctypes.data_as(C.POINTER(C.c_float)) for a in self._tables])
        capi.check(self.lib, self.lib.hipr_upload_tables(self.handle, C.byref(t)), "hipr_upload_tables")
        self.frame = None

    def remember_built_scene(self, scene):
        """A host.Scene whose builds call hipr_build_bvh2 and hipr_build_wide8 on this context (Scene.use_device_builder)."""
        if not hasattr(self, "_built_scenes"):
            import weakref
            self._built_scenes = weakref.WeakSet()
        self._built_scenes.add(scene)

    def forget_built_scene(self, scene):
        getattr(self, "_built_scenes", set()).discard(scene)

    def close(self):
        if self.handle:
            for scene in list(getattr(self, "_built_scenes", ())):      # no scene keeps a destroyed context as the source of its builds
                if getattr(scene, "handle", None):
                    scene.use_device_builder(None)
            self.lib.hipr_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, status, what):
        capi.check(self.lib, status, what)

    def set_arithmetic(self, arithmetic):
        mode = {"fast": capi.HIPR_ARITHMETIC_FAST, "exact": capi.HIPR_ARITHMETIC_EXACT}.get(arithmetic, arithmetic)
        self._check(self.lib.hipr_set_arithmetic(self.handle, int(mode)), "hipr_set_arithmetic")

    @property
    def arithmetic(self) -> str:
        mode = self.lib.hipr_get_arithmetic(self.handle)
        if mode < 0:
            self._check(mode, "hipr_get_arithmetic")
        return "exact" if mode == capi.HIPR_ARITHMETIC_EXACT else "fast"

    def debug_math(self, function: int, x, y=None):
        """sin (0), cos (1) or pow(x, y) (2) as the shade unit of the context's arithmetic mode evaluates them."""
        x = np.ascontiguousarray(x, np.float32)
        y = np.ascontiguousarray(y if y is not None else np.zeros_like(x), np.float32)
        out = np.zeros_like(x)
        fp = C.POINTER(C.c_float)
        self._check(self.lib.hipr_debug_math(self.handle, function, x.size, x.ctypes.data_as(fp), y.ctypes.data_as(fp), out.ctypes.data_as(fp)), "hipr_debug_math")
        return out

    def set_stream(self, stream_ptr: int | None):
        self._check(self.lib.hipr_set_stream(self.handle, C.c_void_p(stream_ptr or 0)), "hipr_set_stream")

    def upload_scene(self, scene):
        self._scene = scene   # keep the host arrays alive until uploaded (copy happens inside)
        self._rebuilt_counts = None
        self._check(self.lib.hipr_upload_scene(self.handle, C.byref(scene.desc)), "hipr_upload_scene")
        self._resident_counts = (scene.desc.triangle_count, scene.desc.instance_count, scene.desc.material_count)      # an edit of the instance list changes the first two
        state = scene.state
        self._check(self.lib.hipr_set_scene_state(self.handle, C.byref(state)), "hipr_set_scene_state")

    def update_scene_geometry(self, scene):
        self._scene = scene
        self._rebuilt_counts = None
        self._check(self.lib.hipr_update_scene_geometry(self.handle, C.byref(scene.desc)), "hipr_update_scene_geometry")
        self._resident_counts = (scene.desc.triangle_count, scene.desc.instance_count, scene.desc.material_count)      # an edit of the instance list changes the first two

    def refit_scene_transforms(self, moved=(), lights=None) -> dict:
        """hipr_refit_scene_transforms: `moved` is a sequence of (instance index, 3x4 matrix) -- Scene.model_pose() -- refitted on the device; `lights`: None keeps the
        lights, else a sequence of capi.HiprLight that replaces them one for one. Returns needs_rebuild, child_half_area, uploaded_half_area, grid_min, grid_cell."""
        moved = list(moved)
        array = (capi.HiprInstanceTransform * max(len(moved), 1))()
        for k, (index, matrix) in enumerate(moved):
            array[k].instance_index = int(index)
            array[k].object_to_world[:] = [float(v) for v in np.asarray(matrix, np.float32).reshape(12)]
        light_array, light_count = None, 0
        if lights is not None:
            lights = list(lights)
            light_array, light_count = (capi.HiprLight * max(len(lights), 1))(*lights), len(lights)
        result = capi.HiprRefitResult()
        self._check(self.lib.hipr_refit_scene_transforms(self.handle, array, len(moved), light_array, light_count, C.byref(result)), "hipr_refit_scene_transforms")
        return dict(needs_rebuild=bool(result.needs_rebuild), child_half_area=float(result.child_half_area), uploaded_half_area=float(result.uploaded_half_area),
                    grid_min=np.array(result.grid_min[:], np.float32), grid_cell=np.array(result.grid_cell[:], np.float32))

    def update_scene_materials(self, materials=(), assignments=()):
        """hipr_update_scene_materials: `materials` is a sequence of (material index, capi.HiprMaterial) that rewrites slots of the uploaded material pool, `assignments`
        one of (instance index, material index) that gives uploaded instances another material; applied to the resident scene by kernels, no upload."""
        materials, assignments = list(materials), list(assignments)
        self._check(self.lib.hipr_update_scene_materials(self.handle, capi.material_updates(materials), len(materials), capi.instance_materials(assignments), len(assignments)),
                    "hipr_update_scene_materials")

    def build_bvh2(self, triangles: np.ndarray, max_depth: int = 62, nodes: np.ndarray | None = None, order: np.ndarray | None = None):
        """hipr_build_bvh2: the host builder's BVH2 of `triangles` ((n, 12) uint32 words of HiprTriangle) built on the device. Returns (status, nodes (node_count, 16) uint32,
        order (n,) uint32, deepest leaf); on a status other than HIPR_OK the arrays are the caller's `nodes` / `order` (or zeros) as the call left them, whole."""
        triangles = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 12)
        n = len(triangles)
        nodes = np.zeros((max(n - 1, 1), 16), np.uint32) if nodes is None else nodes
        order = np.zeros(n, np.uint32) if order is None else order
        node_count, deepest = C.c_uint32(0), C.c_uint32(0)
        status = self.lib.hipr_build_bvh2(self.handle, C.cast(triangles.ctypes.data, C.POINTER(capi.HiprTriangle)), n, max_depth, C.cast(nodes.ctypes.data, C.POINTER(capi.HiprBvhNode)), len(nodes),
                                          C.byref(node_count), C.cast(order.ctypes.data, C.POINTER(C.c_uint32)), C.byref(deepest))
        if status != capi.HIPR_OK:
            return status, nodes, order, 0
        return status, nodes[:node_count.value], order, deepest.value

    def build_times(self) -> dict:
        """Milliseconds of the last build_bvh2: argument checks, allocation + upload, kernels, read-back."""
        out = (C.c_double * 4)()
        self._check(self.lib.hipr_debug_build_times(self.handle, out), "hipr_debug_build_times")
        return dict(validate=out[0], upload=out[1], kernels=out[2], readback=out[3])

    def build_wide8(self, nodes: np.ndarray, triangles: np.ndarray, order: np.ndarray | None = None, slots: np.ndarray | None = None, result: np.ndarray | None = None):
        """hipr_build_wide8: the host's 8-wide tree over the BVH2 `nodes` ((n, 16) uint32 words of HiprBvhNode), `triangles` ((t, 12) words of HiprTriangle) and the
        `order` the leaves reference them in (None: as stored), collapsed on the device. Returns (status, slots (slot_count, 16) uint32, result): `result` a dict of
        slot_count, height, grid_min, grid_cell, node_count, leaf_count, paired_leaves. `slots` ((capacity, 16) uint32) and `result` (12 uint32 words of
        HiprWide8BuildResult) may be the caller's; on a status other than HIPR_OK both are returned whole as the call left them."""
        nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 16)
        triangles = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 12)
        order = None if order is None else np.ascontiguousarray(order, np.uint32)
        slots = np.zeros((max(2 * len(triangles), 1), 16), np.uint32) if slots is None else slots
        raw = np.zeros(C.sizeof(capi.HiprWide8BuildResult) // 4, np.uint32) if result is None else result
        status = self.lib.hipr_build_wide8(self.handle, C.cast(nodes.ctypes.data, C.POINTER(capi.HiprBvhNode)), len(nodes), C.cast(triangles.ctypes.data, C.POINTER(capi.HiprTriangle)),
                                           C.cast(order.ctypes.data, C.POINTER(C.c_uint32)) if order is not None else None, len(triangles), slots.ctypes.data, len(slots),
                                           C.cast(raw.ctypes.data, C.POINTER(capi.HiprWide8BuildResult)))
        if status != capi.HIPR_OK:
            return status, slots, raw
        r = capi.HiprWide8BuildResult.from_buffer_copy(raw.tobytes())
        return status, slots[:r.slot_count], dict(slot_count=r.slot_count, height=r.height, grid_min=np.array(r.grid_min[:], np.float32), grid_cell=np.array(r.grid_cell[:], np.float32),
                                                  node_count=r.node_count, leaf_count=r.leaf_count, paired_leaves=r.paired_leaves)

    def build_wide4(self, nodes: np.ndarray, triangle_count: int, wide: np.ndarray | None = None, result: np.ndarray | None = None, group=None):
        """hipr_build_wide4: the host's compressed 4-wide tree over the BVH2 `nodes` ((n, 16) uint32 words of HiprBvhNode) whose leaves reference `triangle_count`
        triangles, collapsed on the device. Returns (status, wide nodes (node_count, 16) uint32, result): `result` a dict of node_count and stack_entries. `wide`
        ((capacity, 16) uint32) and `result` (2 uint32 words of HiprWide4BuildResult) may be the caller's; on a status other than HIPR_OK both are returned whole as the
        call left them. `group`: a HiprGroup handle, for hipr_group_build_wide4."""
        nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 16)
        wide = np.zeros((max(len(nodes), 1), 16), np.uint32) if wide is None else wide
        raw = np.zeros(2, np.uint32) if result is None else result
        call, handle = (self.lib.hipr_group_build_wide4, group) if group is not None else (self.lib.hipr_build_wide4, self.handle)
        status = call(handle, C.cast(nodes.ctypes.data, C.POINTER(capi.HiprBvhNode)), len(nodes), triangle_count, wide.ctypes.data, len(wide), C.cast(raw.ctypes.data, C.POINTER(capi.HiprWide4BuildResult)))
        if status != capi.HIPR_OK:
            return status, wide, raw
        return status, wide[:int(raw[0])], dict(node_count=int(raw[0]), stack_entries=int(raw[1]))

    def collapse4_times(self) -> dict:
        """Milliseconds of the last build_wide4: the walk over the indices, allocation + upload, kernels, read-back."""
        out = (C.c_double * 4)()
        self._check(self.lib.hipr_debug_collapse4_times(self.handle, out), "hipr_debug_collapse4_times")
        return dict(validate=out[0], upload=out[1], kernels=out[2], readback=out[3])

    def rebuild_scene_trees(self, max_depth: int = 62, read_back: bool = True, group=None) -> dict:
        """hipr_rebuild_scene_trees: the trees of the resident scene rebuilt on the device from the triangles it holds (after a refit_scene_transforms that moved a model
        far, or reported needs_rebuild). Returns a dict of status, node_count, deepest, wide8 (as build_wide8's result), half_area and -- `read_back` -- nodes
        ((node_count, 16) uint32), order ((triangles,) uint32, Scene.adopt_trees takes them) and slots ((slot_count, 16)). On a status other than HIPR_OK the dict holds
        the status and the arrays whole as the call left them. `group`: a HiprGroup handle, for hipr_group_rebuild_scene_trees."""
        n = self._scene.desc.triangle_count
        nodes = np.zeros((max(n - 1, 1), 16), np.uint32) if read_back else None
        order = np.zeros(n, np.uint32) if read_back else None
        slots = np.zeros((max(min(2 * n, 0xFFFFFF), 1), 16), np.uint32) if read_back else None
        result = capi.HiprSceneRebuildResult()
        pointer = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        call, handle = (self.lib.hipr_group_rebuild_scene_trees, group) if group is not None else (self.lib.hipr_rebuild_scene_trees, self.handle)
        status = call(handle, max_depth, pointer(nodes), len(nodes) if read_back else 0, pointer(order), pointer(slots), len(slots) if read_back else 0, C.byref(result))
        if status != capi.HIPR_OK:
            return dict(status=status, nodes=nodes, order=order, slots=slots)
        w = result.wide8
        if group is None:
            self._rebuilt_counts = (result.node_count, w.slot_count)
        out = dict(status=status, node_count=result.node_count, deepest=result.deepest, half_area=float(result.half_area),
                   wide8=dict(slot_count=w.slot_count, height=w.height, grid_min=np.array(w.grid_min[:], np.float32), grid_cell=np.array(w.grid_cell[:], np.float32), node_count=w.node_count,
                              leaf_count=w.leaf_count, paired_leaves=w.paired_leaves), raw=result)
        if read_back:
            out.update(nodes=nodes[:result.node_count], order=order, slots=slots[:w.slot_count])
        return out

    def edit_scene_instances(self, edits, max_depth: int = 62, read_back: bool = True, group=None, capacities=None) -> dict:
        """hipr_edit_scene_instances: models of the resident scene added and removed on the device. `edits` is the NEW instance list in order, a ctypes array of
        capi.HiprInstanceEdit (Scene.staged_instance_edits makes it) or a sequence of them. Returns a dict of status, triangle_count, instance_count, node_count,
        deepest, wide8 (as build_wide8's result), half_area and -- `read_back` -- nodes, order and slots (Scene.adopt_edited_trees takes them). On a status other than
        HIPR_OK the dict holds the status and the arrays whole as the call left them. `capacities`: (nodes, order words, slots) of the read-back arrays, by default
        what the largest list the pools allow can need. `group`: a HiprGroup handle, for hipr_group_edit_scene_instances."""
        if edits is not None and not isinstance(edits, C.Array):
            edits = (capi.HiprInstanceEdit * len(edits))(*edits)
        count = len(edits) if edits is not None else 0
        triangles = self._resident_counts[0]      # not the host scene's: its description lags behind while edits are staged
        bound = triangles + sum(int(e.primitive_count) for e in edits if e.source == capi.EDIT_NEW_INSTANCE) if edits is not None else triangles
        node_room, order_room, slot_room = capacities or (max(bound - 1, 1), max(bound, 1), max(min(2 * bound, 0xFFFFFF), 1))
        nodes = np.zeros((node_room, 16), np.uint32) if read_back else None
        order = np.zeros(order_room, np.uint32) if read_back else None
        slots = np.zeros((slot_room, 16), np.uint32) if read_back else None
        result = capi.HiprSceneEditResult()
        pointer = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        call, handle = (self.lib.hipr_group_edit_scene_instances, group) if group is not None else (self.lib.hipr_edit_scene_instances, self.handle)
        status = call(handle, edits, count, max_depth, pointer(nodes), len(nodes) if read_back else 0, pointer(order), len(order) if read_back else 0, pointer(slots),
                      len(slots) if read_back else 0, C.byref(result))
        if status != capi.HIPR_OK:
            return dict(status=status, nodes=nodes, order=order, slots=slots)
        w = result.wide8
        if group is None:
            self._rebuilt_counts = (result.node_count, w.slot_count)
            self._resident_counts = (result.triangle_count, result.instance_count, self._resident_counts[2])
        out = dict(status=status, triangle_count=result.triangle_count, instance_count=result.instance_count, node_count=result.node_count, deepest=result.deepest,
                   half_area=float(result.half_area),
                   wide8=dict(slot_count=w.slot_count, height=w.height, grid_min=np.array(w.grid_min[:], np.float32), grid_cell=np.array(w.grid_cell[:], np.float32), node_count=w.node_count,
                              leaf_count=w.leaf_count, paired_leaves=w.paired_leaves), raw=result)
        if read_back:
            out.update(nodes=nodes[:result.node_count], order=order[:result.triangle_count], slots=slots[:w.slot_count])
        return out

    def append_scene_pools(self, growth, group=None) -> int:
        """hipr_append_scene_pools: the resident pools grown at their tails, the step before edit_scene_instances when a model comes over a new mesh, material or
        texture. `growth` is a capi.HiprPoolGrowth (Scene.staged_scene_growth makes it, with the edit list). Returns the status: a refusal leaves the scene as found
        and is the caller's to answer with the full path. `group`: a HiprGroup handle, for hipr_group_append_scene_pools."""
        call, handle = (self.lib.hipr_group_append_scene_pools, group) if group is not None else (self.lib.hipr_append_scene_pools, self.handle)
        status = call(handle, C.byref(growth) if growth is not None else None)
        counts = getattr(self, "_resident_counts", None)
        if status == capi.HIPR_OK and group is None and counts is not None:
            self._resident_counts = (counts[0], counts[1], counts[2] + growth.material_count)
        return status

    def update_scene_lighting(self, lights=(), action: int = capi.ENVIRONMENT_KEEP, build=None, read_back: bool = True, group=None, capacities=None) -> dict:
        """hipr_update_scene_lighting: the lights of the resident scene replaced by `lights` (capi.HiprLight, WITHOUT the environment's) and the environment kept,
        removed or -- `build`, a capi.HiprEnvironmentBuild (Scene.staged_environment_build makes it) -- rebuilt on the device from the resident texels. Returns a dict of
        status and, when it is HIPR_OK, result (capi.HiprLightingResult), pdf_width, pdf_height, sample_count, disabled, light_count, switches and -- a build with
        `read_back` -- per_pixel_PDF (float32) and samples ((n, 8) float32) as Scene.adopt_lighting takes them. `capacities`: (PDF floats, samples) of the read-back
        arrays. `group`: a HiprGroup handle, for hipr_group_update_scene_lighting."""
        lights = list(lights) if lights is not None else None
        array = (capi.HiprLight * max(len(lights), 1))(*lights) if lights is not None else None
        pdf = samples = None
        if build is not None and read_back:
            texture = self.read_scene_buffer(capi.SCENE_BUFFER_TEXTURES)
            width = int(texture[build.environment_map_ID][0]) if 0 < build.environment_map_ID < len(texture) else 1
            pdf_room, sample_room = capacities or (width * build.pdf_height, build.sample_count)
            pdf, samples = np.zeros(max(pdf_room, 1), np.float32), np.zeros((max(sample_room, 1), 8), np.float32)
        result = capi.HiprLightingResult()
        call, handle = (self.lib.hipr_group_update_scene_lighting, group) if group is not None else (self.lib.hipr_update_scene_lighting, self.handle)
        status = call(handle, array, len(lights) if lights is not None else 1, action, C.byref(build) if build is not None else None,
                      pdf.ctypes.data_as(C.POINTER(C.c_float)) if pdf is not None else None, (capacities[0] if capacities else len(pdf)) if pdf is not None else 0,
                      C.cast(samples.ctypes.data, C.POINTER(capi.HiprLightSample)) if samples is not None else None, (capacities[1] if capacities else len(samples)) if samples is not None else 0,
                      C.byref(result))
        if status != capi.HIPR_OK:
            return dict(status=status)
        out = dict(status=status, result=result, pdf_width=result.pdf_width, pdf_height=result.pdf_height, sample_count=result.sample_count, disabled=bool(result.importance_sampling_disabled),
                   light_count=result.light_count, switches=result.switches)
        if pdf is not None:
            out["per_pixel_PDF"] = np.ascontiguousarray(pdf[:result.pdf_width * result.pdf_height])
            out["samples"] = np.ascontiguousarray(samples[:result.sample_count])
        return out

    def update_scene_texels(self, edits, group=None) -> dict:
        """hipr_update_scene_texels: rectangles of new texels of textures the device holds, applied to the resident scene by kernels, no upload. `edits` as
        capi.texel_edits takes them. Returns a dict of status and, when it is HIPR_OK, candidate_triangles, changed_triangles, all_triangles_opaque and
        environment_stale: a refusal leaves the scene as found and is the caller's to answer with the full path. `group`: a HiprGroup handle, for
        hipr_group_update_scene_texels."""
        array, keep = capi.texel_edits(edits)
        result = capi.HiprTexelUpdateResult()
        call, handle = (self.lib.hipr_group_update_scene_texels, group) if group is not None else (self.lib.hipr_update_scene_texels, self.handle)
        status = call(handle, array, len(keep), C.byref(result))
        if status != capi.HIPR_OK:
            return dict(status=status)
        return dict(status=status, candidate_triangles=result.candidate_triangles, changed_triangles=result.changed_triangles, all_triangles_opaque=bool(result.all_triangles_opaque),
                    environment_stale=bool(result.environment_stale))

    def texel_update_times(self) -> dict:
        """Milliseconds of the last update_scene_texels: the rows packed and their staging copy, the rectangle writes, the coverage passes, the leaf pass."""
        out = (C.c_double * 4)()
        self._check(self.lib.hipr_debug_texel_update_times(self.handle, out), "hipr_debug_texel_update_times")
        return dict(staging=out[0], writes=out[1], coverage=out[2], leaves=out[3])

    def update_scene_vertices(self, edits, group=None) -> dict:
        """hipr_update_scene_vertices: new values for vertices of meshes the device holds, applied to the resident scene by kernels, no upload. `edits` as
        capi.vertex_edits takes them, in POOL coordinates (Scene.stage_vertex_edits makes them). Returns a dict of status and, when it is HIPR_OK, needs_rebuild,
        child_half_area, uploaded_half_area, grid_min, grid_cell, moved_triangles, candidate_triangles, changed_triangles and all_triangles_opaque: a refusal leaves
        the scene as found and is the caller's to answer with the full path. `group`: a HiprGroup handle, for hipr_group_update_scene_vertices."""
        edits = list(edits)
        array, keep = capi.vertex_edits(edits)
        result = capi.HiprVertexUpdateResult()
        call, handle = (self.lib.hipr_group_update_scene_vertices, group) if group is not None else (self.lib.hipr_update_scene_vertices, self.handle)
        status = call(handle, array, len(edits), C.byref(result))
        if status != capi.HIPR_OK:
            return dict(status=status)
        refit = result.refit
        return dict(status=status, needs_rebuild=bool(refit.needs_rebuild), child_half_area=refit.child_half_area, uploaded_half_area=refit.uploaded_half_area,
                    grid_min=np.array(refit.grid_min[:], np.float32), grid_cell=np.array(refit.grid_cell[:], np.float32), moved_triangles=result.moved_triangles,
                    candidate_triangles=result.candidate_triangles, changed_triangles=result.changed_triangles, all_triangles_opaque=bool(result.all_triangles_opaque))

    def set_scene_rigs(self, rigs, group=None) -> int:
        """hipr_set_scene_rigs: the resident rig set replaced (an empty list removes all rigs). `rigs` as capi.rig_descs takes them, `first` in POOL coordinates.
        Returns the status: a refusal leaves the bound set and the scene as found. `group`: a HiprGroup handle, for hipr_group_set_scene_rigs."""
        rigs = list(rigs)
        array, keep = capi.rig_descs(rigs)
        call, handle = (self.lib.hipr_group_set_scene_rigs, group) if group is not None else (self.lib.hipr_set_scene_rigs, self.handle)
        return call(handle, array, len(rigs))

    def pose_scene_rigs(self, poses, group=None) -> dict:
        """hipr_pose_scene_rigs: bound rigs posed by one kernel, then what update_scene_vertices runs after an edit of geometry. `poses` as capi.rig_poses takes
        them. Returns a dict shaped like update_scene_vertices'. `group`: a HiprGroup handle, for hipr_group_pose_scene_rigs."""
        poses = list(poses)
        array, keep = capi.rig_poses(poses)
        result = capi.HiprVertexUpdateResult()
        call, handle = (self.lib.hipr_group_pose_scene_rigs, group) if group is not None else (self.lib.hipr_pose_scene_rigs, self.handle)
        status = call(handle, array, len(poses), C.byref(result))
        if status != capi.HIPR_OK:
            return dict(status=status)
        refit = result.refit
        return dict(status=status, needs_rebuild=bool(refit.needs_rebuild), child_half_area=refit.child_half_area, uploaded_half_area=refit.uploaded_half_area,
                    grid_min=np.array(refit.grid_min[:], np.float32), grid_cell=np.array(refit.grid_cell[:], np.float32), moved_triangles=result.moved_triangles,
                    candidate_triangles=result.candidate_triangles, changed_triangles=result.changed_triangles, all_triangles_opaque=bool(result.all_triangles_opaque))

    def vertex_pose_times(self) -> dict:
        """Milliseconds of the last pose_scene_rigs: the block table, matrices and weights packed and their staging copy, the pose kernel, the refit passes with the
        records."""
        out = (C.c_double * 4)()
        self._check(self.lib.hipr_debug_vertex_pose_times(self.handle, out), "hipr_debug_vertex_pose_times")
        return dict(staging=out[0], pose=out[1], refit=out[2])

    def vertex_update_times(self) -> dict:
        """Milliseconds of the last update_scene_vertices: the table and rows packed and their staging copy, the pool writes, the refit passes with the records, the
        flag pass with the leaf pass."""
        out = (C.c_double * 4)()
        self._check(self.lib.hipr_debug_vertex_update_times(self.handle, out), "hipr_debug_vertex_update_times")
        return dict(staging=out[0], writes=out[1], refit=out[2], flags=out[3])

    def lighting_times(self) -> dict:
        """Milliseconds of the last update_scene_lighting: allocations + uploads, kernels, the host's finish of the samples, read-back."""
        out = (C.c_double * 4)()
        self._check(self.lib.hipr_debug_lighting_times(self.handle, out), "hipr_debug_lighting_times")
        return dict(upload=out[0], kernels=out[1], finish=out[2], readback=out[3])

    def append_times(self) -> dict:
        """Milliseconds of the last append_scene_pools: the new allocations, the device-to-device copies of the resident parts, the tails with the mirror segments."""
        out = (C.c_double * 3)()
        self._check(self.lib.hipr_debug_append_times(self.handle, out), "hipr_debug_append_times")
        return dict(allocation=out[0], resident_copies=out[1], tails=out[2])

    def rebuild_times(self) -> dict:
        """Milliseconds of the last rebuild_scene_trees: flatten order, BVH2, collapse (with the slots copied to the host), the new resident arrays, the outputs' read-back."""
        out = (C.c_double * 5)()
        self._check(self.lib.hipr_debug_rebuild_times(self.handle, out), "hipr_debug_rebuild_times")
        return dict(flatten=out[0], bvh2=out[1], collapse=out[2], install=out[3], readback=out[4])

    def collapse_times(self) -> dict:
        """Milliseconds of the last build_wide8: the walk over the indices, allocation + upload, kernels, read-back."""
        out = (C.c_double * 4)()
        self._check(self.lib.hipr_debug_collapse_times(self.handle, out), "hipr_debug_collapse_times")
        return dict(validate=out[0], upload=out[1], kernels=out[2], readback=out[3])

    def read_scene_buffer(self, which: int) -> np.ndarray:
        """The scene array the device holds (hipr_debug_read_scene_buffer): capi.SCENE_BUFFER_TRIANGLES -> (triangles, 12) uint32 words, SCENE_BUFFER_WIDE8_SLOTS -> (slots, 16),
        _TRACE_TRIANGLES -> (triangles, 12), _SHADE_TRIANGLES -> (triangles, 32), _TRIANGLE_CLASS -> (triangles,) uint8, _MATERIALS -> (materials, 16), _INSTANCES -> (instances, 20), SCENE_BUFFER_NODES -> (BVH2 nodes, 16). The pools append_scene_pools grows, each as long as
        the device's count says (hipr_debug_scene_buffer_bytes): _INDICES -> (words,) uint32, _GEOMETRY -> (vertices, 4), _TEXCOORDS -> (vertices, 2), _TINTS -> (vertices,),
        _EMISSIONS -> (vertices, 3), _TEXTURES -> (textures, 6), all uint32 words, _TEXELS -> (bytes,) uint8; a pool the device does not hold has no rows."""
        pools = {capi.SCENE_BUFFER_INDICES: (1, np.uint32), capi.SCENE_BUFFER_GEOMETRY: (4, np.uint32), capi.SCENE_BUFFER_TEXCOORDS: (2, np.uint32), capi.SCENE_BUFFER_TINTS: (1, np.uint32),
                 capi.SCENE_BUFFER_EMISSIONS: (3, np.uint32), capi.SCENE_BUFFER_TEXTURES: (6, np.uint32), capi.SCENE_BUFFER_TEXELS: (1, np.uint8),
                 capi.SCENE_BUFFER_LIGHTS: (12, np.uint32), capi.SCENE_BUFFER_ENVIRONMENT_PDF: (1, np.uint32), capi.SCENE_BUFFER_ENVIRONMENT_SAMPLES: (8, np.uint32)}
        if which in pools:
            width, dtype = pools[which]
            size = capi.c_u64()
            self._check(self.lib.hipr_debug_scene_buffer_bytes(self.handle, int(which), C.byref(size)), "hipr_debug_scene_buffer_bytes")
            rows = size.value // (width * np.dtype(dtype).itemsize)
            out = np.zeros((rows, width) if width > 1 else (rows,), dtype)
            self._check(self.lib.hipr_debug_read_scene_buffer(self.handle, int(which), C.c_void_p(out.ctypes.data if rows else C.addressof(size)), out.nbytes), "hipr_debug_read_scene_buffer")
            return out
        # the device's counts, not the host scene's: a device rebuild changes the first two, and the description lags behind while edits or moves are staged in it
        node_count, slot_count = getattr(self, "_rebuilt_counts", None) or (self._scene.desc.node_count, self._scene.desc.wide8_slot_count)
        counts = getattr(self, "_resident_counts", None)      # absent on a context whose scene was uploaded past this wrapper: then the description is the device's
        triangle_count, instance_count, material_count = counts or (self._scene.desc.triangle_count, self._scene.desc.instance_count, self._scene.desc.material_count)
        shape, dtype = {capi.SCENE_BUFFER_TRIANGLES: ((triangle_count, 12), np.uint32), capi.SCENE_BUFFER_WIDE8_SLOTS: ((slot_count, 16), np.uint32), capi.SCENE_BUFFER_NODES: ((node_count, 16), np.uint32),
                        capi.SCENE_BUFFER_TRACE_TRIANGLES: ((triangle_count, 12), np.uint32), capi.SCENE_BUFFER_SHADE_TRIANGLES: ((triangle_count, 32), np.uint32),
                        capi.SCENE_BUFFER_TRIANGLE_CLASS: ((triangle_count,), np.uint8), capi.SCENE_BUFFER_MATERIALS: ((material_count, 16), np.uint32),
                        capi.SCENE_BUFFER_INSTANCES: ((instance_count, 20), np.uint32)}.get(which, ((0,), np.uint8))
        out = np.zeros(shape, dtype)
        self._check(self.lib.hipr_debug_read_scene_buffer(self.handle, int(which), C.c_void_p(out.ctypes.data), out.nbytes), "hipr_debug_read_scene_buffer")
        return out

    def set_scene_state(self, state: capi.HiprSceneState):
        self._check(self.lib.hipr_set_scene_state(self.handle, C.byref(state)), "hipr_set_scene_state")

    def set_frame(self, width, height, tile_phase=0, tile_stride=1, samples_per_pass=1):
        f = capi.HiprFrameDesc(width, height, tile_phase, tile_stride, samples_per_pass)
        self._check(self.lib.hipr_set_frame(self.handle, C.byref(f)), "hipr_set_frame")
        self.frame = f

    def set_entry_point(self, entry: int):
        self._check(self.lib.hipr_set_entry_point(self.handle, entry), "hipr_set_entry_point")

    def use_scratch_accumulation(self, on: bool):
        self._check(self.lib.hipr_use_scratch_accumulation(self.handle, int(on)), "hipr_use_scratch_accumulation")

    def owned_pixel_count(self) -> int:
        n = C.c_uint32()
        self._check(self.lib.hipr_owned_pixel_count(self.handle, C.byref(n)), "hipr_owned_pixel_count")
        return n.value

    def render_pass(self, camera: capi.HiprCameraState, out_ptr: int = 0, out_pitch: int = 0, synchronize: bool = False):
        self._check(self.lib.hipr_render_pass(self.handle, C.byref(camera), C.c_void_p(out_ptr), out_pitch, int(synchronize)), "hipr_render_pass")

    def set_samples_per_pass(self, samples: int):
        self._check(self.lib.hipr_set_samples_per_pass(self.handle, samples), "hipr_set_samples_per_pass")
        self.frame.samples_per_pass = samples

    def trace_pass(self, camera: capi.HiprCameraState):
        self._check(self.lib.hipr_trace_pass(self.handle, C.byref(camera)), "hipr_trace_pass")

    def accumulate_samples(self, first_sample: int, sample_count: int, first_accumulation: int, out_ptr: int = 0, out_pitch: int = 0, synchronize: bool = False):
        self._check(self.lib.hipr_accumulate_samples(self.handle, first_sample, sample_count, first_accumulation, C.c_void_p(out_ptr), out_pitch, int(synchronize)),
                    "hipr_accumulate_samples")

    def synchronize(self):
        self._check(self.lib.hipr_synchronize(self.handle), "hipr_synchronize")

    def read_accumulation(self) -> np.ndarray:
        f = self.frame
        if f.tile_stride == 1:
            out = np.zeros((f.height, f.width, 4), np.float64)
        else:
            out = np.zeros((self.owned_pixel_count(), 4), np.float64)
        self._check(self.lib.hipr_read_accumulation(self.handle, out.ctypes.data_as(C.POINTER(C.c_double)), out.size // 4), "hipr_read_accumulation")
        return out

    def counters(self) -> dict:
        c = capi.HiprCounters()
        self._check(self.lib.hipr_get_counters(self.handle, C.byref(c)), "hipr_get_counters")
        return {name: int(getattr(c, name)) for name, _ in capi.HiprCounters._fields_}

    def reset_counters(self):
        self._check(self.lib.hipr_reset_counters(self.handle), "hipr_reset_counters")

    def set_instrumentation(self, on: bool):
        self._check(self.lib.hipr_set_instrumentation(self.handle, int(on)), "hipr_set_instrumentation")

    def reset_timers(self):
        self._check(self.lib.hipr_reset_timers(self.handle), "hipr_reset_timers")

    def wavefront_count(self) -> int:
        n = C.c_int()
        self._check(self.lib.hipr_get_wavefront_count(self.handle, C.byref(n)), "hipr_get_wavefront_count")
        return n.value

    def set_wavefront_count(self, count: int):
        self._check(self.lib.hipr_set_wavefront_count(self.handle, count), "hipr_set_wavefront_count")

    def trace_variant(self) -> int:
        """capi.TRACE_BVH2 / TRACE_WIDE_PERSISTENT / TRACE_EXHAUSTIVE for the uploaded scene."""
        v = C.c_int(0)
        self._check(self.lib.hipr_get_trace_variant(self.handle, C.byref(v)), "hipr_get_trace_variant")
        return v.value

    def set_trace_variant(self, variant: int):
        """Forces a search for the scenes uploaded after the call (-1: by scene size)."""
        self._check(self.lib.hipr_set_trace_variant(self.handle, int(variant)), "hipr_set_trace_variant")

    def set_backface_culling(self, enable: bool):
        self._check(self.lib.hipr_set_backface_culling(self.handle, int(enable)), "hipr_set_backface_culling")

    def set_pass_pipelining(self, enable: bool):
        self._check(self.lib.hipr_set_pass_pipelining(self.handle, int(enable)), "hipr_set_pass_pipelining")

    def trace_is_fused(self) -> bool:
        return self.trace_variant() in (capi.TRACE_WIDE_PERSISTENT, capi.TRACE_WIDE8_PERSISTENT)

    def oracle_search(self) -> int:
        """The `use_bvh` mode of the oracle that states the same search: 0 exhaustive, 1 BVH2, 2 compressed 4-wide BVH, 3 compressed 8-wide BVH with leaf records."""
        return {capi.TRACE_BVH2: 1, capi.TRACE_WIDE_PERSISTENT: 2, capi.TRACE_EXHAUSTIVE: 0, capi.TRACE_WIDE8_PERSISTENT: 3}[self.trace_variant()]

    def kernel_times(self) -> dict:
        t = capi.HiprKernelTimes()
        self._check(self.lib.hipr_get_kernel_times(self.handle, C.byref(t)), "hipr_get_kernel_times")
        return {name: dict(ms=t.milliseconds[i], launches=int(t.launches[i])) for i, name in enumerate(capi.HIPR_KERNEL_NAMES)}

    def valu_issue_rates(self) -> dict:
        """Wave64 instructions per second device-wide of v_fma_f32 / v_max_f32 / v_cvt_f32_ubyte1 chains (hipr_debug_valu_issue_rates)."""
        out = (C.c_double * 3)()
        self._check(self.lib.hipr_debug_valu_issue_rates(self.handle, out), "hipr_debug_valu_issue_rates")
        return {"v_fma_f32": out[0], "v_max_f32": out[1], "v_cvt_f32_ubyte1": out[2]}

    def scatter_tiles(self, compact_ptr, rank_stride, rank_count, width, height, out_ptr, out_pitch):
        self._check(self.lib.hipr_scatter_tiles(self.handle, C.c_void_p(compact_ptr), rank_stride, rank_count, width, height, C.c_void_p(out_ptr), out_pitch),
                    "hipr_scatter_tiles")

    # ---- stage-level parity entry points -------------------------------------------------------
    def debug_generate(self, camera, accumulation):
        n = self.owned_pixel_count()
        o = np.zeros((n, 4), np.float32); d = np.zeros((n, 4), np.float32); px = np.zeros(n, np.uint32)
        fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        self._check(self.lib.hipr_debug_generate(self.handle, C.byref(camera), accumulation, o.ctypes.data_as(fp), d.ctypes.data_as(fp), px.ctypes.data_as(up)),
                    "hipr_debug_generate")
        return o, d, px

    def debug_shading(self, shading_model, params10, wo, inputs, mode=0):
        """mode 0: sample(wo, u) -> (n, 7) f, pdf, direction; mode 1: evaluate_with_PDF(wo, wi) -> (n, 7) f, pdf, 0, 0, 0."""
        inputs = np.ascontiguousarray(inputs, np.float32).reshape(-1, 3)
        wo = np.ascontiguousarray(np.broadcast_to(np.asarray(wo, np.float32), inputs.shape))
        params = np.ascontiguousarray(params10, np.float32)
        out = np.zeros((len(inputs), 7), np.float32)
        fp = C.POINTER(C.c_float)
        self._check(self.lib.hipr_debug_shading(self.handle, int(shading_model), params.ctypes.data_as(fp), wo.ctypes.data_as(fp), inputs.ctypes.data_as(fp), len(inputs),
                                                int(mode), out.ctypes.data_as(fp)), "hipr_debug_shading")
        return out

    def debug_shade(self, camera, rays, throughput_bounces, hits, last_triangle, pixel_hash, accumulation):
        """hipr_debug_shade: shade_path for n queue entries of the uploaded scene -> (n, 32) records (include/hiprenderer_c.h)."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n = len(rays)
        throughput_bounces = np.ascontiguousarray(throughput_bounces, np.float32).reshape(n, 4)
        hits = np.ascontiguousarray(hits, np.float32).reshape(n, 4)
        words = [np.ascontiguousarray(a, np.uint32).reshape(n) for a in (last_triangle, pixel_hash, accumulation)]
        out = np.zeros((n, 32), np.float32)
        fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        self._check(self.lib.hipr_debug_shade(self.handle, C.byref(camera), n, rays.ctypes.data_as(fp), throughput_bounces.ctypes.data_as(fp), hits.ctypes.data_as(fp),
                                              *[a.ctypes.data_as(up) for a in words], out.ctypes.data_as(fp)), "hipr_debug_shade")
        return out

    def debug_light(self, light: capi.HiprLight, position, inputs, mode=0):
        """mode 0: sample_radiance(light, position, u = inputs[:, :2]) -> (n, 8) radiance, PDF, direction, distance;
        mode 1 (spot lights): evaluate and pdf for the directions in `inputs` -> (n, 8) radiance, pdf, 0, 0, 0, 0."""
        inputs = np.ascontiguousarray(inputs, np.float32)
        if inputs.ndim == 2 and inputs.shape[1] == 2:
            inputs = np.concatenate([inputs, np.zeros((len(inputs), 1), np.float32)], axis=1)
        inputs = np.ascontiguousarray(inputs.reshape(-1, 3))
        position = np.ascontiguousarray(position, np.float32)
        out = np.zeros((len(inputs), 8), np.float32)
        fp = C.POINTER(C.c_float)
        self._check(self.lib.hipr_debug_light(self.handle, C.byref(light), position.ctypes.data_as(fp), inputs.ctypes.data_as(fp), len(inputs), int(mode), out.ctypes.data_as(fp)),
                    "hipr_debug_light")
        return out

    def debug_sobol(self, triples):
        triples = np.ascontiguousarray(triples, np.uint32).reshape(-1, 3)
        out = np.zeros((len(triples), 4), np.uint32)
        up = C.POINTER(C.c_uint32)
        self._check(self.lib.hipr_debug_sobol(self.handle, triples.ctypes.data_as(up), len(triples), out.ctypes.data_as(up)), "hipr_debug_sobol")
        return out

    def debug_sample_offsets(self):
        out = np.zeros((256, 4), np.float32)
        self._check(self.lib.hipr_debug_sample_offsets(self.handle, out.ctypes.data_as(C.POINTER(C.c_float))), "hipr_debug_sample_offsets")
        return out

    def debug_trace_closest(self, rays, skip=None):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        hits = np.zeros((len(rays), 4), np.float32)
        fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        sk = np.ascontiguousarray(skip, np.uint32).ctypes.data_as(up) if skip is not None else None
        self._check(self.lib.hipr_debug_trace_closest(self.handle, rays.ctypes.data_as(fp), sk, len(rays), hits.ctypes.data_as(fp)), "hipr_debug_trace_closest")
        return hits

    def debug_trace_shadow(self, rays):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros(len(rays), np.float32)
        fp = C.POINTER(C.c_float)
        self._check(self.lib.hipr_debug_trace_shadow(self.handle, rays.ctypes.data_as(fp), len(rays), out.ctypes.data_as(fp)), "hipr_debug_trace_shadow")
        return out

    def debug_classify_hits(self, hits, coat_classes=False, grid=0):
        """The listing pass of a bounce on the given (n, 4) hits -> order (n,): the queue entry the shade kernel takes at each place (hipr_debug_classify_hits)."""
        hits = np.ascontiguousarray(hits, np.float32).reshape(-1, 4)
        order = np.zeros(len(hits), np.uint32)
        self._check(self.lib.hipr_debug_classify_hits(self.handle, hits.ctypes.data_as(C.POINTER(C.c_float)), len(hits), int(bool(coat_classes)), int(grid),
                                                      order.ctypes.data_as(C.POINTER(C.c_uint32))), "hipr_debug_classify_hits")
        return order

    def debug_trace_fused(self, closest_rays, skip, shadow_rays):
        """One fused launch over both queues, as a bounce makes it: -> (hits (n_closest, 4), transmittance (n_shadow,)). Either set of rays may be empty."""
        closest_rays = np.ascontiguousarray(closest_rays, np.float32).reshape(-1, 8)
        shadow_rays = np.ascontiguousarray(shadow_rays, np.float32).reshape(-1, 8)
        hits = np.zeros((len(closest_rays), 4), np.float32)
        out = np.zeros(len(shadow_rays), np.float32)
        fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        if skip is not None:
            skip = np.ascontiguousarray(skip, np.uint32)
            assert len(skip) == len(closest_rays)
        sk = skip.ctypes.data_as(up) if skip is not None else None
        self._check(self.lib.hipr_debug_trace_fused(self.handle, closest_rays.ctypes.data_as(fp), sk, len(closest_rays), shadow_rays.ctypes.data_as(fp), len(shadow_rays),
                                                    hits.ctypes.data_as(fp), out.ctypes.data_as(fp)), "hipr_debug_trace_fused")
        return hits, out

    def debug_trace_hinted(self, mode, closest_rays, skip, shadow_rays, hints):
        """hipr_debug_trace_hinted: the closest-only (mode 0), shadow-only (1) or fused (2) launch over the 8-wide tree with the hint table `hints` (uint32 words, tag | record
        slot) -> (hits (n_closest, 4), transmittance (n_shadow,), the table as the launch left it, the resident tree's tag)."""
        closest_rays = np.ascontiguousarray(closest_rays, np.float32).reshape(-1, 8)
        shadow_rays = np.ascontiguousarray(shadow_rays, np.float32).reshape(-1, 8)
        hints = np.array(hints, np.uint32).reshape(-1)      # a copy: the call writes it
        hits = np.zeros((len(closest_rays), 4), np.float32)
        out = np.zeros(len(shadow_rays), np.float32)
        tag = C.c_uint32(0)
        fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        if skip is not None:
            skip = np.ascontiguousarray(skip, np.uint32)
            assert len(skip) == len(closest_rays)
        sk = skip.ctypes.data_as(up) if skip is not None else None
        self._check(self.lib.hipr_debug_trace_hinted(self.handle, int(mode), closest_rays.ctypes.data_as(fp), sk, len(closest_rays), shadow_rays.ctypes.data_as(fp), len(shadow_rays),
                                                     hints.ctypes.data_as(up), len(hints), hits.ctypes.data_as(fp), out.ctypes.data_as(fp), C.byref(tag)), "hipr_debug_trace_hinted")
        return hits, out, hints, tag.value
