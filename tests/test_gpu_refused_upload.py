"""hipr_upload_scene runs every argument check before it touches the device: a refused description leaves the resident scene's arrays, its search and its
images as they were. Beside test_gpu_device_refit.py::test_refusals_leave_everything_as_it_was, whose frame (64 x 36, 4 bounces) and `render` this uses."""
import ctypes as C

import numpy as np
import pytest

from bifrost3d_amd import capi
from bifrost3d_amd.host import Scene
from bifrost3d_amd.renderer import Context
from test_gpu_device_refit import render

pytestmark = pytest.mark.gpu


def test_a_refused_upload_leaves_the_resident_scene_as_it_was():
    """The refused description is no larger than the resident one in any pool (53 / 114 / 126 / 64 against 88 / 184 / 168 / 73 nodes / triangles / indices /
    vertices, equal elsewhere), so no buffer would have had to grow for it either: what is compared is what an upload that checks too late overwrites.
    The read-backs are compared before the second render: a scene that was overwritten fails there and renders nothing."""
    ctx = Context(0)
    try:
        scene = Scene("cornell", param0=4, environment=True)
        ctx.upload_scene(scene)
        variant = ctx.trace_variant()
        before = render(ctx, scene, spp=1)
        triangles, slots = ctx.read_scene_buffer(capi.SCENE_BUFFER_TRIANGLES), ctx.read_scene_buffer(capi.SCENE_BUFFER_WIDE8_SLOTS)
        smaller = Scene("cornell", param0=3, environment=True)
        resident, refused = scene.desc, smaller.desc
        for pool in ("node_count", "triangle_count", "index_count", "vertex_count", "instance_count", "material_count", "light_count", "texture_count", "texel_bytes"):
            assert getattr(refused, pool) <= getattr(resident, pool), pool
        environment = capi.HiprEnvironment.from_buffer_copy(refused.environment.contents)
        environment.environment_map_ID = 0
        broken = capi.HiprSceneDesc.from_buffer_copy(refused)
        broken.environment = C.pointer(environment)
        assert ctx.lib.hipr_upload_scene(ctx.handle, C.byref(broken)) == capi.HIPR_ERROR_INVALID_ARGUMENT
        assert ctx.trace_variant() == variant
        assert np.array_equal(ctx.read_scene_buffer(capi.SCENE_BUFFER_TRIANGLES), triangles) and np.array_equal(ctx.read_scene_buffer(capi.SCENE_BUFFER_WIDE8_SLOTS), slots)
        assert np.array_equal(render(ctx, scene, spp=1).view(np.uint64), before.view(np.uint64))
    finally:
        ctx.close()
