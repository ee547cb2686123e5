"""hipr_validate_scene is the preflight hipr_upload_scene runs before it touches the device (no GPU): what an upload refuses for the description alone,
hipr_validate_scene refuses too. The index checks are in test_coverage_cpu.py (test_validate_scene_rejects_out_of_range_indices), whose `_mutated` pattern
this reuses: a copy of the description with one array replaced by a changed copy."""
import ctypes as C

from bifrost3d_amd import capi
from bifrost3d_amd.host import Scene
from test_coverage_cpu import _mutated


def refused(lib, d, what):
    status = lib.hipr_validate_scene(C.byref(d))
    message = lib.hipr_last_error().decode()
    assert status == capi.HIPR_ERROR_INVALID_ARGUMENT and what in message, (status, message)


def test_an_incomplete_environment_is_refused():
    lib = capi.load_library()
    scene = Scene("cornell", param0=3, environment=True)
    desc = scene.desc
    assert desc.environment and lib.hipr_validate_scene(C.byref(desc)) == 0

    def set_field(name, value):
        def mutate(array):
            setattr(array[0], name, value)
        return mutate

    fp, sp = type(desc.environment.contents.per_pixel_PDF), type(desc.environment.contents.samples)
    for name, value in [("environment_map_ID", 0), ("environment_map_ID", desc.texture_count), ("per_pixel_PDF", fp()), ("samples", sp()), ("sample_count", 0), ("pdf_width", 0)]:
        d, keep = _mutated(desc, "environment", 1, capi.HiprEnvironment, set_field(name, value))      # a copy of the environment with one field changed
        refused(lib, d, "environment")


def test_a_flagged_attribute_without_its_pool_is_refused():
    lib = capi.load_library()
    scene = Scene("opacity", param0=8)
    desc = scene.desc
    assert any(desc.instances[i].mesh_flags & 2 for i in range(desc.instance_count))      # HIPR_MESH_TEXCOORDS
    d = capi.HiprSceneDesc()
    C.memmove(C.byref(d), C.byref(desc), C.sizeof(capi.HiprSceneDesc))
    d.texcoords = type(desc.texcoords)()
    refused(lib, d, "attribute whose pool is null")
