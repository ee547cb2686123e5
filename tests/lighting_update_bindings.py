"""What the tests of hipr_update_scene_lighting share (csrc/environment_build.h, SceneBuilder::set_lights / staged_environment_build / adopt_lighting): the
environment maps -- the smallest shapes at which each pass of the build can go wrong, made here with numpy --, the light lists, the host path's scenes, a host
scene's environment by name, and the host build of the routines (tests/native/EnvironmentBuildHost.hip).

The yardstick of every case is the host path: SceneBuilder::add_light, InfiniteAreaLight + presample_environment + set_environment, rebuild(), byte for byte."""
import ctypes as C
from pathlib import Path

import numpy as np

import device_rebuild_bindings as rb
import instance_edit_bindings as ie
from bifrost3d_amd import capi

CORNELL = ie.CORNELL      # 184 triangles and 88 BVH2 nodes: the 8-wide search


def _float_map(width, height, seed):
    """Positive RGBA32F texels with a bright spot: every row and column gets its own weight."""
    rng = np.random.default_rng(seed)
    pixels = rng.uniform(0.05, 1.5, (height, width, 4)).astype(np.float32)
    pixels[height // 3, width // 2, :3] += np.float32(40.0)
    pixels[..., 3] = 1.0
    return pixels


def _one_white_texel(width, height):
    pixels = np.zeros((height, width, 4), np.uint8)
    pixels[..., 3] = 255
    pixels[height // 2, width // 3] = 255
    return pixels


def _bytes_map(width, height, seed):
    pixels = np.random.default_rng(seed).integers(0, 256, (height, width, 4), dtype=np.uint8)
    pixels[..., 3] = 255
    return pixels


# name -> the keywords of Scene.add_environment but the sample count. linear = (magnification, minification), repeat = (u, v).
MAPS = {
    # lower than 128 rows: resampled through sample2D (bilinear), then blurred
    "64x32_float_linear": dict(pixels=_float_map(64, 32, 1), width=64, height=32, texel_format=capi.TEXEL_RGBA32F, linear=(True, True), repeat=(True, False)),
    # no resample, no blur, an odd width, rows past four bands of the row sums
    "67x130_float_nearest": dict(pixels=_float_map(67, 130, 2), width=67, height=130, texel_format=capi.TEXEL_RGBA32F, linear=(False, False), repeat=(True, False)),
    # one white texel amid black: rows whose total is zero (no division there), the sRGB table, a blur that spreads the texel
    "65x128_srgb_one_white": dict(pixels=_one_white_texel(65, 128), width=65, height=128, texel_format=capi.TEXEL_RGBA8, is_sRGB=True, linear=(True, True), repeat=(True, False)),
    # the blur's left = right = x
    "1x1_float_linear": dict(pixels=np.array([[[0.5, 0.25, 2.0, 1.0]]], np.float32), width=1, height=1, texel_format=capi.TEXEL_RGBA32F, linear=(True, True), repeat=(True, True)),
    "1x128_bytes_linear": dict(pixels=_bytes_map(1, 128, 3), width=1, height=128, texel_format=capi.TEXEL_RGBA8, linear=(True, True), repeat=(False, False)),
    # the edges of a 64-column tile
    "63x129_float_nearest": dict(pixels=_float_map(63, 129, 4), width=63, height=129, texel_format=capi.TEXEL_RGBA32F, linear=(False, False), repeat=(True, False)),
    "64x129_bytes_nearest_min_linear": dict(pixels=_bytes_map(64, 129, 5), width=64, height=129, texel_format=capi.TEXEL_RGBA8, linear=(False, True), repeat=(False, True)),
    "65x129_float_linear": dict(pixels=_float_map(65, 129, 6), width=65, height=129, texel_format=capi.TEXEL_RGBA32F, linear=(True, False), repeat=(True, True)),
    # the disabled form: no PDF image, one sample, no light appended
    "32x16_all_black": dict(pixels=np.zeros((16, 32, 4), np.float32), width=32, height=16, texel_format=capi.TEXEL_RGBA32F, linear=(True, True), repeat=(True, False)),
}
MAP_IDS = list(MAPS)
# (map, sample count): every map at 1024 samples as the procedural sky, the two extremes on one map each
BUILDS = [(name, 1024) for name in MAP_IDS] + [("67x130_float_nearest", 2), ("64x32_float_linear", 8192)]
BUILD_IDS = [f"{name}-{count}" for name, count in BUILDS]


def sphere_light(position, power=(6.0, 5.0, 4.0), radius=0.03) -> capi.HiprLight:
    light = capi.HiprLight()
    light.data[0:7] = [*power, *position, radius]
    light.flags = capi.LIGHT_SPHERE
    return light


def spot_light(position, direction, power=(9.0, 9.0, 7.0), radius=0.02, cos_angle=0.8) -> capi.HiprLight:
    d = np.asarray(direction, np.float32) / np.float32(np.linalg.norm(np.asarray(direction, np.float32)))
    light = capi.HiprLight()
    light.data[0:11] = [*power, *position, radius, *[float(v) for v in d], cos_angle]
    light.flags = capi.LIGHT_SPOT
    return light


def directional_light(direction, radiance=(1.5, 1.4, 1.2)) -> capi.HiprLight:
    d = np.asarray(direction, np.float32) / np.float32(np.linalg.norm(np.asarray(direction, np.float32)))
    light = capi.HiprLight()
    light.data[0:6] = [*radiance, *[float(v) for v in d]]
    light.flags = capi.LIGHT_DIRECTIONAL
    return light


def own_lights(scene) -> list:
    """A host scene's lights without the presampled environment's."""
    return [light for light in scene.lights() if (light.flags & capi.LIGHT_TYPE_MASK) != capi.LIGHT_PRESAMPLED_ENVIRONMENT]


def light_lists(scene) -> dict:
    """The lists of the cases, from the lights the scene starts with (the Cornell box: its one ceiling light)."""
    start = own_lights(scene)
    inside = (0.1, 0.25, -0.2)
    return {
        "a light added": start + [sphere_light(inside)],
        "one removed": start[:-1],
        "a type changed": start[:-1] + [spot_light((start[-1].data[3], start[-1].data[4], start[-1].data[5]), (0.1, -1.0, 0.05))],
        "zero lights": [],
        "33 lights": start + [sphere_light((-0.3 + 0.02 * k, 0.1 + 0.01 * k, -0.25), power=(0.2, 0.25, 0.3), radius=0.005) for k in range(32)],
        "a directional among them": start + [directional_light((0.2, -1.0, 0.3)), sphere_light(inside)],
    }


LIST_IDS = ["a light added", "one removed", "a type changed", "zero lights", "33 lights", "a directional among them"]


def host_scene(arguments, lights=None, environment=None, sample_count=1024):
    """The yardstick: a scene built by the host path alone. `environment` (a name of MAPS) goes in by InfiniteAreaLight + presample_environment + set_environment,
    then rebuild(); `lights` (None: the scene's own) as with_lights describes them."""
    scene = rb.make_scene(arguments)
    if environment is not None:
        scene.add_environment(sample_count=sample_count, **MAPS[environment])
        scene.rebuild()
    return scene if lights is None else with_lights(scene, lights)


class _Described:
    """A host scene under another light list: its description with `lights` (the presampled environment's appended last, by set_environment's rule), as
    hipr_upload_scene takes it. Quacks like a Scene where the tests and Context.upload_scene need one."""

    def __init__(self, scene, lights):
        self.scene, self.state, self.camera = scene, scene.state, scene.camera
        d = scene.desc
        lights = list(lights)
        if d.environment and d.environment.contents.sample_count > 1:
            environment_light = capi.HiprLight()
            environment_light.flags = capi.LIGHT_PRESAMPLED_ENVIRONMENT
            lights.append(environment_light)
        self._lights = (capi.HiprLight * max(len(lights), 1))(*lights)
        self.desc = capi.HiprSceneDesc.from_buffer_copy(bytes(d))
        self.desc.lights, self.desc.light_count = self._lights, len(lights)


def with_lights(scene, lights):
    return _Described(scene, lights)


def environment_of(desc) -> dict:
    """The environment of a description by name, as words: None without one."""
    if not desc.environment:
        return None
    e = desc.environment.contents
    return dict(map=e.environment_map_ID, extent=(e.pdf_width, e.pdf_height, e.sample_count),
                pdf=np.ctypeslib.as_array(C.cast(e.per_pixel_PDF, C.POINTER(C.c_uint32)), shape=(e.pdf_width * e.pdf_height,)).copy(),
                samples=np.ctypeslib.as_array(C.cast(e.samples, C.POINTER(C.c_uint32)), shape=(e.sample_count, 8)).copy())


def expected_switches(desc) -> int:
    """ResidentScene::derive_switches_from_pools restated over a description: an environment, a presampled environment light or a float texture pick the generic
    samplers; a material that references a texture, or any of those, the textured shade kernel."""
    lights = [desc.lights[k].flags & capi.LIGHT_TYPE_MASK for k in range(desc.light_count)]
    formats = [desc.textures[k].format for k in range(1, desc.texture_count)]
    environment = bool(desc.environment) or capi.LIGHT_PRESAMPLED_ENVIRONMENT in lights or capi.TEXEL_R32F in formats or capi.TEXEL_RGBA32F in formats
    materials = [desc.materials[k] for k in range(desc.material_count)]
    textures = environment or any(m.tint_roughness_texture_ID or m.roughness_texture_ID or m.metallic_texture_ID or m.coverage_texture_ID for m in materials)
    return (capi.SWITCH_TEXTURES if textures else 0) | (capi.SWITCH_ENVIRONMENT if environment else 0)


LIGHTING_BUFFERS = (capi.SCENE_BUFFER_LIGHTS, capi.SCENE_BUFFER_ENVIRONMENT_PDF, capi.SCENE_BUFFER_ENVIRONMENT_SAMPLES)
LIGHTING_NAMES = ("lights", "environment PDF", "environment samples")


def lighting_buffers(context) -> list:
    return [context.read_scene_buffer(which) for which in LIGHTING_BUFFERS]


def unequal_lighting(a, b) -> list:
    return [name for name, x, y in zip(LIGHTING_NAMES, a, b) if x.shape != y.shape or not np.array_equal(x, y)]


# ---- the host build of the routines (tests/native/EnvironmentBuildHost.hip) ----
LIB_PATH = Path(__file__).resolve().parent / "native" / "libenvironment_build_host.so"
_lib = None


def library():
    global _lib
    if _lib is None:
        assert LIB_PATH.exists(), f"{LIB_PATH} is missing: run __graft_entry__.build()"
        _lib = C.CDLL(str(LIB_PATH))
        _lib.build_host_environment.argtypes = [C.POINTER(capi.HiprTexture), C.c_void_p, C.POINTER(capi.HiprEnvironmentBuild), C.POINTER(C.c_float), C.c_uint64, C.POINTER(capi.HiprLightSample),
                                                C.c_uint32, C.POINTER(capi.HiprLightingResult)]
    return _lib


def routines_build(scene, texture_index: int, build) -> dict:
    """build_host_environment over texture `texture_index` of a host scene's pools and the staged description `build`: the dict Context.update_scene_lighting returns
    for a build (without light_count and switches, which are the entry point's)."""
    d = scene.desc
    texture = d.textures[texture_index]
    texels = np.ctypeslib.as_array(d.texels, shape=(d.texel_bytes,))[texture.texel_offset:].copy()
    pdf = np.zeros(texture.width * build.pdf_height, np.float32)
    samples = np.zeros((build.sample_count, 8), np.float32)
    result = capi.HiprLightingResult()
    status = library().build_host_environment(C.byref(texture), C.c_void_p(texels.ctypes.data), C.byref(build), pdf.ctypes.data_as(C.POINTER(C.c_float)), len(pdf),
                                              C.cast(samples.ctypes.data, C.POINTER(capi.HiprLightSample)), len(samples), C.byref(result))
    if status != 0:
        return dict(status=status)
    return dict(status=0, result=result, pdf_width=result.pdf_width, pdf_height=result.pdf_height, sample_count=result.sample_count, disabled=bool(result.importance_sampling_disabled),
                per_pixel_PDF=np.ascontiguousarray(pdf[:result.pdf_width * result.pdf_height]), samples=np.ascontiguousarray(samples[:result.sample_count]))
