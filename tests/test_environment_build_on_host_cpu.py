"""The routines of hipr_update_scene_lighting's environment build (csrc/environment_build.h) walked on the CPU in the kernels' shape -- tiles, one virtual thread per
element, the threads of every launch taken backwards (tests/native/EnvironmentBuildHost.hip) -- over the tables SceneBuilder::staged_environment_build makes, held
to the host path byte for byte: InfiniteAreaLight + presample_environment + set_environment. And SceneBuilder::set_lights / adopt_lighting held to rebuild()."""
import numpy as np
import pytest

import device_rebuild_bindings as rb
import lighting_update_bindings as lu
from bifrost3d_amd import capi


def staged_scene(name):
    """A built scene that holds the map's texture and no environment: what is resident before the build."""
    scene = rb.make_scene(lu.CORNELL)
    m = lu.MAPS[name]
    index = scene.add_texture(m["pixels"], m["width"], m["height"], m["texel_format"], m.get("is_sRGB", False), repeat=m["repeat"], linear=m["linear"])
    scene.rebuild()
    return scene, index


@pytest.mark.parametrize("name, sample_count", lu.BUILDS, ids=lu.BUILD_IDS)
def test_the_walk_leaves_what_the_host_path_leaves(name, sample_count):
    host = lu.host_scene(lu.CORNELL, environment=name, sample_count=sample_count)
    scene, index = staged_scene(name)
    build = scene.staged_environment_build(index, sample_count)
    assert build is not None and build.sample_count == max(2, sample_count) and build.pdf_height == max(lu.MAPS[name]["height"], 128)
    assert (build.srgb_decode is not None and bool(build.srgb_decode)) == bool(lu.MAPS[name].get("is_sRGB", False))
    walked = lu.routines_build(scene, index, build)
    assert walked["status"] == 0
    expected = lu.environment_of(host.desc)
    assert expected["map"] == index
    assert (walked["pdf_width"], walked["pdf_height"], walked["sample_count"]) == expected["extent"]
    black = name == "32x16_all_black"
    assert walked["disabled"] == black and (expected["extent"] == (1, 1, 1)) == black
    assert np.array_equal(walked["per_pixel_PDF"].view(np.uint32), expected["pdf"])
    assert np.array_equal(walked["samples"].view(np.uint32), expected["samples"])
    if not black:
        assert np.isfinite(walked["per_pixel_PDF"]).all() and walked["per_pixel_PDF"].max() > 0 and (walked["samples"][:, 7] == np.float32(1e30)).all()
    # the adoption: the builder's description follows without a rebuild
    assert scene.adopt_lighting(lu.own_lights(scene), capi.ENVIRONMENT_BUILD, index, walked)
    assert rb.differences(rb.description(host), rb.description(scene)) == []
    adopted = lu.environment_of(scene.desc)
    assert adopted["map"] == index and adopted["extent"] == expected["extent"] and np.array_equal(adopted["pdf"], expected["pdf"]) and np.array_equal(adopted["samples"], expected["samples"])


def test_the_walk_refuses_what_the_entry_point_refuses():
    scene, index = staged_scene("65x128_srgb_one_white")
    build = scene.staged_environment_build(index, 64)
    assert lu.routines_build(scene, index, build)["status"] == 0
    for field, value in (("pdf_height", 129), ("sample_count", 48), ("sample_count", 1), ("srgb_decode", None)):
        bad = capi.HiprEnvironmentBuild.from_buffer_copy(bytes(build))
        setattr(bad, field, value)
        assert lu.routines_build(scene, index, bad)["status"] == -1, field
    assert scene.staged_environment_build(0, 64) is None and scene.staged_environment_build(index + 1, 64) is None


@pytest.mark.parametrize("which", lu.LIST_IDS)
def test_set_lights_leaves_what_a_rebuild_over_the_list_leaves(which):
    for environment in (None, "64x32_float_linear"):
        scene = lu.host_scene(lu.CORNELL, environment=environment)
        lights = lu.light_lists(scene)[which]
        expected = lu.with_lights(lu.host_scene(lu.CORNELL, environment=environment), lights).desc
        before = rb.description(scene)
        assert scene.set_lights(lights)
        after = rb.description(scene)
        assert [k for k in rb.differences(before, after) if k not in ("lights", "scalars")] == []
        assert scene.desc.light_count == expected.light_count == len(lights) + (1 if environment else 0)
        assert np.array_equal(after["lights"], rb.words(expected.lights, expected.light_count, 12))
        if environment:
            assert scene.desc.lights[scene.desc.light_count - 1].flags == capi.LIGHT_PRESAMPLED_ENVIRONMENT
        # a rebuild afterwards changes nothing: the description was whole
        scene.rebuild()
        assert rb.differences(after, rb.description(scene)) == []


def test_adopt_lighting_removes_and_keeps_and_refuses():
    scene = lu.host_scene(lu.CORNELL, environment="67x130_float_nearest")
    plain = rb.make_scene(lu.CORNELL)
    lights = lu.own_lights(scene)
    environment_light = capi.HiprLight()
    environment_light.flags = capi.LIGHT_PRESAMPLED_ENVIRONMENT
    before = rb.description(scene)
    assert not scene.adopt_lighting(lights + [environment_light], capi.ENVIRONMENT_KEEP) and not scene.set_lights([environment_light]) and not scene.adopt_lighting(lights, 3)
    assert rb.differences(before, rb.description(scene)) == []
    assert scene.adopt_lighting(lights, capi.ENVIRONMENT_KEEP) and rb.differences(before, rb.description(scene)) == []
    assert scene.adopt_lighting(lights, capi.ENVIRONMENT_REMOVE)
    assert lu.environment_of(scene.desc) is None and scene.desc.light_count == plain.desc.light_count == len(lights)
    assert np.array_equal(rb.description(scene)["lights"], rb.description(plain)["lights"])
