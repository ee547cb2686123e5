"""hipr_update_scene_texels without a GPU: the bodies of csrc/texel_update.h compiled for the host (tests/native/TexelUpdateHost.hip) and walked the way the three
passes walk them -- rectangle writes, the flags of the affected materials' triangles decided again, the leaf pass -- must leave, byte for byte, what
SceneBuilder::update_texels leaves, and that in turn what a builder made anew from the edited image builds: flags, trace flag words, leaf bits, the texel pool."""
import numpy as np
import pytest

import material_update_bindings as mu
import texel_update_bindings as tu
from bifrost3d_amd import capi


def assert_held_equals(held, scene, what):
    d = scene.desc
    trace, shade, classes = mu.derived_arrays(scene)
    assert np.array_equal(held["triangles"], scene.triangles()), what
    assert np.array_equal(held["trace"], trace) and np.array_equal(held["shade"], shade) and np.array_equal(held["classes"], classes), what
    assert np.array_equal(held["slots"], scene.wide8_slots()), what
    assert np.array_equal(held["texels"], np.ctypeslib.as_array(d.texels, shape=(d.texel_bytes,))), what


@pytest.mark.parametrize("name", tu.CASE_IDS)
def test_the_passes_leave_what_the_builder_leaves(name):
    _, v, steps = tu.case(name)
    scene, info = tu.make_scene(v)
    held = tu.arrays_of(scene)
    image = info["images"]["coverage"]
    for edits, expectation in steps:
        before = tu.opaque(scene, info)
        listed = tu.coverage_edits(info, edits)
        answer = tu.run_kernel_bodies(scene, held, listed)
        assert scene.update_texels(listed) is True
        after = tu.opaque(scene, info)
        tu.check_expectation(expectation, before, after)
        assert_held_equals(held, scene, "against SceneBuilder::update_texels")
        for x, y, pixels in edits:
            image = tu.painted(image, x, y, pixels)
        anew, _ = tu.make_scene(v, dict(coverage=image))
        assert_held_equals(held, anew, "against a builder made anew")
        # the books: every triangle of the quad -- the one model whose material leaves its flags to the texture -- is decided again, and the AND is the scene's
        assert answer["changed"] == int((before != after).sum()) and answer["decided"] == len(info["quad"])
        assert answer["all_opaque"] == bool((scene.triangles()[:, 11] & capi.TRIANGLE_OPAQUE != 0).all())


@pytest.mark.parametrize("tint", [tu.R32F, tu.RGBA32F], ids=["r32f", "rgba32f"])
def test_a_float_tint_texture_lands_in_the_pool_and_changes_no_flag(tint):
    v = tu.variant(tint=tint)
    scene, info = tu.make_scene(v)
    held = tu.arrays_of(scene)
    pixels = np.random.default_rng(9).uniform(0.0, 2.0, (3, 5) if tint == tu.R32F else (3, 5, 4)).astype(np.float32)
    edits = [(info["textures"]["tint"], 2, 4, pixels)]
    answer = tu.run_kernel_bodies(scene, held, edits)
    assert scene.update_texels(edits) is True
    assert_held_equals(held, scene, "against SceneBuilder::update_texels")
    anew, _ = tu.make_scene(v, dict(tint=tu.painted(info["images"]["tint"], 2, 4, pixels)))
    assert_held_equals(held, anew, "against a builder made anew")
    assert answer["decided"] == 0 and answer["changed"] == 0 and answer["all_opaque"]


def test_a_pitch_beyond_the_row_and_two_textures_in_one_call():
    _, v, _ = tu.case("hole_nearest_r8")
    scene, info = tu.make_scene(v)
    held = tu.arrays_of(scene)
    wide = np.full((4, 11), 77, np.uint8)       # rows of 11 bytes of which 6 are the rectangle's
    wide[:, :6] = np.arange(24, dtype=np.uint8).reshape(4, 6)
    other = np.full((2, 3, 4), 9, np.uint8)
    edits = [(info["textures"]["coverage"], 21, 2, 6, 4, wide, 11), (info["textures"]["unrelated"], 13, 14, other)]
    tu.run_kernel_bodies(scene, held, edits)
    assert scene.update_texels(edits) is True
    assert_held_equals(held, scene, "against SceneBuilder::update_texels")
    unrelated = tu.UNRELATED.copy()
    unrelated[14:16, 13:16] = other
    d = scene.desc
    pool = np.ctypeslib.as_array(d.texels, shape=(d.texel_bytes,))
    at = lambda index: d.textures[index].texel_offset
    assert np.array_equal(pool[at(info["textures"]["unrelated"]):][:unrelated.size], unrelated.reshape(-1))
    assert np.array_equal(pool[at(info["textures"]["coverage"]):][:32 * 32].reshape(32, 32), tu.painted(info["images"]["coverage"], 21, 2, wide[:, :6]))
    assert 77 not in pool[at(info["textures"]["coverage"]):][:32 * 32]


def test_the_builder_refuses_what_the_device_refuses():
    _, v, _ = tu.case("hole_nearest_r8")
    scene, info = tu.make_scene(v)
    before = tu.arrays_of(scene)
    texture, one = info["textures"]["coverage"], np.zeros((1, 1), np.uint8)
    refused = [[(0, 0, 0, one)], [(scene.desc.texture_count, 0, 0, one)], [(texture, 32, 0, one)], [(texture, 0, 32, one)], [(texture, 31, 0, np.zeros((1, 2), np.uint8))],
               [(texture, 0, 30, np.zeros((3, 1), np.uint8))], [(texture, 0, 0, 0, 1, one, 1)], [(texture, 0, 0, 1, 0, one, 1)], [(texture, 0, 0, 4, 1, np.zeros((1, 4), np.uint8), 3)],
               [(texture, 0, 0, 1, 1, None, 1)]]
    for edits in refused:
        assert scene.update_texels(edits) is False, edits
    after = tu.arrays_of(scene)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    # a texture added since the last build is not the device's yet
    added = scene.add_texture(one, 1, 1, tu.R8)
    assert scene.update_texels([(added, 0, 0, one)]) is False


def test_every_triangle_whose_flag_differs_is_decided_again():
    """The "never miss" rule, on 2 000 random triangles with coordinates in [-3, 3] and random rectangles, over every wrap and filter combination: a triangle whose
    flag differs between a builder of the image before and one of the image after must be among the triangles the flag pass decides again -- and come out with the
    flag of the builder made anew."""
    rng = np.random.default_rng(20261021)
    size, triangle_count = 32, 2000
    uv = rng.uniform(-3.0, 3.0, (triangle_count, 3, 2)).astype(np.float32)
    small = rng.random(triangle_count) < 0.8      # most triangles small enough for a box of at most 64 texels
    uv[small, 1:] = uv[small, :1] + rng.uniform(-0.4, 0.4, (int(small.sum()), 2, 2)).astype(np.float32)
    positions = np.zeros((triangle_count * 3, 3), np.float32)
    positions[:, :2] = uv.reshape(-1, 2) * 0.01
    mesh = dict(positions=positions, primitives=np.arange(triangle_count * 3, dtype=np.uint32).reshape(-1, 3), normals=np.tile(np.array([0, 0, -1], np.float32), (triangle_count * 3, 1)),
                texcoords=uv.reshape(-1, 2))
    import pool_growth_bindings as pg
    from bifrost3d_amd.host import Scene
    missed_nothing = 0
    for repeat in (False, True):
        for linear in (False, True):
            # about a tenth of the texels fail before, so that flags go both ways
            image = np.where(rng.random((size, size)) < 0.1, 0, 255).astype(np.uint8)

            def build(pixels):
                scene = Scene("cornell", param0=4)
                texture = scene.add_texture(pixels, size, size, tu.R8, repeat=(repeat, repeat), linear=(linear, linear))
                material = scene.add_material(pg.material(flags=capi.MATERIAL_THIN_WALLED | capi.MATERIAL_CUTOUT, coverage=0.5, coverage_texture=texture))
                scene.insert_model(1000, scene.add_mesh(**mesh), material, model_index=202, **pg.BESIDE_IT)
                scene.rebuild()
                return scene, texture

            scene, texture = build(image)
            for _ in range(6):
                w, h = int(rng.integers(1, 9)), int(rng.integers(1, 9))
                x, y = int(rng.integers(0, size - w + 1)), int(rng.integers(0, size - h + 1))
                pixels = np.where(rng.random((h, w)) < 0.5, 0, 255).astype(np.uint8)
                held = tu.arrays_of(scene)
                flags_before = held["triangles"][:, 11].copy()
                answer = tu.run_kernel_bodies(scene, held, [(texture, x, y, pixels)])
                image = tu.painted(image, x, y, pixels)
                anew, _ = build(image)
                differing = np.nonzero(anew.triangles()[:, 11] != flags_before)[0]
                assert answer["decided"] == triangle_count and answer["changed"] == len(differing), (repeat, linear, x, y, w, h)
                assert np.array_equal(held["triangles"], anew.triangles()) and np.array_equal(held["slots"], anew.wide8_slots())
                missed_nothing += len(differing)
                assert scene.update_texels([(texture, x, y, pixels)]) is True
    assert missed_nothing > 0      # flags did differ: the property was put to the test
