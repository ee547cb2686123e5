"""The kernels' texture, coverage and environment lookups held to a PLAIN statement of a lookup (tests/texture_reference.py) and, where the arithmetic is exact, to the
oracle bit for bit -- through what the C-ABI already returns: hipr_debug_trace_shadow on the four searches (the generic coverage sampler and the R8-only one of the
8-wide kernel), hipr_debug_shade in both arithmetic modes (cut-out decisions, the environment through the miss program), the tint and roughness AOVs, one exact
path-traced frame, and the triangle flags the device holds after an upload and after a material edit. The inputs, their excluded shares and the non-vacuity of the
rule's cases are checked without a GPU in tests/test_texture_lookups_cpu.py; every case here is a few thousand rays or 64 x 36 frames."""
import functools
import os

import numpy as np
import pytest

import texture_lookup_cases as tc
import texture_reference as ref
from bifrost3d_amd import capi
from conftest import verification_build_equals_oracle
from device_host_bindings import oracle_shade

pytestmark = pytest.mark.gpu

EIGHT_BIT = (capi.TEXEL_R8, capi.TEXEL_RGBA8)
FAST_POW = 1e-5      # relative: the bound tests/test_gpu_verify_build.py puts on the fast unit's pow (test_specified_transcendentals_on_the_device)
SEARCHES = {"exhaustive": capi.TRACE_EXHAUSTIVE, "bvh2": capi.TRACE_BVH2, "wide4": capi.TRACE_WIDE_PERSISTENT, "wide8": capi.TRACE_WIDE8_PERSISTENT}


@pytest.fixture(scope="module")
def ctx():
    from bifrost3d_amd.renderer import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def exact_oracle():
    """The oracle with the tables as uploaded (unorm16) and the specified f64 transcendentals: the exact mode's checker."""
    from oracle_bindings import get_oracle
    o = get_oracle(True)
    before = o.lib.oracle_set_f64_transcendentals(1)
    yield o
    o.lib.oracle_set_f64_transcendentals(before)


@pytest.fixture(scope="module")
def coverage_scenes():
    return tc.coverage_scenes()


def uploaded_with(ctx, scene, variant):
    ctx.set_trace_variant(variant)
    try:
        ctx.upload_scene(scene)
    finally:
        ctx.set_trace_variant(-1)
    assert ctx.trace_variant() == variant


def closest_without_skip(ctx, rays):
    """hipr_debug_trace_closest with no triangle for a ray to skip."""
    return ctx.debug_trace_closest(rays, np.full(len(rays), 0xFFFFFFFF, np.uint32))


# ---- shadow kernels ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("search", list(SEARCHES))
def test_shadow_kernels_against_the_oracle_and_the_reference(ctx, exact_oracle, coverage_scenes, search):
    """hipr_debug_trace_shadow of each search -- the exhaustive kernel on the scenes of two-triangle quads, the BVH2, 4-wide and 8-wide kernels on the tessellated ones --
    through every texture size, format, addressing mode and filter value under texture coordinates inside and far outside [0, 1]: the oracle's transmittance bit for
    bit, and 1 - coverage of the reference at the device's own hit within the lookup's tolerance."""
    for number, (quads, rays) in enumerate(coverage_scenes["two_triangle_quads" if search == "exhaustive" else "tessellated_quads"]):
        uploaded_with(ctx, quads, SEARCHES[search])
        got = ctx.debug_trace_shadow(rays)
        theirs, _ = exact_oracle.trace_shadow(quads.desc, rays, use_bvh=ctx.oracle_search())
        assert np.array_equal(got.view(np.uint32), theirs.view(np.uint32)), (search, number, int((got != theirs).sum()))
        expected, tolerance, excluded = tc.expected_transmittance(functools.partial(closest_without_skip, ctx), tc.Pools(quads.desc), rays)
        tc.held_to_reference(f"gpu shadow {search}[{number}]", got, expected, tolerance, excluded)


def test_the_r8_coverage_sampler_gives_the_generic_samplers_bits(ctx, exact_oracle):
    """A pool of nothing but single-channel linear coverage textures runs k_trace_wide8<..., COVERAGE_R8 = true>; one RGBA8 coverage material elsewhere in the scene puts
    the same quads under the generic sampler. Same rays at the R8 quads: the same bits both times, the oracle's, and the reference's values.

    Which of the two ran is not observable through the C-ABI. The test relies on launch_wide8's rule (csrc/hiprenderer.hip): the R8 instantiation serves a shadow launch
    when instrumentation is off (a new context's state), HIPR_LEAN_TRACE is not 0, some triangle is not flagged opaque, and ResidentScene::derive_switches_from_pools
    found every material's coverage texture HIPR_TEXEL_R8 and not sRGB. What of that the test can see, it asserts; were the rule to change, both uploads would run the
    generic sampler, which test_shadow_kernels_against_the_oracle_and_the_reference holds to the reference on its own."""
    specs = tc.texture_specs(formats=(capi.TEXEL_R8,), srgb=(False,))
    entries = tc.coverage_entries(specs)
    rgba8 = dict(width=5, height=7, texel_format=capi.TEXEL_RGBA8, is_sRGB=False, repeat=(True, True), linear=(True, False), salt=3)
    other = (rgba8, lambda t: tc.material(coverage=0.75, coverage_texture=t), dict(u_range=tc.RANGES["signed"]))
    r8_only, with_rgba8 = tc.QuadScene(entries, cells=tc.TESSELLATION), tc.QuadScene(entries + [other], cells=tc.TESSELLATION)
    assert os.environ.get("HIPR_LEAN_TRACE", "1") != "0"
    for quads, every_coverage_texture_r8 in ((r8_only, True), (with_rgba8, False)):
        pools = tc.Pools(quads.desc)
        coverage_textures = [pools.textures[m.coverage_texture_ID] for m in pools.materials if m.coverage_texture_ID]
        assert coverage_textures and all(t.format == capi.TEXEL_R8 and not t.is_sRGB for t in coverage_textures) == every_coverage_texture_r8
        assert ((pools.triangles[:, 11] & capi.TRIANGLE_OPAQUE) == 0).any()
    rays = tc.rays_at_quads(r8_only.quads, 12, 31)
    results = []
    for quads in (r8_only, with_rgba8):
        uploaded_with(ctx, quads, capi.TRACE_WIDE8_PERSISTENT)
        got = ctx.debug_trace_shadow(rays)
        theirs, _ = exact_oracle.trace_shadow(quads.desc, rays, use_bvh=3)
        assert np.array_equal(got.view(np.uint32), theirs.view(np.uint32))
        expected, tolerance, excluded = tc.expected_transmittance(functools.partial(closest_without_skip, ctx), tc.Pools(quads.desc), rays)
        tc.held_to_reference(f"gpu shadow wide8, pool {'R8 only' if quads is r8_only else 'R8 and one RGBA8'}", got, expected, tolerance, excluded)
        results.append(got)
    assert np.array_equal(results[0].view(np.uint32), results[1].view(np.uint32))
    assert len(np.unique(results[0])) > 100      # not a comparison of constants


# ---- hipr_debug_shade in both arithmetic modes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", ["eight_bit", "every_format"])
def test_cutout_decisions_of_both_shade_units(ctx, verify_ctx, exact_oracle, pool):
    """The cut-out hits of the CPU leg through hipr_debug_shade: an 8-bit pool runs k_shade<..., TEXTURES = 1>, a pool with float textures the generic samplers. The exact
    mode's records equal the oracle's bit for bit, and its decisions follow the reference; the fast mode's decisions are asserted where the reference's texel is at
    least 2 / 255 from the threshold."""
    quads = tc.QuadScene(tc.cutout_entries(tc.texture_specs(formats=EIGHT_BIT) if pool == "eight_bit" else tc.texture_specs()))
    pools = tc.Pools(quads.desc)
    entries = tc.chosen_hits(quads, 40, 17)
    camera = quads.camera(64, 36, accumulations=3, max_bounce_count=4)
    triangles, u, v = entries[2][:, 3].view(np.uint32), entries[2][:, 1], entries[2][:, 2]
    cover, _, excluded = tc.expected_coverage(pools, triangles, u, v)
    assert excluded.mean() <= 0.01
    theirs = oracle_shade(exact_oracle, quads, camera, *entries)
    verify_ctx.upload_scene(quads)
    exact = verify_ctx.debug_shade(camera, *entries)
    assert tc.same_bits(exact, theirs).all(), (pool, int((~tc.same_bits(exact, theirs).all(axis=1)).sum()))
    wrong = (tc.decisions(exact) != (cover == 1.0)) & ~excluded
    assert not wrong.any(), (pool, "exact", int(wrong.sum()))
    # the fast unit: its division and contraction may move a filtered texel by rounding errors, never by 2 / 255
    near_threshold = np.zeros(len(cover), bool)
    materials = pools.material_of(triangles)
    uv = pools.texcoord(triangles, u, v)
    for index in np.unique(materials):
        m = pools.materials[index]
        chosen = materials == index
        texel = ref.sample(pools.textures[m.coverage_texture_ID], pools.texels, uv[chosen])[:, 0]
        near_threshold[chosen] = np.abs(texel - float(m.coverage)) < 2.0 / 255.0
    ctx.upload_scene(quads)
    fast = tc.decisions(ctx.debug_shade(camera, *entries))
    wrong = (fast != (cover == 1.0)) & ~excluded & ~near_threshold
    print(f"LOOKUPS gpu cut-out decisions {pool}: {len(cover)} hits, exact records equal the oracle's, fast decisions against the reference {int(wrong.sum())}, "
          f"excluded share {excluded.mean():.5f}, within 2/255 of the threshold {near_threshold.mean():.5f}")
    assert not wrong.any(), (pool, "fast", int(wrong.sum()))
    assert (~near_threshold).mean() > 0.9


def environment_cases():
    from bifrost3d_amd.host import Scene
    return {"procedural_sky": lambda: Scene("cornell", environment=True),
            "constructed_repeat_clamp": lambda: tc.constructed_environment(Scene("cornell"), (True, False)),
            "constructed_clamp_clamp": lambda: tc.constructed_environment(Scene("cornell"), (False, False)),
            "constructed_repeat_repeat": lambda: tc.constructed_environment(Scene("cornell"), (True, True)),
            "constructed_nearest": lambda: tc.constructed_environment(Scene("cornell"), (True, False), bilinear=False, size=tc.NEAREST_ENVIRONMENT_MAP)}


@pytest.mark.parametrize("case", list(environment_cases()))
def test_escaped_rays_of_both_shade_units(ctx, verify_ctx, exact_oracle, case):
    """The miss entries of the CPU leg through hipr_debug_shade: the exact mode's records equal the oracle's bit for bit, every one of them,
    and both modes add the reference's environment -- alone under a delta BSDF PDF, weighted p / (p + pdf) under the reference's own."""
    scene = environment_cases()[case]()
    tint = [float(c) for c in scene.state.environment_tint]
    e = scene.desc.environment.contents
    directions = tc.environment_directions((e.pdf_width, e.pdf_height), 1500, 5)
    camera = scene.camera(64, 36, accumulations=3, max_bounce_count=4)
    verify_ctx.upload_scene(scene)
    ctx.upload_scene(scene)
    for kind, d in directions.items():
        for with_mis in (False, True):
            share = 0.01 if kind == "random" else None
            given, alternatives, tolerance, excluded = tc.expected_environment(scene.desc, tint, d, with_mis)
            entries = tc.miss_entries(d, given)
            theirs = oracle_shade(exact_oracle, scene, camera, *entries)
            exact = verify_ctx.debug_shade(camera, *entries)
            differing = np.where(~tc.same_bits(exact, theirs).all(axis=1))[0]
            print(f"LOOKUPS gpu environment {case} {kind} mis {int(with_mis)} exact: {len(differing)} of {len(d)} records differ from the oracle's")
            assert len(differing) == 0, (case, kind, with_mis, [(d[k].tolist(), exact[k].view(np.uint32).tolist(), theirs[k].view(np.uint32).tolist()) for k in differing[:4]])
            tc.held_to_reference(f"gpu environment {case} {kind} mis {int(with_mis)} exact", exact[:, 1:4], tc.nearest_alternative(exact[:, 1:4], alternatives), tolerance,
                                 np.broadcast_to(excluded[:, None], tolerance.shape), allowed_share=share)
            given, alternatives, tolerance, excluded = tc.expected_environment(scene.desc, tint, d, with_mis, srgb_relative=FAST_POW)
            fast = ctx.debug_shade(camera, *entries)
            assert (np.ascontiguousarray(fast[:, 0]).view(np.uint32) == 0).all()
            tc.held_to_reference(f"gpu environment {case} {kind} mis {int(with_mis)} fast", fast[:, 1:4], tc.nearest_alternative(fast[:, 1:4], alternatives), tolerance,
                                 np.broadcast_to(excluded[:, None], tolerance.shape), allowed_share=share)


# ---- the tint and roughness AOVs ------------------------------------------------------------------------------------------------------------------------------
def one_r32f_texture(scene):
    scene.add_texture(tc.pixels_of(5, 7, capi.TEXEL_R32F), 5, 7, capi.TEXEL_R32F, False, (True, True), (True, True))


AOV_POOLS = {"eight_bit": lambda: tc.QuadScene(tc.tint_entries(tc.texture_specs(formats=EIGHT_BIT))),
             "eight_bit_and_one_r32f": lambda: tc.QuadScene(tc.tint_entries(tc.texture_specs(formats=EIGHT_BIT)), extra=one_r32f_texture),      # a float texture: TEXTURES = 2
             "every_format": lambda: tc.QuadScene(tc.tint_entries(tc.texture_specs()))}


@pytest.mark.parametrize("pool", list(AOV_POOLS))
def test_tint_and_roughness_images_of_both_shade_units(ctx, verify_ctx, exact_oracle, pool):
    """1 spp through the tint and the roughness entry over white materials, 64 x 36 frames each over a block of quads: a pixel whose first hit (hipr_debug_generate +
    hipr_debug_trace_closest) is a quad shows the reference's RGB / A in both arithmetic modes, and the exact mode's image equals the oracle's."""
    quads = AOV_POOLS[pool]()
    pools = tc.Pools(quads.desc)
    width, height = tc.FRAME
    for context, mode in ((verify_ctx, "exact"), (ctx, "fast")):
        context.upload_scene(quads)
        context.set_frame(width, height, 0, 1, 1)
        for entry, channels in ((capi.ENTRY_TINT, slice(0, 3)), (capi.ENTRY_ROUGHNESS, slice(3, 4))):
            got, expected, tolerance, excluded = [], [], [], []
            for camera in tc.frame_cameras(len(quads.quads)):
                o, d, px = context.debug_generate(camera, 0)
                valid = px != 0xFFFFFFFF      # the ray queue is padded to whole blocks
                assert valid.sum() == width * height
                o, d, px = o[valid], d[valid], px[valid]
                rays = np.concatenate([o[:, :3], np.zeros((len(o), 1), np.float32), d[:, :3], np.full((len(o), 1), np.inf, np.float32)], axis=1)
                hits = closest_without_skip(context, rays)
                on, value, allowed, near = tc.expected_tint_roughness(pools, hits, srgb_relative=FAST_POW if mode == "fast" else None)
                context.set_entry_point(entry)
                try:
                    context.render_pass(camera, synchronize=True)
                    image = context.read_accumulation()
                finally:
                    context.set_entry_point(capi.ENTRY_PATH_TRACING)
                if mode == "exact":
                    theirs, _, _ = exact_oracle.render(quads.desc, quads.state, camera, width, height, 1, use_bvh=context.oracle_search(), entry=entry)
                    assert np.array_equal(image[..., :3], theirs[..., :3]), (pool, entry)
                shown = image[(px >> 16).astype(np.int64), (px & 0xFFFF).astype(np.int64)][:, :3][:, channels if entry == capi.ENTRY_TINT else slice(0, 1)]
                got.append(shown[on]); expected.append(value[on][:, channels]); tolerance.append(allowed[on][:, channels]); excluded.append(near[on])
            got, expected, tolerance, excluded = (np.concatenate(a) for a in (got, expected, tolerance, excluded))
            assert len(got) > 0.5 * len(tc.frame_cameras(len(quads.quads))) * width * height
            tc.held_to_reference(f"gpu aov {pool} entry {entry} {mode}", got, expected, tolerance, np.broadcast_to(excluded[:, None], got.shape))


def test_a_path_traced_frame_over_eight_bit_textures_equals_the_oracle(verify_ctx, exact_oracle):
    """The only way the samplers of k_shade<..., TEXTURES = 1> outside the AOV branch show in an image: tint-roughness and coverage textures of the 8-bit formats under
    the Cornell box's light, 64 x 36 at 4 spp in the exact mode, every pixel the oracle's."""
    specs = tc.texture_specs(formats=EIGHT_BIT)[:32]
    entries = [(spec, (lambda t, k=k: tc.material(tint_texture=t, coverage_texture=t if k % 2 else 0, coverage=0.8, tint=(0.9, 0.8, 0.7), roughness=0.7)), dict(u_range=tc.RANGES[name]))
               for k, (spec, name) in enumerate(zip(specs, list(tc.RANGES) * 11))]
    quads = tc.QuadScene(entries)
    width, height = tc.FRAME

    class Framed:      # the scene under a free camera over its block of quads: what verification_build_equals_oracle reads of a scene
        desc, state = quads.desc, quads.state

        @staticmethod
        def camera(w, h, accumulations=0, max_bounce_count=4, **_):
            return tc.free_camera(w, h, (0.0, 0.5, -6.0), accumulations, max_bounce_count)

    image = verification_build_equals_oracle(verify_ctx, exact_oracle, Framed, width, height, 4, 4, "eight-bit textures")
    assert np.isfinite(image).all() and (image > 0).mean() > 0.2


# ---- the flags the device holds ---------------------------------------------------------------------------------------------------------------------------------
def test_flags_on_the_device_are_the_hosts_after_an_upload_and_after_a_material_edit(ctx):
    """HiprTriangle::flags as hipr_upload_scene leaves them, and after a hipr_update_scene_materials that gives a quad's material another coverage texture (the hole
    somewhere else): the host builder's, which the CPU leg holds to the reference. The edit must change flags, or it shows nothing."""
    entries = tc.rule_entries()
    quads = tc.QuadScene(entries, cells=tc.TESSELLATION)
    ctx.upload_scene(quads)
    before = ctx.read_scene_buffer(capi.SCENE_BUFFER_TRIANGLES)
    assert np.array_equal(before, quads.scene.triangles())
    names = [q["spec"]["name"] for q in quads.quads]
    first, second = names.index("plain left_border wrap (True, True) bilinear True unit"), names.index("plain top_border wrap (True, True) bilinear True unit")
    materials = quads.scene.materials()
    edited = materials[quads.quads[first]["material"]]
    edited.coverage_texture_ID = quads.quads[second]["texture"]
    changes = [(quads.quads[first]["material"], edited)]
    ctx.update_scene_materials(changes)
    assert quads.scene.update_materials(changes)
    after = ctx.read_scene_buffer(capi.SCENE_BUFFER_TRIANGLES)
    assert np.array_equal(after, quads.scene.triangles())
    assert not np.array_equal(after[:, 11], before[:, 11]) and np.array_equal(after[:, :11], before[:, :11])
