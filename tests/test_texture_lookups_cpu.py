"""The oracle and the host build of the device's shade stage held to a PLAIN statement of a texture lookup (tests/texture_reference.py: numpy, float64, no text shared with
either), where every other test compares them with each other: the software samplers (csrc/kernels.h sample_texture / fetch_texel / wrap_coord / wrap_next), the
latitude-longitude environment lookups and the upload-time rule covered_everywhere (csrc/material_rules.h). tests/test_gpu_texture_lookups.py holds the kernels to the same
reference and to the oracle bit for bit; this leg is where the inputs are checked: the excluded shares, the non-vacuity of the rule's cases."""
import numpy as np
import pytest

import texture_lookup_cases as tc
import texture_reference as ref
from bifrost3d_amd import capi


# ---- shadow transmittance: 1 - coverage through every texture, on every search -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def coverage_scenes():
    return tc.coverage_scenes()


@pytest.mark.parametrize("search", [0, 1, 2, 3])
@pytest.mark.parametrize("which", ["two_triangle_quads", "tessellated_quads"])
def test_shadow_transmittance_is_one_minus_the_reference_coverage(oracle, coverage_scenes, which, search):
    """oracle.trace_shadow on the exhaustive, BVH2, 4-wide and 8-wide searches, rays aimed at random points of quads that carry every texture size, format, addressing mode
    and filter value under texture coordinates in [0, 1], [-3.25, 2.5] and [5, 8]: the transmittance is 1 - coverage of the reference at the hit, whose (u, v) come
    from trace_closest on the same ray and whose corner coordinates come from the description's pools."""
    shares = []
    for number, (quads, rays) in enumerate(coverage_scenes[which]):
        pools = tc.Pools(quads.desc)
        expected, tolerance, excluded = tc.expected_transmittance(lambda r: oracle.trace_closest(quads.desc, r, None, use_bvh=search, with_lights=False)[0], pools, rays)
        got, _ = oracle.trace_shadow(quads.desc, rays, use_bvh=search)
        shares.append(tc.held_to_reference(f"cpu shadow {which}[{number}] search {search}", got, expected, tolerance, excluded))
    assert max(shares) <= 0.01


# ---- the upload-time rule: a triangle flagged HIPR_TRIANGLE_OPAQUE is covered everywhere ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rule_scene():
    return tc.QuadScene(tc.rule_entries(), cells=tc.TESSELLATION)


def triangles_by_quad(quads, pools):
    """{quad number: its triangles of the description}: instance k of the scene is quad k's."""
    assert len(pools.instances) == len(quads.quads)
    instance = pools.triangles[:, 9]
    return {k: np.where(instance == k)[0] for k in range(len(quads.quads))}


def test_triangles_flagged_opaque_are_covered_wherever_the_reference_looks(rule_scene):
    """SOUNDNESS of covered_everywhere as the host builder applied it: over every flagged triangle of the tessellated quads the reference's coverage is 1 on a 33 x 33
    barycentric lattice plus corners and edge midpoints -- also with the boundary of the lattice displaced by the 2^-13 texel the device's f32 interpolation may add.
    NON-VACUITY: every constructed hole leaves triangles unflagged, among them a neighbour that does not hold the hole itself; and at least a quarter of the triangles
    the reference finds solid are flagged."""
    pools = tc.Pools(rule_scene.desc)
    lattice = tc.barycentric_lattice()
    boundary = lattice[(lattice[:, 0] == 0) | (lattice[:, 1] == 0) | (np.abs(lattice.sum(axis=1) - 1.0) < 1e-12)]
    solid_triangles = flagged_solid = 0
    for k, triangles in triangles_by_quad(rule_scene, pools).items():
        spec = rule_scene.quads[k]["spec"]
        assert len(triangles) == 2 * tc.TESSELLATION ** 2
        flagged = (pools.flags_of(triangles) & capi.TRIANGLE_OPAQUE) != 0
        cover = tc.lattice_coverage(pools, triangles, lattice)
        displaced = tc.lattice_coverage(pools, triangles, boundary, displacement_texels=2.0 ** -13)
        solid = (cover == 1.0).all(axis=1) & (displaced == 1.0).all(axis=1)
        assert solid[flagged].all(), (spec["name"], "flagged triangles the reference finds open somewhere", triangles[flagged & ~solid][:8].tolist())
        solid_triangles += int(solid.sum())
        flagged_solid += int((flagged & solid).sum())
        if spec["hole"] is not None:
            assert (~solid).any(), (spec["name"], "the hole shows in no triangle")
            assert (~flagged & solid).any(), (spec["name"], "no solid neighbour of the hole was left to the sampler: the rule's margin is not exercised")
        else:
            assert flagged.all(), (spec["name"], "a texture without a hole covers every triangle")
    print(f"LOOKUPS cpu rule: {flagged_solid} of {solid_triangles} solid triangles flagged ({flagged_solid / solid_triangles:.3f})")
    assert flagged_solid >= 0.25 * solid_triangles


def test_flagged_triangles_keep_the_margin_the_rule_documents(rule_scene):
    """What the soundness test cannot see: the rule's header promises that EVERY texel under the bounding box of the corners' coordinates passes, with a texel of slack on
    every side for the interpolation's rounding, plus the bilinear neighbour. Stated here in float64 from that sentence (the box shrunk by 2^-13 texel where a corner sits
    on a texel edge: there f32 may take either side): no flagged triangle has the hole inside its promised box. A rule that gives up the slack on one side is still sound
    in exact arithmetic, so only this test notices."""
    pools = tc.Pools(rule_scene.desc)
    eps = 2.0 ** -13
    checked = 0
    for k, triangles in triangles_by_quad(rule_scene, pools).items():
        spec = rule_scene.quads[k]["spec"]
        if spec["hole"] is None:
            continue
        texture = pools.textures[rule_scene.quads[k]["texture"]]
        bilinear = ref.is_bilinear(texture)
        flagged = triangles[(pools.flags_of(triangles) & capi.TRIANGLE_OPAQUE) != 0]
        t = pools.corner_texcoords(flagged)
        inside = np.ones(len(flagged), bool)
        for axis, (n, repeat) in enumerate(((int(texture.width), bool(texture.wrap_u)), (int(texture.height), bool(texture.wrap_v)))):
            low, high = t[:, :, axis].min(axis=1) * n, t[:, :, axis].max(axis=1) * n
            offset = 0.5 if bilinear else 0.0
            first = np.floor(low - offset + eps).astype(np.int64) - 1
            last = np.floor(high - offset - eps).astype(np.int64) + (1 if bilinear else 0) + 1
            touched = np.zeros(len(flagged), bool)
            for step in range(int((last - first).max()) + 1 if len(flagged) else 0):
                texel = first + step
                touched |= (texel <= last) & (ref.address(texel, n, repeat) == spec["hole"][axis])
            inside &= touched
        checked += len(flagged)
        assert not inside.any(), (spec["name"], "flagged although the hole lies in the box the rule promises to check", flagged[inside][:8].tolist())
    assert checked > 1000


# ---- the tint and roughness AOVs: RGB and A of every format ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tint_scene():
    return tc.QuadScene(tc.tint_entries(tc.texture_specs()))


@pytest.mark.parametrize("entry, channels", [(capi.ENTRY_TINT, slice(0, 3)), (capi.ENTRY_ROUGHNESS, slice(3, 4))])
def test_tint_and_roughness_images_show_the_reference_texels(oracle, tint_scene, entry, channels):
    """oracle.render at 1 spp through the tint / roughness entry over white materials of roughness 1: a pixel whose first hit (generate_rays + trace_closest) is a quad shows
    the reference's RGB / A there -- all four formats, sRGB on three channels and never on alpha, every addressing mode and filter value."""
    pools = tc.Pools(tint_scene.desc)
    width, height = tc.FRAME
    got, expected, tolerance, excluded = [], [], [], []
    for camera in tc.frame_cameras(len(tint_scene.quads)):
        o, d = oracle.generate_rays(camera, width, height, 0, tc.all_pixels())
        rays = np.concatenate([o[:, :3], np.zeros((len(o), 1), np.float32), d[:, :3], np.full((len(o), 1), np.inf, np.float32)], axis=1)
        hits, _ = oracle.trace_closest(tint_scene.desc, rays, None, use_bvh=1, with_lights=True)
        on, value, allowed, near = tc.expected_tint_roughness(pools, hits)
        image, _, _ = oracle.render(tint_scene.desc, tint_scene.state, camera, width, height, 1, use_bvh=1, entry=entry)
        shown = image.reshape(-1, 4)[:, :3][:, channels if entry == capi.ENTRY_TINT else slice(0, 1)]
        got.append(shown[on]); expected.append(value[on][:, channels]); tolerance.append(allowed[on][:, channels]); excluded.append(near[on])
    got, expected, tolerance, excluded = (np.concatenate(a) for a in (got, expected, tolerance, excluded))
    assert len(got) > 0.5 * len(tc.frame_cameras(len(tint_scene.quads))) * width * height      # the frames are full of quads
    tc.held_to_reference(f"cpu aov entry {entry}", got, expected, tolerance, np.broadcast_to(excluded[:, None], got.shape))


# ---- the shade stage: cut-out decisions and the environment, on the oracle and on the host build of the device code -------------------------------------------------
def shade_units(oracle, scene, instantiations):
    """{name: shade(camera, *entries) -> records} of the oracle's hit programs and of the device's shade_path compiled for the host in the given TEXTURES instantiations."""
    from device_host_bindings import DeviceShadeOnHost, oracle_shade
    device = DeviceShadeOnHost(scene)
    units = {"oracle": lambda camera, *entries: oracle_shade(oracle, scene, camera, *entries)}
    for textures in instantiations:
        units[f"host build TEXTURES={textures}"] = lambda camera, *entries, textures=textures: device.shade(camera, *entries, models=7 if textures == 2 else 1, textures=textures)      # the instantiations built: <7, 2> and <1, 1>; every material here is Default
    return units, device


@pytest.mark.parametrize("pool, instantiations", [("eight_bit", (1, 2)), ("every_format", (2,))])
def test_cutout_decisions_follow_the_reference_comparison(oracle, pool, instantiations):
    """oracle_debug_shade and the host build of the device's shade_path (the 8-bit-only sampler where the pool allows it, and the generic one) on hits with chosen
    barycentrics over cut-out materials: a hit is shaded where the reference's texel is not below the threshold, and rejected -- the same ray sent on -- where it is.
    The triangles' corners carry (0, 0), (A, 0), (0, B) with A, B powers of two of either sign, so the coordinates reach far below zero and the lookups are exact."""
    specs = tc.texture_specs(formats=(capi.TEXEL_R8, capi.TEXEL_RGBA8)) if pool == "eight_bit" else tc.texture_specs()
    quads = tc.QuadScene(tc.cutout_entries(specs))
    pools = tc.Pools(quads.desc)
    entries = tc.chosen_hits(quads, 40, 17)
    triangles, u, v = entries[2][:, 3].view(np.uint32), entries[2][:, 1], entries[2][:, 2]
    cover, _, excluded = tc.expected_coverage(pools, triangles, u, v)
    assert 0.2 < cover.mean() < 0.8 and (pools.texcoord(triangles, u, v) < -1.0).any()      # both decisions, and coordinates below zero
    units, device = shade_units(oracle, quads, instantiations)
    try:
        for name, shade in units.items():
            shaded = tc.decisions(shade(quads.camera(64, 36, accumulations=3, max_bounce_count=4), *entries))
            wrong = (shaded != (cover == 1.0)) & ~excluded
            print(f"LOOKUPS cpu cut-out decisions {pool} {name}: {int((~excluded).sum())} decisions, {int(wrong.sum())} against the reference, excluded share {excluded.mean():.5f}")
            assert excluded.mean() <= 0.01 and not wrong.any(), (name, int(wrong.sum()), triangles[wrong][:8].tolist())
    finally:
        device.close()


def environment_cases():
    from bifrost3d_amd.host import Scene
    cases = {"procedural_sky": lambda: Scene("cornell", environment=True)}
    for repeat in ((True, False), (False, False), (True, True), (False, True)):
        cases[f"constructed_repeat_{int(repeat[0])}{int(repeat[1])}"] = lambda repeat=repeat: tc.constructed_environment(Scene("cornell"), repeat)
    cases["constructed_nearest"] = lambda: tc.constructed_environment(Scene("cornell"), (True, False), bilinear=False, size=tc.NEAREST_ENVIRONMENT_MAP)
    return cases


@pytest.mark.parametrize("case", list(environment_cases()))
def test_escaped_rays_take_the_reference_environment(oracle, case):
    """Miss entries of debug_shade on the oracle and on the host build of the device code: with a delta BSDF PDF the radiance added is tint * the reference's sample at
    ((atan2(z, x) + pi) / 2 pi, (asin(y) + pi / 2) / pi); with the reference's own PDF as the ray's it is that times p / (p + pdf), pdf = per_pixel_PDF[clamped
    nearest] / sqrt(1 - y^2). Random directions, the poles (whose PDF is the delta -0 and weighs nothing), the seam (-1, 0, +-0), the axes, the plane x = 0 and the
    texel edges of the PDF image; the procedural sky, and an 8 x 4 RGBA32F map under every addressing combination."""
    scene = environment_cases()[case]()
    state = scene.state
    tint = [float(c) for c in state.environment_tint]
    e = scene.desc.environment.contents
    directions = tc.environment_directions((e.pdf_width, e.pdf_height), 1500, 5)
    units, device = shade_units(oracle, scene, (2,))
    camera = scene.camera(64, 36, accumulations=3, max_bounce_count=4)
    try:
        for kind, d in directions.items():
            for with_mis in (False, True):
                given, alternatives, tolerance, excluded = tc.expected_environment(scene.desc, tint, d, with_mis)
                for name, shade in units.items():
                    records = shade(camera, *tc.miss_entries(d, given))
                    assert (np.ascontiguousarray(records[:, 0]).view(np.uint32) == 0).all()      # a miss ends the path
                    # the share bound is for random inputs; the constructed directions sit on the map's texel edges on purpose (a nearest map leaves those out)
                    tc.held_to_reference(f"cpu environment {case} {kind} mis {int(with_mis)} {name}", records[:, 1:4], tc.nearest_alternative(records[:, 1:4], alternatives),
                                         tolerance, np.broadcast_to(excluded[:, None], tolerance.shape), allowed_share=0.01 if kind == "random" else None)
    finally:
        device.close()


# ---- the inputs themselves, the edited flags, and the two restatements against each other ----------------------------------------------------------------------
def test_the_textures_meet_every_combination_they_claim():
    """The 80 textures: every size under every wrap combination and every filter value; every (format, sRGB) under nearest and bilinear lookups, at every size and under
    every wrap combination; all texels of a texture distinct."""
    specs = tc.texture_specs()
    key = lambda s: ((s["width"], s["height"]), s["repeat"], int(s["linear"][0]) | 2 * int(s["linear"][1]))
    assert {key(s) for s in specs} == {(size, wrap, f) for size in tc.SIZES for wrap in tc.WRAPS for f in tc.FILTERS}
    kinds = {(f, srgb) for f in tc.FORMATS for srgb in (False, True)}
    for bilinear in (False, True):
        assert {(s["texel_format"], s["is_sRGB"]) for s in specs if s["linear"][0] == bilinear} == kinds
    for size in tc.SIZES:
        assert {(s["texel_format"], s["is_sRGB"]) for s in specs if (s["width"], s["height"]) == size} == kinds
    for wrap in tc.WRAPS:
        assert {(s["texel_format"], s["is_sRGB"]) for s in specs if s["repeat"] == wrap} == kinds
    for s in specs:
        texels = tc.pixels_of(s["width"], s["height"], s["texel_format"], s["salt"]).reshape(s["width"] * s["height"], -1)
        words = texels.view(np.float32) if s["texel_format"] in (capi.TEXEL_R32F, capi.TEXEL_RGBA32F) else texels
        assert all(len(np.unique(words[:, c])) == len(words) for c in range(words.shape[1])), s


def test_flags_after_a_material_edit_on_the_host_are_sound_too():
    """SceneBuilder::update_materials gives a quad's material another coverage texture -- the hole at another border --: the flags change, and the flagged triangles of
    that quad are covered wherever the reference looks in the NEW texture."""
    quads = tc.QuadScene(tc.rule_entries(), cells=tc.TESSELLATION)
    names = [q["spec"]["name"] for q in quads.quads]
    first, second = names.index("plain left_border wrap (True, True) bilinear True unit"), names.index("plain top_border wrap (True, True) bilinear True unit")
    before = quads.scene.triangles()
    edited = quads.scene.materials()[quads.quads[first]["material"]]
    edited.coverage_texture_ID = quads.quads[second]["texture"]
    assert quads.scene.update_materials([(quads.quads[first]["material"], edited)])
    pools = tc.Pools(quads.desc)
    assert (pools.triangles[:, 11] != before[:, 11]).sum() > 20
    triangles = np.where(pools.triangles[:, 9] == first)[0]
    flagged = (pools.flags_of(triangles) & capi.TRIANGLE_OPAQUE) != 0
    solid = (tc.lattice_coverage(pools, triangles, tc.barycentric_lattice()) == 1.0).all(axis=1)
    assert solid[flagged].all() and flagged.any() and (~solid).any() and (solid & ~flagged).any()


def test_host_build_and_oracle_agree_bit_for_bit_on_these_entries():
    """The device's shade_path compiled for the host against the oracle's hit programs (unorm16 tables, specified transcendentals) on the cut-out hits and the escaped rays
    of this module, word for word: the two restatements stay one, also at negative coordinates, at the poles and on the seam."""
    from bifrost3d_amd.host import Scene
    from device_host_bindings import DeviceShadeOnHost, oracle_shade
    from oracle_bindings import get_oracle
    exact = get_oracle(True)
    before = exact.lib.oracle_set_f64_transcendentals(1)
    try:
        quads = tc.QuadScene(tc.cutout_entries(tc.texture_specs()))
        sky = tc.constructed_environment(Scene("cornell"), (True, False))
        for scene, batches in ((quads, [tc.chosen_hits(quads, 40, 17)]),
                               (sky, [tc.miss_entries(d, tc.expected_environment(sky.desc, sky.tint, d, True)[0]) for d in tc.environment_directions(tc.ENVIRONMENT_PDF, 1500, 5).values()])):
            camera = scene.camera(64, 36, accumulations=3, max_bounce_count=4)
            device = DeviceShadeOnHost(scene)
            try:
                for entries in batches:
                    ours, theirs = device.shade(camera, *entries), oracle_shade(exact, scene, camera, *entries)
                    assert tc.same_bits(ours, theirs).all(), int((~tc.same_bits(ours, theirs).all(axis=1)).sum())
            finally:
                device.close()
    finally:
        exact.lib.oracle_set_f64_transcendentals(before)
