"""hipr_append_scene_pools on the GPU (csrc/pool_growth.h): the resident pools grown at their tails, then hipr_edit_scene_instances over them -- a model created over a
NEW mesh, material or texture, or drawn mirrored -- must leave, byte for byte, what the host path leaves: SceneBuilder::add_mesh / add_material / add_texture,
insert_model / remove_model, rebuild(), hipr_upload_scene on a fresh context. Every equality is of bytes; every refusal is an argument error that leaves the resident
scene as the call found it."""
import ctypes as C

import numpy as np
import pytest

import device_rebuild_bindings as rb
import instance_edit_bindings as ie
import pool_growth_bindings as pg
from bifrost3d_amd import capi
from bifrost3d_amd.renderer import Context
from test_gpu_device_rebuild import H, SPP, W, buffers, not_ready, render, same_trees, unequal
from test_gpu_instance_edit import adopt

pytestmark = pytest.mark.gpu

# the pools hipr_append_scene_pools grows, beside the eight buffers of test_gpu_device_rebuild.py
POOL_BUFFERS = (capi.SCENE_BUFFER_INDICES, capi.SCENE_BUFFER_GEOMETRY, capi.SCENE_BUFFER_TEXCOORDS, capi.SCENE_BUFFER_TINTS, capi.SCENE_BUFFER_EMISSIONS, capi.SCENE_BUFFER_TEXTURES,
                capi.SCENE_BUFFER_TEXELS)
POOL_NAMES = ("indices", "geometry", "texcoords", "tints", "emissions", "textures", "texels")


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fresh():
    """The context of the host path: it only ever takes uploads, each of which replaces everything an earlier one left."""
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle_q():
    from oracle_bindings import get_oracle
    return get_oracle(True)


def pool_buffers(context):
    return [context.read_scene_buffer(which) for which in POOL_BUFFERS]


def unequal_pools(a, b):
    return [name for name, x, y in zip(POOL_NAMES, a, b) if x.shape != y.shape or not np.array_equal(x, y)]


def all_unequal(mine, theirs):
    """Every readable buffer of two contexts, the old enumerators and the new ones."""
    return unequal(buffers(mine), buffers(theirs)) + unequal_pools(pool_buffers(mine), pool_buffers(theirs))


def pools_of_the_builder(scene):
    """A built host scene's pools in the order and the shapes of pool_buffers()."""
    p = pg.pools(scene)
    flat = lambda a: a.reshape(-1)
    return [flat(p["indices"]), p["geometry"], p["texcoords"], flat(p["tints"]), p["emissions"], p["textures"], p["texels"]]


def append_on_the_device(context, staged, operations, made=None, group=None):
    """The operations staged in the host scene and the tails appended to the resident pools. Returns (made, the edit list)."""
    made = pg.apply(staged, operations, made)
    growth_and_edits = staged.staged_scene_growth()
    assert growth_and_edits is not None
    growth, edits = growth_and_edits
    assert context.append_scene_pools(growth, group=group) == capi.HIPR_OK, context.lib.hipr_last_error()
    return made, edits


def grow_on_the_device(context, staged, operations, made=None):
    """Append, then edit. Returns (made, the edit's dict)."""
    made, edits = append_on_the_device(context, staged, operations, made)
    edited = context.edit_scene_instances(edits)
    assert edited["status"] == capi.HIPR_OK, context.lib.hipr_last_error()
    return made, edited


@pytest.mark.parametrize("name, arguments, rounds, attributes, opaque", pg.CASES, ids=pg.CASE_IDS)
def test_the_growths_leave_what_a_fresh_upload_of_the_hosts_rebuild_leaves(ctx, fresh, name, arguments, rounds, attributes, opaque):
    scene, host, made, host_made = rb.make_scene(arguments), rb.make_scene(arguments), {}, {}
    ctx.upload_scene(scene)
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    for operations in rounds:
        before = render(ctx, scene, spp=1)
        made, edited = grow_on_the_device(ctx, scene, operations, made)
        host_made = pg.apply(host, operations, host_made)
        host.rebuild()
        fresh.upload_scene(host)
        assert edited["instance_count"] == host.desc.instance_count and edited["triangle_count"] == host.desc.triangle_count
        assert all_unequal(ctx, fresh) == []
        same_trees(edited, host)
        assert edited["half_area"] == fresh.refit_scene_transforms([])["uploaded_half_area"] == ctx.refit_scene_transforms([])["uploaded_half_area"]
        # the host's description is brought along without a flatten of the whole scene
        adopt(scene, edited)
        assert rb.differences(rb.description(host), rb.description(scene)) == []
        after = render(ctx, scene, spp=1)
        print(f"{name}: {int((after != before).any(axis=-1).sum())} of {W * H} pixels differ from the image before the growth")
        assert after.tobytes() == render(fresh, host, spp=1).tobytes() and not np.array_equal(after, before)
    assert tuple(len(b) > 0 for b in pool_buffers(ctx)[2:5]) == attributes[1] and ie.switches(host)[0] == opaque[1]


@pytest.mark.parametrize("which", ["cornell_first_textured_quad", "cornell_new_box_and_its_mirror", "atrium_new_box_inserted_and_one_removed"])
def test_after_the_append_alone_the_scene_is_ready_and_only_the_pools_have_changed(ctx, which):
    name, arguments, rounds, attributes, opaque = pg.case(which)
    scene, host = rb.make_scene(arguments), pg.grown_on_the_host(arguments, rounds)
    ctx.upload_scene(scene)
    kept = buffers(ctx)
    still = render(ctx, scene)
    twin = rb.make_scene(arguments)      # the staging goes into a twin: `scene` keeps the description the device still draws
    append_on_the_device(ctx, twin, rounds[0])
    mine = buffers(ctx)
    # the material pool has grown where the case brings a material; trees, triangles, derived records and instances are untouched
    assert unequal(kept[:5] + kept[6:], mine[:5] + mine[6:]) == []
    assert np.array_equal(mine[5][:len(kept[5])], kept[5]) and np.array_equal(mine[5], pg.pools(host)["materials"])
    assert unequal_pools(pool_buffers(ctx), pools_of_the_builder(host)) == []
    image = render(ctx, scene)      # ready: no instance draws a tail yet
    print(f"{which}: after the append alone {int((image != still).any(axis=-1).sum())} of {W * H} pixels differ")
    assert np.isfinite(image).all()
    # the same image bit for bit where the append leaves the switches alone; the first texture of a scene picks the shade kernel's textured instantiation, whose
    # fast arithmetic need not round like the other's
    if which != "cornell_first_textured_quad":
        assert np.array_equal(image, still)


def test_the_mirror_kernel_alone(ctx):
    """Appends of nothing but one mirror segment: 1, 63, 64, 65 and 257 triples (a wave is 64 lanes, a block 256 threads), each over the pool the one before left."""
    scene = rb.make_scene(pg.ATRIUM)
    ctx.upload_scene(scene)
    pool = ctx.read_scene_buffer(capi.SCENE_BUFFER_INDICES)
    assert np.array_equal(pool, pg.pools(scene)["indices"].reshape(-1))
    others = buffers(ctx) + pool_buffers(ctx)[1:]
    triples = len(pool) // 3
    for count, source in ((257, 1234), (1, 0), (63, triples - 63), (64, 7000), (65, triples + 100)):      # the last one mirrors a range the first call of this loop appended
        growth, keep = pg.mirror_only_growth(source, count)
        assert ctx.append_scene_pools(growth) == capi.HIPR_OK, ctx.lib.hipr_last_error()
        grown = ctx.read_scene_buffer(capi.SCENE_BUFFER_INDICES)
        assert len(grown) == len(pool) + 3 * count and np.array_equal(grown[:len(pool)], pool)
        assert np.array_equal(grown[len(pool):], pg.mirrored(pool[3 * source:3 * (source + count)]))
        pool = grown
    # nothing else has moved
    assert unequal(others[:8], buffers(ctx)) == [] and unequal_pools(others[8:], pool_buffers(ctx)[1:]) == []


@pytest.mark.parametrize("arithmetic", ["fast", "exact"])
@pytest.mark.parametrize("which", ["cornell_first_textured_quad", "textured_new_quad_rgba8"])
def test_images_equal_the_fresh_uploads(arithmetic, which):
    """Both arithmetic modes, in the f64 mean; the first case flips the texture switches and all_triangles_opaque, so other kernel instantiations run, as after a fresh upload."""
    name, arguments, rounds, attributes, opaque = pg.case(which)
    context = Context(0, arithmetic=arithmetic)
    try:
        scene, host = rb.make_scene(arguments), pg.grown_on_the_host(arguments, rounds)
        context.upload_scene(scene)
        still = render(context, scene)
        made, edited = grow_on_the_device(context, scene, rounds[0])
        adopt(scene, edited)
        on_the_device = render(context, scene)
        context.upload_scene(host)
        on_the_host = render(context, host)
        print(f"{which}, {arithmetic}: {int((on_the_device != still).any(axis=-1).sum())} of {W * H} pixels differ from the image before the growth")
        assert not np.array_equal(on_the_device, still)
        assert np.array_equal(on_the_device.view(np.uint64), on_the_host.view(np.uint64))
    finally:
        context.close()


def test_traced_hits_and_counters_equal_the_oracles_on_the_hosts_grown_description(ctx, oracle_q):
    from test_coverage_cpu import cornell_box_rays
    name, arguments, rounds, attributes, opaque = pg.case("cornell_new_box")
    scene, host = rb.make_scene(arguments), pg.grown_on_the_host(arguments, rounds)
    ctx.upload_scene(scene)
    grow_on_the_device(ctx, scene, rounds[0])
    assert ctx.trace_variant() == capi.TRACE_WIDE8_PERSISTENT
    ctx.set_instrumentation(True)
    rays = cornell_box_rays(40000, 8)
    skip = np.full(len(rays), 0xFFFFFFFF, np.uint32)
    gpu = ctx.debug_trace_closest(rays, skip)
    counters = ctx.counters()
    cpu, (nodes, tris) = oracle_q.trace_closest(host.desc, rays, skip, use_bvh=ctx.oracle_search(), with_lights=True)
    assert np.array_equal(gpu.view(np.uint32), cpu.view(np.uint32))
    assert counters["closest_nodes"] == nodes and counters["closest_triangles"] == tris
    rays[:, 7] = np.random.default_rng(3).uniform(0.05, 2.0, len(rays))
    gpu_s = ctx.debug_trace_shadow(rays)
    counters = ctx.counters()
    ctx.set_instrumentation(False)
    cpu_s, (nodes, tris) = oracle_q.trace_shadow(host.desc, rays, use_bvh=ctx.oracle_search())
    assert np.array_equal(gpu_s, cpu_s) and counters["shadow_nodes"] == nodes and counters["shadow_triangles"] == tris


def test_life_after_a_growth(ctx, fresh):
    name, arguments, rounds, attributes, opaque = pg.case("atrium_new_box_inserted_and_one_removed")
    scene = rb.make_scene(arguments)
    ctx.upload_scene(scene)
    made, edited = grow_on_the_device(ctx, scene, rounds[0])
    adopt(scene, edited)
    # a device refit of the new model against the host path on the adopted scene
    nudged = dict(ie.NEAR, translation=(0.62, 0.41, -0.79))
    refitted = ctx.refit_scene_transforms(scene.model_pose(206, **nudged))
    assert not refitted["needs_rebuild"]
    assert scene.move_model(206, rebuild_threshold=1e30, **nudged) is True
    assert np.array_equal(ctx.read_scene_buffer(capi.SCENE_BUFFER_WIDE8_SLOTS), scene.wide8_slots()) and np.array_equal(ctx.read_scene_buffer(capi.SCENE_BUFFER_TRIANGLES), scene.triangles())
    # a material edit that gives another instance the NEW material slot, and rewrites that slot, against a fresh upload of the edited scene
    materials = scene.materials()
    new_slot = made["material coated"]
    materials[new_slot].coverage = 0.5
    changed, assignments = [(new_slot, materials[new_slot])], [(3, new_slot)]
    ctx.update_scene_materials(changed, assignments)
    assert scene.update_materials(changed, assignments) is True
    fresh.upload_scene(scene)
    mine, theirs = buffers(ctx), buffers(fresh)
    assert unequal(mine[:7], theirs[:7]) == []      # the BVH2 nodes are the ones the refit leaves stale
    assert unequal_pools(pool_buffers(ctx), pool_buffers(fresh)) == []
    assert render(ctx, scene, spp=1).tobytes() == render(fresh, scene, spp=1).tobytes()
    # a second growth after the first against the host path: the first tints of the scene, the pool whole
    second = [("mesh", "tinted_box"), ("remove", 206), ("insert", 0, "new tinted_box", new_slot, ie.NEAR, 212)]
    host, host_made = rb.make_scene(arguments), {}      # the host path on a twin: the same history, then rebuild()
    host_made = pg.apply(host, rounds[0], host_made)
    host.rebuild()
    assert host.move_model(206, rebuild_threshold=1e30, **nudged) is True
    assert host.update_materials(changed, assignments) is True
    host_made = pg.apply(host, second, host_made)
    host.rebuild()
    made, edited = grow_on_the_device(ctx, scene, second, made)
    assert made == host_made
    fresh.upload_scene(host)
    assert all_unequal(ctx, fresh) == []
    same_trees(edited, host)
    adopt(scene, edited)
    assert rb.differences(rb.description(host), rb.description(scene)) == []
    # a geometry update with the adopted description is accepted -- its pools have the grown sizes -- brings the new 4-wide tree and ends the stale state
    ctx.update_scene_geometry(scene)
    assert all_unequal(ctx, fresh) == []
    assert ctx.lib.hipr_set_trace_variant(ctx.handle, capi.TRACE_WIDE_PERSISTENT) == 0 and ctx.lib.hipr_set_trace_variant(ctx.handle, capi.TRACE_BVH2) == 0
    ctx.set_trace_variant(-1)
    assert render(ctx, scene, spp=1).tobytes() == render(fresh, host, spp=1).tobytes()


def test_an_append_after_a_refit_that_awaits_a_rebuild_leaves_that_state(ctx, tmp_path):
    import device_refit_bindings as refit
    scene = refit.scene_with_a_parting_pair(tmp_path / "pair.obj")
    ctx.upload_scene(scene)
    assert ctx.refit_scene_transforms(scene.model_pose(1, **refit.LARGE_POSE))["needs_rebuild"]
    assert not_ready(ctx, scene)
    words = len(ctx.read_scene_buffer(capi.SCENE_BUFFER_INDICES))
    growth, keep = pg.mirror_only_growth(0, 1)
    assert ctx.append_scene_pools(growth) == capi.HIPR_OK, ctx.lib.hipr_last_error()
    assert len(ctx.read_scene_buffer(capi.SCENE_BUFFER_INDICES)) == words + 3
    assert not_ready(ctx, scene)      # still awaiting the rebuild ...
    assert ctx.rebuild_scene_trees()["status"] == capi.HIPR_OK      # ... which the scene still takes
    assert not not_ready(ctx, scene)


def test_refusals_leave_the_buffers_and_a_render_as_before(ctx):
    INVALID = capi.HIPR_ERROR_INVALID_ARGUMENT
    lib = ctx.lib
    name, arguments, rounds, attributes, opaque = pg.case("cornell_first_textured_quad")
    scene, staged = rb.make_scene(arguments), rb.make_scene(arguments)
    pg.apply(staged, rounds[0])
    good, edits = staged.staged_scene_growth()
    # no scene: not ready, and still not ready afterwards
    empty = Context(0)
    try:
        assert lib.hipr_append_scene_pools(empty.handle, C.byref(good)) == capi.HIPR_ERROR_NOT_READY
        assert not_ready(empty, scene)
    finally:
        empty.close()
    ctx.upload_scene(scene)
    kept, kept_pools, before = buffers(ctx), pool_buffers(ctx), render(ctx, scene)
    d = scene.desc
    triples = d.index_count // 3

    def changed(**fields):
        g = capi.HiprPoolGrowth.from_buffer_copy(bytes(good))
        for field, value in fields.items():
            setattr(g, field, value)
        return g

    def segments(*pairs):
        return (capi.HiprIndexSegment * len(pairs))(*[capi.HiprIndexSegment(a, b) for a, b in pairs])

    def texture(**fields):
        t = (capi.HiprTexture * 1).from_buffer_copy(bytes(good.textures[0]))
        for field, value in fields.items():
            setattr(t[0], field, value)
        return t

    def material(**fields):
        m = (capi.HiprMaterial * 1).from_buffer_copy(bytes(good.materials[0]))
        for field, value in fields.items():
            setattr(m[0], field, value)
        return m

    HOST = capi.SEGMENT_FROM_HOST
    assert (good.vertex_count, good.texcoord_vertices, good.tint_vertices, good.index_count, good.material_count, good.texture_count, good.texel_bytes) == (4, d.vertex_count + 4, 4, 6, 1, 1, 16)
    refused = [
        ("a null description", None),
        # a null array with a non-zero count
        ("null geometry", changed(geometry=None)), ("null texcoords", changed(texcoords=None)), ("null tints", changed(tints=None)), ("null indices", changed(indices=None)),
        ("null segments", changed(segments=None)), ("null materials", changed(materials=None)), ("null textures", changed(textures=None)), ("null texels", changed(texels=None)),
        ("null emissions", changed(emissions=None, emission_vertices=d.vertex_count + 4)),
        # the index segments
        ("a host segment that is not whole triples", changed(segments=segments((HOST, 5)), index_count=5)),
        ("a mirror segment that is not whole triples", changed(segments=segments((HOST, 6), (0, 4)), segment_count=2)),
        ("host segments that take more than given", changed(segments=segments((HOST, 6), (HOST, 3)), segment_count=2)),
        ("host segments that take less than given", changed(segments=segments((HOST, 3)))),
        ("a mirror range past the pool as it stands", changed(segments=segments((triples - 1, 6), (HOST, 6)), segment_count=2)),
        ("a mirror range into its own place", changed(segments=segments((HOST, 6), (triples + 1, 6)), segment_count=2)),
        ("a mirror that starts past the pool", changed(segments=segments((HOST, 6), (triples + 2, 3)), segment_count=2)),
        # the attribute pools: tints are resident in the Cornell box, texcoords and emissions are not
        ("a resident attribute pool without its tail", changed(tints=None, tint_vertices=0)),
        ("a resident attribute pool given whole", changed(tint_vertices=d.vertex_count + 4)),
        ("an absent attribute pool given as a tail", changed(texcoord_vertices=4)),
        ("an absent attribute pool given short", changed(emissions=good.texcoords, emission_vertices=d.vertex_count)),
        # sums that do not fit their field
        ("vertices past 32 bits", changed(vertex_count=0xFFFFFFFF)),
        ("index words past 32 bits", changed(segments=segments((HOST, 0xFFFFFFFC)), index_count=0xFFFFFFFC)),
        ("materials past 32 bits", changed(material_count=0xFFFFFFFF)),
        ("textures past 32 bits", changed(texture_count=0xFFFFFFFF)),
        # a texture hipr_validate_scene would refuse against the grown texel pool
        ("a texture of an unknown format", changed(textures=texture(format=3))),
        ("a texture without extent", changed(textures=texture(width=0))),
        ("a texture larger than the grown texel pool", changed(textures=texture(height=5))),
        ("a texture that starts past the grown texel pool", changed(textures=texture(texel_offset=32))),
        ("a texture off its alignment", changed(textures=texture(texel_offset=2, height=2))),
        # a material it would refuse against the grown texture count
        ("a material with a texture past the grown pool", changed(materials=material(coverage_texture_ID=d.texture_count + 1))),
        ("a material with a negative texture", changed(materials=material(tint_roughness_texture_ID=-1))),
        ("a material of an unknown shading model", changed(materials=material(shading_model=9))),
    ]
    for what, growth in refused:
        status = lib.hipr_append_scene_pools(ctx.handle, C.byref(growth) if growth is not None else None)
        assert status == INVALID, (what, status, lib.hipr_last_error())
        assert unequal(kept, buffers(ctx)) == [] and unequal_pools(kept_pools, pool_buffers(ctx)) == [], what
        assert np.array_equal(render(ctx, scene), before), what
    # an empty description is taken and changes nothing
    assert lib.hipr_append_scene_pools(ctx.handle, C.byref(capi.HiprPoolGrowth())) == capi.HIPR_OK
    assert unequal(kept, buffers(ctx)) == [] and unequal_pools(kept_pools, pool_buffers(ctx)) == [] and np.array_equal(render(ctx, scene), before)
    # ... and the sound description is taken afterwards: nothing of the refusals stayed behind
    assert ctx.append_scene_pools(good) == capi.HIPR_OK, lib.hipr_last_error()
    edited = ctx.edit_scene_instances(edits)
    assert edited["status"] == capi.HIPR_OK, lib.hipr_last_error()
    host = pg.grown_on_the_host(arguments, rounds)
    same_trees(edited, host)
    assert unequal_pools(pool_buffers(ctx), pools_of_the_builder(host)) == []


def test_a_group_of_one_member_grows_like_a_single_context(ctx):
    lib = ctx.lib
    name, arguments, rounds, attributes, opaque = pg.case("atrium_new_box_inserted_and_one_removed")
    scene, staged = rb.make_scene(arguments), rb.make_scene(arguments)
    ctx.upload_scene(scene)
    made, single = grow_on_the_device(ctx, staged, rounds[0])
    adopt(staged, single)
    image = render(ctx, staged)
    devices = (C.c_int * 1)(0)
    group = C.c_void_p()
    assert lib.hipr_group_create(devices, 1, C.byref(group)) == 0
    try:
        tables = capi.load_tables()
        t = capi.HiprTables(*[a.ctypes.data_as(C.POINTER(C.c_float)) for a in tables])
        assert lib.hipr_group_upload_tables(group, C.byref(t)) == 0
        assert lib.hipr_group_upload_scene(group, C.byref(scene.desc)) == 0
        state = scene.state
        assert lib.hipr_group_set_scene_state(group, C.byref(state)) == 0
        assert lib.hipr_group_set_frame(group, W, H, 1) == 0
        again = rb.make_scene(arguments)
        # a description one member refuses leaves the group as it was ...
        bad, keep = pg.mirror_only_growth(scene.desc.index_count // 3, 1)
        assert lib.hipr_group_append_scene_pools(group, C.byref(bad)) == capi.HIPR_ERROR_INVALID_ARGUMENT
        # ... and the sound one is appended on every member
        made_again, edits = append_on_the_device(ctx, again, rounds[0], group=group)
        n = single["triangle_count"]
        edited = ctx.edit_scene_instances(edits, group=group, capacities=(n - 1, n, 2 * n))
        assert edited["status"] == capi.HIPR_OK, lib.hipr_last_error()
        assert all(np.array_equal(edited[k], single[k]) for k in ("nodes", "order", "slots")) and bytes(edited["raw"]) == bytes(single["raw"])
        for a in range(SPP):
            cam = staged.camera(W, H, accumulations=a, max_bounce_count=4)
            assert lib.hipr_group_trace_pass(group, C.byref(cam)) == 0
            assert lib.hipr_group_accumulate_samples(group, 0, 1, a, None, 0, 1) == 0
        accumulation = np.zeros((H, W, 4), np.float64)
        assert lib.hipr_group_read_accumulation(group, accumulation.ctypes.data_as(C.POINTER(C.c_double)), W * H) == 0
    finally:
        lib.hipr_group_destroy(group)
    assert np.array_equal(accumulation.view(np.uint64), image.view(np.uint64))


def test_a_model_over_a_new_mesh_through_the_renderer_class():
    """tests/native/PoolGrowthTest.cpp: with HIPR_DEVICE_POOL_GROWTH=1 HIPRenderer::Renderer appends a new mesh and a new material to the resident pools, edits the
    resident scene, counts the tick, uploads nothing further and gives the frame of the host path bit for bit; with the variable unset the counter stays 0."""
    import subprocess
    from pathlib import Path
    binary = Path(__file__).resolve().parent / "native" / "renderer_test"
    assert binary.exists(), f"{binary} is missing: run __graft_entry__.build()"
    p = subprocess.run([str(binary), "--gpu", "PoolGrowthFixture"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert "[       OK ] PoolGrowthFixture.a_model_over_a_new_mesh_grows_the_resident_pools" in p.stdout, p.stdout[-4000:]
    # a mesh destroyed in one growth tick and another created under its recycled ID in the next: drawn as itself, the full path's frame bit for bit
    assert "[       OK ] PoolGrowthFixture.a_new_mesh_under_a_recycled_mesh_id_is_drawn_as_itself" in p.stdout, p.stdout[-4000:]
