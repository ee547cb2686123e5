"""hipr_build_bvh2 on the GPU (csrc/bvh2_build.h): the BVH2 the kernels build is the host builder's, byte for byte -- nodes (64 B each), triangle order, depth --
a decline writes nothing, and a scene built through the device is the scene the host builds."""
import ctypes as C

import numpy as np
import pytest

import device_build_bindings as build
from bifrost3d_amd import capi
from bifrost3d_amd.host import Scene
from bifrost3d_amd.renderer import Context

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 36, 4
SETS = {
    **{f"n{n}": (lambda n=n: build.random_triangles(n, seed=n)) for n in (1, 2, 3, 4, 5, 7, 8)},
    "strip": lambda: build.strip(257),
    "zeros_negative_first": lambda: build.signed_zeros(True),
    "zeros_positive_first": lambda: build.signed_zeros(False),
    "cluster": build.with_cluster,
    "n257": lambda: build.random_triangles(257, 257),          # one past a block
    "n4097": lambda: build.random_triangles(4097, 4097),       # one past a block of blocks in the scans
    "n70000": lambda: build.random_triangles(70000, 7, size=0.01),        # long ranges span many blocks for bins and partition
    "n300000": lambda: build.random_triangles(300000, 21, size=0.004),    # the host's threaded path
}


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def device_build(ctx, triangles, max_depth=62):
    status, nodes, order, deepest = ctx.build_bvh2(triangles, max_depth)
    assert status == capi.HIPR_OK, ctx.lib.hipr_last_error()
    return dict(nodes=nodes, order=order, deepest=deepest)


@pytest.mark.parametrize("name", list(SETS))
def test_the_device_builds_the_hosts_tree_byte_for_byte(ctx, name):
    triangles = SETS[name]()
    build.same_tree(device_build(ctx, triangles), build.host_build(triangles))


def test_a_short_depth_budget(ctx):
    triangles = build.skewed(64)
    build.same_tree(device_build(ctx, triangles, 8), build.host_build(triangles, 8))


@pytest.mark.parametrize("triangles, max_depth", [(build.identical(300), 62), (build.random_triangles(4096, 11), 8)], ids=["identical", "budget_at_the_root"])
def test_a_decline_writes_nothing_and_the_context_builds_on(ctx, triangles, max_depth):
    nodes = np.full((len(triangles) - 1, 16), build.PATTERN, np.uint32)
    order = np.full(len(triangles), build.PATTERN, np.uint32)
    status, nodes, order, _ = ctx.build_bvh2(triangles, max_depth, nodes=nodes, order=order)
    assert status == capi.HIPR_ERROR_UNSUPPORTED
    assert f"[0, {len(triangles)})" in ctx.lib.hipr_last_error().decode()
    assert (nodes == build.PATTERN).all() and (order == build.PATTERN).all()
    status, handle = build.host_build_on_device(ctx, triangles, max_depth)      # the host entry hands the status out
    assert status == capi.HIPR_ERROR_UNSUPPORTED and handle is None
    following = build.random_triangles(1000, 3)
    build.same_tree(device_build(ctx, following), build.host_build(following))


def test_a_corner_that_is_not_finite_is_refused(ctx):
    for bad in (np.nan, np.inf):
        triangles = build.random_triangles(100, 1)
        triangles[57, 4] = np.array([bad], np.float32).view(np.uint32)[0]
        status, _, _, _ = ctx.build_bvh2(triangles)
        assert status == capi.HIPR_ERROR_INVALID_ARGUMENT and "triangle 57" in ctx.lib.hipr_last_error().decode()


def test_two_builds_of_one_input_are_byte_equal(ctx):
    triangles = SETS["n70000"]()
    first, second = device_build(ctx, triangles), device_build(ctx, triangles)
    build.same_tree(first, second)


def test_the_host_entry_collapses_the_devices_tree_like_its_own(ctx):
    triangles = build.random_triangles(5000, 17)
    status, ours = build.host_build_on_device(ctx, triangles)
    theirs = build.host_build(triangles)
    assert status == capi.HIPR_OK
    build.same_tree(ours, theirs)
    assert np.array_equal(ours["wide_nodes"], theirs["wide_nodes"])


def words(pointer, rows, columns):
    return np.ctypeslib.as_array(C.cast(pointer, C.POINTER(C.c_uint32)), shape=(rows, columns)).copy()


def test_a_scene_built_through_the_device_is_the_hosts_scene():
    ctx = Context(0, arithmetic="exact")
    try:
        plain = Scene("atrium", param0=20000)
        ours = Scene("atrium", param0=20000, device_builder=ctx)
        assert ours.build_counts()["device_builds"] == 1 and ours.build_counts()["declined_builds"] == 0
        a, b = ours.desc, plain.desc
        assert (a.node_count, a.wide_node_count, a.triangle_count, a.wide8_slot_count) == (b.node_count, b.wide_node_count, b.triangle_count, b.wide8_slot_count)
        assert np.array_equal(ours.nodes(), plain.nodes())
        assert np.array_equal(words(a.wide_nodes, a.wide_node_count, 16), words(b.wide_nodes, b.wide_node_count, 16))
        assert np.array_equal(ours.triangles(), plain.triangles())
        assert np.array_equal(ours.wide8_slots(), plain.wide8_slots())
        assert a.wide8_grid_min[:] == b.wide8_grid_min[:] and a.wide8_grid_cell[:] == b.wide8_grid_cell[:]
        assert (a.bvh_max_depth, a.wide_stack_entries, a.wide8_height) == (b.bvh_max_depth, b.wide_stack_entries, b.wide8_height)
        images = []
        for scene in (ours, plain):
            ctx.upload_scene(scene)
            ctx.set_frame(W, H)
            for k in range(SPP):
                ctx.render_pass(scene.camera(W, H, accumulations=k, max_bounce_count=4), synchronize=True)
            images.append(ctx.read_accumulation())
        assert np.array_equal(images[0], images[1])
    finally:
        ctx.close()


def test_a_build_leaves_the_resident_scene_untouched(ctx):
    scene = Scene("atrium", param0=20000)
    ctx.upload_scene(scene)
    buffers = [capi.SCENE_BUFFER_TRIANGLES, capi.SCENE_BUFFER_WIDE8_SLOTS, capi.SCENE_BUFFER_TRACE_TRIANGLES, capi.SCENE_BUFFER_SHADE_TRIANGLES, capi.SCENE_BUFFER_TRIANGLE_CLASS,
               capi.SCENE_BUFFER_MATERIALS, capi.SCENE_BUFFER_INSTANCES]
    before = [ctx.read_scene_buffer(which) for which in buffers]
    triangles = build.random_triangles(30000, 5, size=0.01)
    build.same_tree(device_build(ctx, triangles), build.host_build(triangles))
    for which, held in zip(buffers, before):
        assert np.array_equal(ctx.read_scene_buffer(which), held), which


def test_a_closed_context_is_no_longer_a_scenes_builder():
    ctx = Context(0)
    scene = Scene("cornell", param0=4, device_builder=ctx)
    assert scene.build_counts()["device_builds"] == 1
    before = scene.nodes()
    ctx.close()
    scene.rebuild()      # on the host: close() took the source out
    assert scene.build_counts() == dict(device_builds=1, declined_builds=0, longest_median_range=scene.build_counts()["longest_median_range"])
    assert np.array_equal(scene.nodes(), before)
    with pytest.raises(capi.HiprError):
        scene.use_device_builder(ctx)
