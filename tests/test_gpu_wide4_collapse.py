"""hipr_build_wide4 on the GPU (csrc/wide4_build.h): the compressed 4-wide tree the kernels collapse a BVH2 to is the host's, byte for byte -- nodes (64 B each), node
count, stack entries --, a refusal writes nothing and leaves the resident scene alone, a scene built through all three device stages is the scene the host builds, and
an instance edit adopted with the source installed asks the device for its 4-wide tree."""
import ctypes as C

import numpy as np
import pytest

import device_rebuild_bindings as rb
import instance_edit_bindings as ie
import wide4_collapse_bindings as w4
from bifrost3d_amd import capi
from bifrost3d_amd.host import Scene
from bifrost3d_amd.renderer import Context

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 36, 4
BUFFERS = capi.SCENE_BUFFERS + (capi.SCENE_BUFFER_NODES,)      # the eight readable buffers
NAMES = ("triangles", "slots", "trace triangles", "shade triangles", "classes", "materials", "instances", "nodes")


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def buffers(context):
    return [context.read_scene_buffer(which) for which in BUFFERS]


def unequal(a, b):
    return [name for name, x, y in zip(NAMES, a, b) if x.shape != y.shape or not np.array_equal(x, y)]


def render(context, scene, spp=SPP):
    context.set_frame(W, H)
    for a in range(spp):
        context.render_pass(scene.camera(W, H, accumulations=a, max_bounce_count=4), synchronize=True)
    return context.read_accumulation()


def device_collapse(context, nodes, triangle_count, group=None):
    status, wide, result = context.build_wide4(nodes, triangle_count, group=group)
    assert status == capi.HIPR_OK, context.lib.hipr_last_error()
    assert len(wide) == result["node_count"]
    return dict(wide_nodes=wide, stack_entries=result["stack_entries"])


# ---- the kernels against the host ----
@pytest.mark.parametrize("name", list(w4.SETS))
def test_the_device_collapses_the_hosts_bvh2_to_the_hosts_tree(ctx, name):
    host = w4.reference(name)
    w4.same_wide4(device_collapse(ctx, host["nodes"], len(host["triangles"])), host)


@pytest.mark.parametrize("name", list(w4.SETS))
def test_the_same_over_a_bvh2_the_device_built(ctx, name):
    host = w4.reference(name)
    status, nodes, order, _ = ctx.build_bvh2(host["triangles"])
    assert status == capi.HIPR_OK, ctx.lib.hipr_last_error()
    w4.same_wide4(device_collapse(ctx, nodes, len(host["triangles"])), host)


@pytest.mark.parametrize("name", list(w4.SYNTHETIC))
def test_the_device_collapses_the_synthetic_trees(ctx, name):
    nodes, triangles = w4.SYNTHETIC[name]()
    host = w4.host_collapse(nodes)
    if name == "budget_binds":
        assert host["did_not_fit"] >= 1 and host["budget"] == w4.SMALL_BUDGET
    if name == "comb":
        assert host["budget"] == w4.LARGE_BUDGET
    w4.same_wide4(device_collapse(ctx, nodes, triangles), host)


def test_the_exponent_seed_at_255_times_a_power_of_two(ctx):
    for name, nodes, triangles in w4.exponent_seed_trees():
        w4.same_wide4(device_collapse(ctx, nodes, triangles), w4.host_collapse(nodes))


def test_two_collapses_of_one_input_are_byte_equal(ctx):
    host = w4.reference("grid_70000")
    first, second = (device_collapse(ctx, host["nodes"], len(host["triangles"])) for _ in range(2))
    w4.same_wide4(first, second)
    w4.same_wide4(first, host)


def test_the_host_entry_returns_the_devices_tree(ctx):
    host = w4.reference("n4097")
    status, ours = w4.host_collapse_on_device(ctx, host["nodes"], len(host["triangles"]))
    assert status == capi.HIPR_OK
    w4.same_wide4(ours, host)
    times = ctx.collapse4_times()
    assert set(times) == {"validate", "upload", "kernels", "readback"} and times["kernels"] > 0.0


def test_a_group_of_one_member_collapses_to_the_same_bytes(ctx):
    host = w4.reference("n4097")
    devices = (C.c_int * 1)(0)
    group = C.c_void_p()
    assert ctx.lib.hipr_group_create(devices, 1, C.byref(group)) == 0
    try:
        w4.same_wide4(device_collapse(ctx, host["nodes"], len(host["triangles"]), group=group), host)
    finally:
        ctx.lib.hipr_group_destroy(group)


# ---- refusals ----
@pytest.fixture(scope="module")
def resident(ctx):
    """A resident scene with what it holds and a 1-spp image of it, for the refusals to leave alone."""
    scene = Scene("cornell", param0=4)
    ctx.upload_scene(scene)
    return scene, buffers(ctx), render(ctx, scene, spp=1)


REFUSALS = ["null_result", "no_nodes", "child_past_the_nodes", "leaf_past_the_triangles", "node_referenced_twice", "too_many_levels", "too_little_room", "child_box_not_finite"]


@pytest.mark.parametrize("what", REFUSALS)
def test_a_refusal_names_its_reason_and_writes_nothing(ctx, resident, what):
    scene, held, image = resident
    host = w4.reference("n17")
    nodes, triangles, reason = host["nodes"].copy(), 17, b""
    capacity = len(nodes)
    first_inner = next(i for i in range(len(nodes)) if np.int32(nodes[i, 12]) >= 0 or np.int32(nodes[i, 13]) >= 0)
    if what == "child_past_the_nodes":
        nodes[first_inner, 12 if np.int32(nodes[first_inner, 12]) >= 0 else 13] = len(nodes)
        reason = b"child"
    elif what == "leaf_past_the_triangles":
        where = next((i, c) for i in range(len(nodes)) for c in (12, 13) if np.int32(nodes[i, c]) < 0)
        nodes[where] = np.uint32(~np.uint32(((triangles - 1) << 3) | 2))
        reason = b"leaf"
    elif what == "node_referenced_twice":
        nodes[len(nodes) - 1, 12] = 0
        reason = b"twice"
    elif what == "too_many_levels":
        nodes, triangles = w4.comb(65)
        capacity, reason = len(nodes), b"level"
    elif what == "too_little_room":
        capacity, reason = len(host["wide_nodes"]) - 1, b"room"
    elif what == "child_box_not_finite":
        nodes[len(nodes) - 1, 1] = np.array([np.inf], np.float32).view(np.uint32)[0]
        reason = b"finite"
    elif what in ("null_result", "no_nodes"):
        reason = b"null argument or no nodes"
    wide = np.full((max(capacity, 1), 16), w4.PATTERN, np.uint32)
    result = np.full(2, w4.PATTERN, np.uint32)
    node_pointer = C.cast(nodes.ctypes.data, C.POINTER(capi.HiprBvhNode))
    if what == "null_result":
        status = ctx.lib.hipr_build_wide4(ctx.handle, node_pointer, len(nodes), triangles, wide.ctypes.data, capacity, None)
    elif what == "no_nodes":
        status = ctx.lib.hipr_build_wide4(ctx.handle, node_pointer, 0, triangles, wide.ctypes.data, capacity, C.cast(result.ctypes.data, C.POINTER(capi.HiprWide4BuildResult)))
    else:
        status, wide, result = ctx.build_wide4(nodes, triangles, wide=wide, result=result)
    message = ctx.lib.hipr_last_error()
    assert status == capi.HIPR_ERROR_INVALID_ARGUMENT, (status, message)
    assert b"hipr_build_wide4" in message and reason in message, message
    assert (wide == w4.PATTERN).all() and (result == w4.PATTERN).all()
    if what not in ("null_result", "no_nodes"):      # the host entry hands the status out
        status, handle = w4.host_collapse_on_device(ctx, nodes, triangles)
        assert (status, handle is None) == ((capi.HIPR_OK, False) if what == "too_little_room" else (capi.HIPR_ERROR_INVALID_ARGUMENT, True))
    assert unequal(buffers(ctx), held) == []
    assert np.array_equal(render(ctx, scene, spp=1), image)
    following = w4.reference("fan")      # ... and the context collapses on
    w4.same_wide4(device_collapse(ctx, following["nodes"], len(following["triangles"])), following)


# ---- scenes ----
def words(pointer, rows, columns):
    return np.ctypeslib.as_array(C.cast(pointer, C.POINTER(C.c_uint32)), shape=(rows, columns)).copy()


def rays_through(scene, n, seed):
    """Rays from inside the scene's bounds in random directions."""
    corners = scene.triangles()[:, :9].view(np.float32).reshape(-1, 3)
    lo, hi = corners.min(axis=0), corners.max(axis=0)
    rng = np.random.default_rng(seed)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = rng.uniform(lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo), (n, 3))
    d = rng.normal(size=(n, 3))
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 7] = np.inf
    return rays


@pytest.mark.parametrize("arguments", [ie.CORNELL, ie.ATRIUM], ids=["cornell", "atrium"])
def test_a_scene_built_through_the_three_device_stages_is_the_hosts_scene(monkeypatch, arguments):
    monkeypatch.setenv("HIPR_DEVICE_COLLAPSE", "1")      # whatever the defaults are
    monkeypatch.setenv("HIPR_DEVICE_COLLAPSE4", "1")
    context, other = Context(0, arithmetic="exact"), Context(0, arithmetic="exact")
    try:
        name, keywords = arguments
        plain = Scene(name, **keywords)
        ours = Scene(name, device_builder=context, **keywords)
        assert ours.build_counts()["device_builds"] == 1 and ours.collapse_counts() == dict(device_collapses=1, declined_collapses=0)
        assert ours.wide4_collapse_counts() == dict(device_collapses=1, declined_collapses=0)
        assert plain.wide4_collapse_counts() == dict(device_collapses=0, declined_collapses=0)
        assert rb.differences(rb.description(plain), rb.description(ours)) == []
        a = ours.desc
        assert a.node_count > 64 and a.wide_node_count > 1
        context.upload_scene(ours)
        other.upload_scene(plain)
        assert unequal(buffers(context), buffers(other)) == []
        # the 4-wide search over a fresh upload of each
        rays = rays_through(plain, 20000, 8)
        skip = np.full(len(rays), 0xFFFFFFFF, np.uint32)
        shadow_rays = rays.copy()
        shadow_rays[:, 7] = np.random.default_rng(3).uniform(0.05, 2.0, len(rays))
        seen = []
        for c, scene in ((context, ours), (other, plain)):
            c.set_trace_variant(capi.TRACE_WIDE_PERSISTENT)
            try:
                c.upload_scene(scene)
            finally:
                c.set_trace_variant(-1)
            assert c.trace_variant() == capi.TRACE_WIDE_PERSISTENT
            c.set_instrumentation(True)
            hits = c.debug_trace_closest(rays, skip)
            closest = c.counters()
            transmittance = c.debug_trace_shadow(shadow_rays)
            shadow = c.counters()
            c.set_instrumentation(False)
            seen.append((hits.view(np.uint32), transmittance.view(np.uint32), closest["closest_nodes"], closest["closest_triangles"], shadow["shadow_nodes"], shadow["shadow_triangles"],
                         render(c, scene).view(np.uint64)))
        device, host = seen
        assert (device[0][:, 3] != 0xFFFFFFFF).any() and device[2] > 0 and device[4] > 0      # rays that hit, counters that count
        assert np.array_equal(device[0], host[0]) and np.array_equal(device[1], host[1])
        assert device[2:6] == host[2:6]
        assert np.array_equal(device[6], host[6])
    finally:
        context.close()
        other.close()


def test_the_collapse_stays_on_the_host_when_asked(monkeypatch):
    monkeypatch.setenv("HIPR_DEVICE_COLLAPSE4", "0")
    context = Context(0)
    try:
        scene = Scene("cornell", param0=4, device_builder=context)
        assert scene.build_counts()["device_builds"] == 1 and scene.wide4_collapse_counts() == dict(device_collapses=0, declined_collapses=0)
        assert set(scene.collapse_counts()) == {"device_collapses", "declined_collapses"}
    finally:
        context.close()


def test_a_closed_context_no_longer_collapses_a_scene(monkeypatch):
    monkeypatch.setenv("HIPR_DEVICE_COLLAPSE4", "1")
    context = Context(0)
    scene = Scene("cornell", param0=4, device_builder=context)
    assert scene.wide4_collapse_counts() == dict(device_collapses=1, declined_collapses=0)
    before = rb.description(scene)
    context.close()
    scene.rebuild()      # on the host: close() took the sources out
    assert scene.wide4_collapse_counts() == dict(device_collapses=1, declined_collapses=0)
    assert rb.differences(before, rb.description(scene)) == []


def test_an_instance_edit_adopted_with_the_sources_installed_asks_the_device(monkeypatch):
    monkeypatch.setenv("HIPR_DEVICE_COLLAPSE", "1")
    monkeypatch.setenv("HIPR_DEVICE_COLLAPSE4", "1")
    name, arguments, prepare, operations, counts, switches = ie.EDITS[ie.EDIT_IDS.index("atrium_insert_middle")]
    context = Context(0)
    try:
        scene, host = ie.prepared(arguments, prepare), ie.edited_on_the_host(arguments, prepare, operations)
        assert scene.use_device_builder(context) is True      # the three sources, and a rebuild through them
        built = scene.wide4_collapse_counts()
        assert built == dict(device_collapses=1, declined_collapses=0)
        context.upload_scene(scene)
        ie.apply(scene, operations)
        edited = context.edit_scene_instances(scene.staged_instance_edits())
        assert edited["status"] == capi.HIPR_OK, context.lib.hipr_last_error()
        assert scene.adopt_edited_trees(edited["nodes"], edited["order"], edited["deepest"], edited["slots"], edited["raw"].wide8) is True
        assert rb.differences(rb.description(host), rb.description(scene)) == []
        assert scene.wide4_collapse_counts() == dict(device_collapses=2, declined_collapses=0)      # one device 4-wide collapse for the tick, no host one
        assert scene.rebuild_counts() == dict(adopted=1, refused=0)
    finally:
        context.close()
