"""hipr_build_wide8 on the GPU (csrc/wide8_build.h): the 8-wide tree the kernels collapse a BVH2 to is the host's, byte for byte -- slots (64 B each), height, grid,
counters --, a refusal writes nothing, and a scene built through the device is the scene the host builds."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import device_collapse_bindings as collapse
from bifrost3d_amd import capi
from bifrost3d_amd.host import Scene
from bifrost3d_amd.renderer import Context

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 36, 4
REPO = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def device_collapse(ctx, nodes, triangles, order):
    status, slots, result = ctx.build_wide8(nodes, triangles, order)
    assert status == capi.HIPR_OK, ctx.lib.hipr_last_error()
    grid = np.concatenate([result["grid_min"], result["grid_cell"]]).astype(np.float32).view(np.uint32)
    return dict(slots=slots, height=result["height"], grid=grid, counts=(result["node_count"], result["leaf_count"], result["paired_leaves"]))


@pytest.mark.parametrize("name", list(collapse.SETS))
def test_the_device_collapses_the_hosts_bvh2_to_the_hosts_tree(ctx, name):
    host = collapse.reference(name)
    collapse.same_wide8(device_collapse(ctx, host["nodes"], host["triangles"], host["order"]), host["wide8"])


@pytest.mark.parametrize("name", list(collapse.SETS))
def test_the_same_over_a_bvh2_the_device_built(ctx, name):
    host = collapse.reference(name)
    status, nodes, order, _ = ctx.build_bvh2(host["triangles"])
    assert status == capi.HIPR_OK, ctx.lib.hipr_last_error()
    collapse.same_wide8(device_collapse(ctx, nodes, host["triangles"], order), host["wide8"])


def test_the_triangles_in_leaf_order_without_an_order_array(ctx):
    host = collapse.reference("grid16")
    collapse.same_wide8(device_collapse(ctx, host["nodes"], host["triangles"][host["order"]], None), host["wide8"])


def test_two_collapses_of_one_input_are_byte_equal(ctx):
    host = collapse.reference("grid_70000")
    first, second = (device_collapse(ctx, host["nodes"], host["triangles"], host["order"]) for _ in range(2))
    collapse.same_wide8(first, second)


@pytest.mark.parametrize("what", ["slot_capacity", "child_index"])
def test_a_refusal_writes_nothing_and_the_context_collapses_on(ctx, what):
    host = collapse.reference("grid16")
    nodes, needed = host["nodes"].copy(), len(host["wide8"]["slots"])
    if what == "child_index":
        inner = next(i for i in range(len(nodes)) if np.int32(nodes[i, 12]) >= 0)
        nodes[inner, 12] = len(nodes)
    slots = np.full((needed - 1 if what == "slot_capacity" else 2 * needed, 16), collapse.PATTERN, np.uint32)
    result = np.full(12, collapse.PATTERN, np.uint32)
    status, slots, result = ctx.build_wide8(nodes, host["triangles"], host["order"], slots=slots, result=result)
    assert status == capi.HIPR_ERROR_INVALID_ARGUMENT, ctx.lib.hipr_last_error()
    assert (slots == collapse.PATTERN).all() and (result == collapse.PATTERN).all()
    status, handle = collapse.host_collapse_on_device(ctx, nodes, host["triangles"], host["order"])      # the host entry hands the status out
    assert (status, handle is None) == ((capi.HIPR_OK, False) if what == "slot_capacity" else (capi.HIPR_ERROR_INVALID_ARGUMENT, True))
    following = collapse.reference("fan")
    collapse.same_wide8(device_collapse(ctx, following["nodes"], following["triangles"], following["order"]), following["wide8"])


def test_a_corner_that_is_not_finite_is_refused(ctx):
    host = collapse.reference("n17")
    triangles = host["triangles"].copy()
    triangles[5, 4] = np.array([np.inf], np.float32).view(np.uint32)[0]
    slots, result = np.full((40, 16), collapse.PATTERN, np.uint32), np.full(12, collapse.PATTERN, np.uint32)
    status, slots, result = ctx.build_wide8(host["nodes"], triangles, host["order"], slots=slots, result=result)
    assert status == capi.HIPR_ERROR_INVALID_ARGUMENT and "finite" in ctx.lib.hipr_last_error().decode()
    assert (slots == collapse.PATTERN).all() and (result == collapse.PATTERN).all()


def test_the_host_entry_returns_the_devices_tree(ctx):
    host = collapse.reference("n4097")
    status, ours = collapse.host_collapse_on_device(ctx, host["nodes"], host["triangles"], host["order"])
    assert status == capi.HIPR_OK
    collapse.same_wide8(ours, host["wide8"])
    times = ctx.collapse_times()
    assert set(times) == {"validate", "upload", "kernels", "readback"} and times["kernels"] > 0.0


def test_a_collapse_leaves_the_resident_scene_untouched(ctx):
    scene = Scene("atrium", param0=20000)
    ctx.upload_scene(scene)
    buffers = [capi.SCENE_BUFFER_TRIANGLES, capi.SCENE_BUFFER_WIDE8_SLOTS, capi.SCENE_BUFFER_TRACE_TRIANGLES, capi.SCENE_BUFFER_SHADE_TRIANGLES, capi.SCENE_BUFFER_TRIANGLE_CLASS,
               capi.SCENE_BUFFER_MATERIALS, capi.SCENE_BUFFER_INSTANCES]
    before = [ctx.read_scene_buffer(which) for which in buffers]
    host = collapse.reference("n4097")
    collapse.same_wide8(device_collapse(ctx, host["nodes"], host["triangles"], host["order"]), host["wide8"])
    for which, held in zip(buffers, before):
        assert np.array_equal(ctx.read_scene_buffer(which), held), which


def words(pointer, rows, columns):
    return np.ctypeslib.as_array(C.cast(pointer, C.POINTER(C.c_uint32)), shape=(rows, columns)).copy()


def test_a_scene_collapsed_on_the_device_is_the_hosts_scene(monkeypatch):
    monkeypatch.setenv("HIPR_DEVICE_COLLAPSE", "1")      # whatever the default is
    ctx = Context(0, arithmetic="exact")
    try:
        plain = Scene("atrium", param0=20000)
        ours = Scene("atrium", param0=20000, device_builder=ctx)
        assert ours.collapse_counts() == dict(device_collapses=1, declined_collapses=0)
        assert plain.collapse_counts() == dict(device_collapses=0, declined_collapses=0)
        assert set(ours.build_counts()) == {"device_builds", "declined_builds", "longest_median_range"} and ours.build_counts()["device_builds"] == 1
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


def test_the_collapse_stays_on_the_host_when_asked(monkeypatch):
    monkeypatch.setenv("HIPR_DEVICE_COLLAPSE", "0")
    ctx = Context(0)
    try:
        scene = Scene("cornell", param0=4, device_builder=ctx)
        assert scene.build_counts()["device_builds"] == 1 and scene.collapse_counts() == dict(device_collapses=0, declined_collapses=0)
    finally:
        ctx.close()


def test_a_closed_context_no_longer_collapses_a_scene(monkeypatch):
    monkeypatch.setenv("HIPR_DEVICE_COLLAPSE", "1")
    ctx = Context(0)
    scene = Scene("cornell", param0=4, device_builder=ctx)
    assert scene.collapse_counts() == dict(device_collapses=1, declined_collapses=0)
    before = scene.wide8_slots()
    ctx.close()
    scene.rebuild()      # on the host: close() took both sources out
    assert scene.collapse_counts() == dict(device_collapses=1, declined_collapses=0)
    assert np.array_equal(scene.wide8_slots(), before)


def test_the_renderer_class_collapses_on_the_device():
    """The native cases of tests/native/DeviceCollapseTest.cpp: the Renderer under HIPR_DEVICE_BUILD=1 renders the frame it renders without, and with HIPR_DEVICE_COLLAPSE=0 it
    counts no device collapse."""
    env = {k: v for k, v in os.environ.items() if k not in ("HIPR_DEVICE_BUILD", "HIPR_DEVICE_COLLAPSE")}
    binary = REPO / "tests" / "native" / "renderer_test"
    assert binary.exists(), f"{binary} is missing: run __graft_entry__.build()"
    done = subprocess.run([str(binary), "--gpu", "DeviceCollapseFixture"], env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-4000:] + done.stderr[-4000:]
    for case in ("the_frame_is_the_same_with_the_trees_built_on_the_device", "the_collapse_stays_on_the_host_when_the_variable_says_so"):
        assert f"[       OK ] DeviceCollapseFixture.{case}" in done.stdout, done.stdout[-4000:]
