"""Models created over NEW meshes, materials and textures on the host (SceneBuilder::add_mesh / add_material / add_texture after a build, staged_scene_growth), and the
mirror routine of hipr_append_scene_pools (csrc/pool_growth.h) walked on the host in the kernel's shape (tests/native/PoolGrowthHost.hip), against the same
operations followed by SceneBuilder::rebuild(). Every equality is of bytes."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import device_rebuild_bindings as rb
import instance_edit_bindings as ie
import material_update_bindings as mu
import pool_growth_bindings as pg
from bifrost3d_amd import capi

REPO = Path(__file__).resolve().parents[1]


def walked_round(scene, device, operations, made):
    """One growth on the host. `device` is a twin that holds what the device would: the scene before the round, rebuilt. The operations are staged in `scene`, the
    tails and segments applied on the CPU to copies of the twin's pools, the edit walked over the grown pools and the twin's triangles, the trees adopted.
    Returns (made, the grown pools, the edit's answer)."""
    old, resident, classes = pg.pools(device), device.triangles(), mu.derived_arrays(device)[2]
    made = pg.apply(scene, operations, made)
    staged = scene.staged_scene_growth()
    assert staged is not None
    growth, edits = staged
    grown = pg.applied_on_the_cpu(old, growth)
    pools, keep = pg.description_with(device, grown)
    answer = ie.routines_edit(resident, classes, pools, edits)
    assert answer["status"] == ie.EDITED, answer["status"]
    assert scene.adopt_edited_trees(answer["nodes"], answer["order"], int(answer["result"][2]), answer["slots"], ie.wide8_of(answer["result"])) is True
    return made, grown, answer


@pytest.mark.parametrize("name, arguments, rounds, attributes, opaque", pg.CASES, ids=pg.CASE_IDS)
def test_the_tails_and_segments_applied_on_the_cpu_and_the_walk_adopted_leave_what_rebuild_leaves(name, arguments, rounds, attributes, opaque):
    scene, host, made, host_made = rb.make_scene(arguments), rb.make_scene(arguments), {}, {}
    assert tuple(len(pg.pools(scene)[k]) > 0 for k in ("texcoords", "tints", "emissions")) == attributes[0] and ie.switches(scene)[0] == opaque[0]
    for operations in rounds:
        made, grown, answer = walked_round(scene, host, operations, made)
        host_made = pg.apply(host, operations, host_made)      # the yardstick: the same operations, then rebuild()
        host.rebuild()
        assert made == host_made
        # the pools the CPU made of the old ones and the tails are the rebuilt builder's, in every byte
        assert pg.unequal_pools(grown, pg.pools(host)) == []
        # ... and the adoption leaves the description rebuild() leaves
        assert rb.differences(rb.description(host), rb.description(scene)) == []
        assert (bool(answer["result"][14]), bool(answer["result"][15])) == ie.switches(host)
        # nothing is staged any more: the next growth starts from here
        growth, edits = scene.staged_scene_growth()
        assert bytes(growth) == bytes(capi.HiprPoolGrowth()) and all(e.source == k for k, e in enumerate(edits))
        assert scene.staged_instance_edits() is not None
    assert tuple(len(pg.pools(scene)[k]) > 0 for k in ("texcoords", "tints", "emissions")) == attributes[1] and ie.switches(scene)[0] == opaque[1]


def test_what_the_cases_stage():
    """The shape of the descriptions: a first mesh with an attribute brings the pool whole, a resident pool its tail; a mirrored copy is a mirror segment and nothing
    else; a mirror of a mesh of the same call reads a segment of that call."""
    def staged(name, round_index=0):
        _, arguments, rounds, _, _ = pg.case(name)
        scene, made = rb.make_scene(arguments), {}
        for operations in rounds[:round_index]:
            made = pg.apply(scene, operations, made)
            scene.rebuild()
        d = capi.HiprSceneDesc.from_buffer_copy(bytes(scene.desc))
        pg.apply(scene, rounds[round_index], made)
        growth, edits = scene.staged_scene_growth()
        return d, growth, edits, scene

    d, g, edits, _ = staged("cornell_new_box")
    assert (g.vertex_count, g.texcoord_vertices, g.tint_vertices, g.emission_vertices) == (8, 0, 8, 0) and pg.segments_of(g) == [(capi.SEGMENT_FROM_HOST, 36)] and g.index_count == 36
    assert (g.material_count, g.texture_count, g.texel_bytes) == (0, 0, 0) and [e.source for e in edits] == list(range(7)) + [capi.EDIT_NEW_INSTANCE] and edits[7].primitive_count == 12
    assert edits[7].instance.index_offset == d.index_count // 3 and edits[7].instance.vertex_offset == d.vertex_count
    d, g, edits, _ = staged("cornell_first_textured_quad")
    assert (g.vertex_count, g.texcoord_vertices, g.tint_vertices) == (4, d.vertex_count + 4, 4)      # the first texcoords: the pool whole
    assert (g.material_count, g.texture_count, g.texel_bytes) == (1, 1, 16) and g.textures[0].texel_offset == 0 and g.materials[0].coverage_texture_ID == d.texture_count
    d, g, edits, _ = staged("cornell_mirrored_copy")
    first = rb.make_scene(pg.CORNELL).instances_array()[5]      # model 6's instance: its mesh's triples
    assert pg.segments_of(g) == [(int(first[12]), 36)] and (g.vertex_count, g.index_count, g.material_count, g.texture_count, g.tint_vertices) == (0, 0, 0, 0, 0) and not g.indices
    assert edits[2].source == capi.EDIT_NEW_INSTANCE and edits[2].instance.index_offset == d.index_count // 3
    d, g, edits, _ = staged("cornell_new_box_and_its_mirror")
    assert pg.segments_of(g) == [(capi.SEGMENT_FROM_HOST, 36), (d.index_count // 3, 36)] and g.index_count == 36      # the mirror reads the segment before it
    d, g, edits, _ = staged("textured_new_quad_rgba8")
    assert (g.vertex_count, g.texcoord_vertices, g.tint_vertices, g.emission_vertices) == (4, 4, 0, 0)      # a resident pool: its tail
    assert (g.material_count, g.texture_count, g.texel_bytes) == (1, 1, 64) and g.textures[0].texel_offset == d.texel_bytes and g.textures[0].is_sRGB == 1
    d, g, edits, _ = staged("atrium_first_tints_then_emission", 1)
    assert (g.vertex_count, g.texcoord_vertices, g.tint_vertices, g.emission_vertices) == (8, 8, 8, d.vertex_count + 8)      # after the adoption of the first round the tints are resident
    # mesh triples on both sides of a mirror: the host's words are gathered, in order, and the segments keep the pool's order
    scene = rb.make_scene(pg.CORNELL)
    made = pg.apply(scene, [("mesh", "box"), ("insert", 0, "new box", 4, dict(pg.BESIDE_IT, scale=-0.25), 220), ("mesh", "quad")])
    growth, edits = scene.staged_scene_growth()
    base = rb.make_scene(pg.CORNELL).desc.index_count
    assert pg.segments_of(growth) == [(capi.SEGMENT_FROM_HOST, 36), (base // 3, 36), (capi.SEGMENT_FROM_HOST, 6)] and growth.index_count == 42
    assert np.array_equal(pg.words_at(growth.indices, 42).reshape(-1), np.concatenate([pg.BOX_PRIMITIVES.reshape(-1), pg.QUAD_PRIMITIVES.reshape(-1)]))
    twin = rb.make_scene(pg.CORNELL)
    grown = pg.applied_on_the_cpu(pg.pools(twin), growth)
    scene.rebuild()
    assert pg.unequal_pools(grown, pg.pools(scene)) == []


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_the_mirror_routine_in_the_kernels_shape(count):
    rng = np.random.default_rng(count)
    resident = rng.integers(0, 2 ** 32, 3 * (count + 5), dtype=np.uint64).astype(np.uint32)
    pool = np.full(len(resident) + 3 * count + 6, rb.PATTERN, np.uint32)
    pool[:len(resident)] = resident
    source, target = 3, len(resident) // 3
    assert pg.mirror_host_triples(pool, source, target, count) == count      # the threads past the count write nothing
    assert np.array_equal(pool[:len(resident)], resident)
    assert np.array_equal(pool[3 * target:3 * (target + count)], pg.mirrored(resident[3 * source:3 * (source + count)]))
    assert (pool[3 * (target + count):] == rb.PATTERN).all()
    # through the segment walk, and a range that reaches into the segment's own place is refused
    growth, keep = pg.mirror_only_growth(source, count)
    again = np.full(len(pool), rb.PATTERN, np.uint32)
    again[:len(resident)] = resident
    assert pg.grow_host_indices(again[:len(resident) + 3 * count], len(resident), growth) == len(resident) + 3 * count and np.array_equal(again, pool)
    growth, keep = pg.mirror_only_growth(target - count + 1, count)
    assert pg.grow_host_indices(again[:len(resident) + 3 * count], len(resident), growth) == -1 and np.array_equal(again, pool)


def test_after_a_growth_the_instance_edits_alone_still_refuse_and_a_staged_move_refuses_both():
    scene = rb.make_scene(pg.CORNELL)
    assert scene.staged_scene_growth() is not None and scene.staged_instance_edits() is not None
    made = pg.apply(scene, [("mesh", "box")])
    assert scene.staged_instance_edits() is None and scene.staged_scene_growth() is not None      # a pool has grown: only the growth carries it
    pg.apply(scene, [("insert", 1000, "new box", 4, pg.IN_THE_BOX, 230)], made)
    assert scene.staged_instance_edits() is None
    growth, edits = scene.staged_scene_growth()
    assert growth.vertex_count == 8 and len(edits) == 8
    assert scene.stage_model(6, **rb.POSE) is True      # a move staged as well: the full path
    assert scene.staged_scene_growth() is None and scene.staged_instance_edits() is None
    scene.rebuild()
    growth, edits = scene.staged_scene_growth()
    assert bytes(growth) == bytes(capi.HiprPoolGrowth()) and len(edits) == 8 and scene.staged_instance_edits() is not None
    # a material or a texture alone grows a pool as well
    scene.add_material(pg.material())
    assert scene.staged_instance_edits() is None and scene.staged_scene_growth()[0].material_count == 1
    # a scene that is not built stages nothing
    from bifrost3d_amd.host import Scene
    assert Scene("cornell", param0=4).staged_scene_growth() is not None      # built by its constructor


def test_the_staging_and_the_mirror_routine_under_the_sanitizers():
    """`make sanitize-pool-growth`: the stand-alone program (tests/native/PoolGrowthSanitize.cpp) stages growths in a scene builder compiled into it and walks their
    segments through the mirror routine under ASan + UBSan on the CPU."""
    done = subprocess.run(["make", "-C", str(REPO / "bifrost3d_amd"), "sanitize-pool-growth"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "4 growths staged and walked" in done.stdout and "a mirror range past the pool: refused" in done.stdout
