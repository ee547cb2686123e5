#!/usr/bin/env python3
"""A model created over a NEW mesh and another destroyed, four ways: the resident pools grown and the resident scene edited on the device (SceneBuilder::add_mesh /
insert_model / remove_model staged, hipr_append_scene_pools, hipr_edit_scene_instances, SceneBuilder::adopt_edited_trees; csrc/pool_growth.h) against the paths the
same tick takes without it -- add_mesh / insert_model / remove_model, rebuild() + hipr_upload_scene, and the same with both build stages on the device (what
HIPR_DEVICE_BUILD=1 gives HIPRenderer::Renderer) -- and, in the same run, against the same edit over a mesh the device already holds (tools/instance_edit_probe.py's
device path). The difference to that last line is what the growth costs; the library splits the append into allocation, device copies and host-to-device tails
(hipr_debug_append_times).

The new mesh of every repeat is the data of a resident model's mesh -- its positions, texcoords and triples read from the description -- added as a new mesh; its
normals are NOT the source's (the description holds them octahedrally encoded) but one constant vector per vertex, which costs what any normal costs: sixteen bytes per
vertex record either way, and no timing depends on their values. The pools grow by one such mesh per repeat, as a scene does whose meshes come and go (destroyed meshes stay pooled).

Wall time around the calls with the stream synchronised inside, the median of `--repeats` repeats after `--warmup` untimed ones.

    python tools/pool_growth_probe.py --scenes atrium251k atrium10M --out profiles/pool_growth_device_vs_host.txt
"""
import argparse
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

from bifrost3d_amd import capi      # noqa: E402
from bifrost3d_amd.host import Scene      # noqa: E402
from bifrost3d_amd.renderer import Context      # noqa: E402
from device_build_probe import SCENES, captured_stderr      # noqa: E402
import instance_edit_probe as resident_mesh      # noqa: E402

POSES = resident_mesh.POSES
FIRST_COPY = 2000      # the model indices of the created models: FIRST_COPY + the repeat that created them


def mesh_of(scene, source) -> dict:
    """The data of the mesh of the model at `source["position"]` of the instance list, from the description: what add_mesh takes to make a new mesh of it."""
    d = scene.desc
    instance = scene.instances_array()[source["position"]]
    index_offset, vertex_offset = int(instance[12]), int(instance[13])
    primitives = int((scene.triangles()[:, 9] == source["position"]).sum())
    triples = np.ctypeslib.as_array(d.indices, shape=(d.index_count,))[3 * index_offset:3 * (index_offset + primitives)].reshape(-1, 3).copy()
    vertices = int(triples.max()) + 1
    geometry = np.ctypeslib.as_array(C_cast_words(d.geometry), shape=(d.vertex_count, 4))[vertex_offset:vertex_offset + vertices]
    mesh = dict(positions=geometry[:, :3].copy().view(np.float32), primitives=triples, normals=np.tile(np.array([0.0, 1.0, 0.0], np.float32), (vertices, 1)))
    if d.texcoords:
        mesh["texcoords"] = np.ctypeslib.as_array(d.texcoords, shape=(2 * d.vertex_count,))[2 * vertex_offset:2 * (vertex_offset + vertices)].reshape(-1, 2).copy()
    return mesh


def C_cast_words(pointer):
    import ctypes as C
    return C.cast(pointer, C.POINTER(C.c_uint32))


def stage(scene, source, mesh, k):
    """The tick of repeat k: the model of repeat k - 1 goes, a new mesh comes and a model over it at the other pose, in the middle of the instance list."""
    if k > 0:
        assert scene.remove_model(FIRST_COPY + k - 1)
    scene.insert_model(source["position"] + 1, scene.add_mesh(**mesh), source["material"], model_index=FIRST_COPY + k, **POSES[k % 2])


def device_path(scene, ctx, source, mesh, first, warmup, repeats):
    rows = []
    for k in range(first, first + warmup + repeats):
        with captured_stderr():
            t0 = time.perf_counter()
            stage(scene, source, mesh, k)
            growth, edits = scene.staged_scene_growth()
            t1 = time.perf_counter()
            status = ctx.append_scene_pools(growth)
            ctx.synchronize()
            t2 = time.perf_counter()
            assert status == capi.HIPR_OK, ctx.lib.hipr_last_error()
            edited = ctx.edit_scene_instances(edits)
            ctx.synchronize()
            t3 = time.perf_counter()
            assert edited["status"] == capi.HIPR_OK, ctx.lib.hipr_last_error()
            adopted = scene.adopt_edited_trees(edited["nodes"], edited["order"], edited["deepest"], edited["slots"], edited["raw"].wide8)
            t4 = time.perf_counter()
        assert adopted, "the scene builder refused the device's trees"
        if k >= first + warmup:
            rows.append(dict(total=(t4 - t0) * 1e3, staging=(t1 - t0) * 1e3, append=(t2 - t1) * 1e3, edit=(t3 - t2) * 1e3, adoption=(t4 - t3) * 1e3, tail_bytes=growth_bytes(growth), **ctx.append_times()))
    d = scene.desc
    same = all(np.array_equal(ctx.read_scene_buffer(which).reshape(-1), expected.reshape(-1)) for which, expected in
               ((capi.SCENE_BUFFER_TRIANGLES, scene.triangles()), (capi.SCENE_BUFFER_WIDE8_SLOTS, scene.wide8_slots()), (capi.SCENE_BUFFER_INSTANCES, scene.instances_array()),
                (capi.SCENE_BUFFER_INDICES, np.ctypeslib.as_array(d.indices, shape=(d.index_count,))), (capi.SCENE_BUFFER_GEOMETRY, np.ctypeslib.as_array(C_cast_words(d.geometry), shape=(d.vertex_count, 4)))))
    med = statistics.median
    out = {key: med(r[key] for r in rows) for key in rows[0]}
    out.update(low=min(r["total"] for r in rows), high=max(r["total"] for r in rows), same=same, triangles=edited["triangle_count"], pool_bytes=pool_bytes(d))
    return out


def growth_bytes(g) -> int:
    words = sum(g.segments[k].index_count for k in range(g.segment_count))
    return 16 * g.vertex_count + 8 * g.texcoord_vertices + 4 * g.tint_vertices + 12 * g.emission_vertices + 4 * words + 64 * g.material_count + 24 * g.texture_count + g.texel_bytes


def pool_bytes(d) -> int:
    return 4 * d.index_count + d.vertex_count * (16 + (8 if d.texcoords else 0) + (4 if d.tints else 0) + (12 if d.emissions else 0)) + 64 * d.material_count + 24 * d.texture_count + d.texel_bytes


def host_path(scene, ctx, source, mesh, first, warmup, repeats):
    """What the renderer class does for the same tick without the device path, given a scene builder that keeps its pools: the tick, SceneBuilder::rebuild(), hipr_upload_scene."""
    walls = []
    for k in range(first, first + warmup + repeats):
        with captured_stderr():
            t0 = time.perf_counter()
            stage(scene, source, mesh, k)
            scene.rebuild()
            t1 = time.perf_counter()
            ctx.upload_scene(scene)
            ctx.synchronize()
            t2 = time.perf_counter()
        if k >= first + warmup:
            walls.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
    med = statistics.median
    return dict(total=med(w[0] for w in walls), rebuild=med(w[1] for w in walls), upload=med(w[2] for w in walls), low=min(w[0] for w in walls), high=max(w[0] for w in walls))


def measure(triangles, seed, model, warmup, repeats):
    os.environ.pop("HIPR_DEVICE_COLLAPSE", None)
    ctx = Context(0)
    scene = Scene("atrium", param0=triangles, param1=seed)
    source = scene.model_info(model)
    mesh = mesh_of(scene, source)
    per = warmup + repeats
    ctx.upload_scene(scene)
    resident = resident_mesh.device_path(scene, ctx, source, 0, warmup, repeats)      # the same edit over the mesh the device holds
    assert scene.remove_model(resident_mesh.FIRST_COPY + per - 1)
    scene.rebuild()
    ctx.upload_scene(scene)
    device = device_path(scene, ctx, source, mesh, 0, warmup, repeats)
    host = host_path(scene, ctx, source, mesh, per, warmup, repeats)
    scene.use_device_builder(ctx)
    both = host_path(scene, ctx, source, mesh, 2 * per, warmup, repeats)
    counts = dict(scene.build_counts(), **scene.collapse_counts())
    scene.use_device_builder(None)
    ctx.close()
    return dict(device=device, host=host, both=both, resident=resident, counts=counts, mesh=(len(mesh["positions"]), len(mesh["primitives"])))


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scenes", nargs="+", default=list(SCENES), choices=list(SCENES))
    p.add_argument("--model", type=int, default=10, help="the model whose mesh data becomes the new mesh (1-based, in creation order)")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=10)
    p.add_argument("--out", default=str(ROOT / "profiles" / "pool_growth_device_vs_host.txt"))
    args = p.parse_args()
    lines = ["Output of tools/pool_growth_probe.py; anything after the line 'Reading' at the end is commentary written by hand.", "",
             f"Per repeat a new mesh (the data of model {args.model}'s mesh of the procedural atrium) with a model over it created and the model of the repeat before destroyed: the resident pools grown",
             "and the resident scene edited on the device against the host's rebuild + upload, and against the same edit over the mesh the device already holds.",
             f"Wall time around the calls, stream synchronised inside; median of {args.repeats} repeats after {args.warmup} warm-up repeats, [min .. max].",
             "The split of the append is the library's own (hipr_debug_append_times).", ""]
    for name in args.scenes:
        r = measure(*SCENES[name], args.model, args.warmup, args.repeats)
        d, h, b, m = r["device"], r["host"], r["both"], r["resident"]
        lines += [f"{name}: {d['triangles']} triangles; the new mesh has {r['mesh'][0]} vertices and {r['mesh'][1]} triangles, a tail of {d['tail_bytes'] / 1e6:.3f} MB behind pools of {d['pool_bytes'] / 1e6:.1f} MB at the end;"
                  f" the resident triangles, instances, slots, indices and vertices {'equal' if d['same'] else 'DIFFER FROM'} the adopted description's",
                  f"  device growth + edit               {d['total']:10.3f} ms  [{d['low']:.3f} .. {d['high']:.3f}]  = staging {d['staging']:.3f} + hipr_append_scene_pools {d['append']:.3f}"
                  f" + hipr_edit_scene_instances {d['edit']:.3f} + adoption {d['adoption']:.3f} ms",
                  f"      hipr_append_scene_pools        = allocation {d['allocation']:.3f} + device-to-device copies of the resident parts {d['resident_copies']:.3f} + host-to-device tails {d['tails']:.3f} ms"
                  f" (the rest: the checks, freeing the old buffers)",
                  f"  the same edit, resident mesh       {m['total']:10.3f} ms  [{m['low']:.3f} .. {m['high']:.3f}]  = staging {m['staging']:.3f} + hipr_edit_scene_instances {m['edit']:.3f} + adoption {m['adoption']:.3f} ms",
                  f"  host: tick + rebuild() + upload    {h['total']:10.3f} ms  [{h['low']:.3f} .. {h['high']:.3f}]  = rebuild {h['rebuild']:.3f} + upload {h['upload']:.3f} ms",
                  f"  the same, both stages on device    {b['total']:10.3f} ms  [{b['low']:.3f} .. {b['high']:.3f}]  = rebuild {b['rebuild']:.3f} + upload {b['upload']:.3f} ms"
                  f"  (BVH2 builds through the device {r['counts']['device_builds']}, declined {r['counts']['declined_builds']}; collapses {r['counts']['device_collapses']}, declined {r['counts']['declined_collapses']})",
                  f"  growth costs {d['total'] - m['total']:.3f} ms over the resident mesh's edit; host / device = {h['total'] / d['total']:.2f}, both stages on device / device = {b['total'] / d['total']:.2f}", ""]
        print("\n".join(lines[-8:]), flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")      # after every scene: a run cut short keeps what it has


if __name__ == "__main__":
    main()
