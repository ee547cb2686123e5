#!/usr/bin/env python3
"""Vertices of a resident mesh edited, three ways: the path every vertex edit used to take -- a new scene: SceneBuilder::rebuild (the triangles flattened again, the
BVH2, the 4-wide and the 8-wide tree built) + hipr_upload_scene of every pool; the host refit where it suffices -- SceneBuilder::update_vertices +
hipr_update_scene_geometry; and the device path -- SceneBuilder::stage_vertex_edits + hipr_update_scene_vertices (csrc/vertex_update.h), after which the builder
catches up with apply_staged_transforms whenever its description is next wanted (timed apart).

Two edits of the textured procedural atrium: the mesh of one model deformed (all its positions, smoothly, so that coincident vertices stay coincident; the normals
travel with them) and the texture coordinates of a lace banner scrolled. All legs are timed around the calls, with a stream synchronise inside the timed span, as the
median of `--repeats` repeats after `--warmup` untimed ones. The result of the three paths is the same bytes (tests/test_gpu_vertex_update.py). The device call's
own figures (hipr_debug_vertex_update_times) are printed with it.

    python tools/vertex_update_probe.py --scenes atrium251k atrium10M --out profiles/vertex_update_device_vs_host.txt
"""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from bifrost3d_amd import capi      # noqa: E402
from bifrost3d_amd.host import Scene      # noqa: E402
from bifrost3d_amd.renderer import Context      # noqa: E402

SCENES = {"atrium251k": (260000, 1), "atrium10M": (10000000, 2)}      # name: (param0 = target triangle count, param1 = seed) of the procedural atrium
EDITS = ("mesh_deformed", "lace_texcoords_scrolled")
NEVER_REBUILD = 1e30


def plan(scene):
    """The model with the most triangles that is not a lace banner, and a lace banner: (mesh, instance, triangles) each, or None."""
    triangles, instances, materials = scene.triangles(), scene.instances_array(), scene.materials()
    counts = np.bincount(triangles[:, 9], minlength=len(instances))
    lace = np.array([materials[m].coverage_texture_ID > 0 for m in instances[:, 15]])
    pick = lambda mask: None if not mask.any() else int(np.argmax(np.where(mask, counts, -1)))
    out = {}
    for name, instance in (("mesh_deformed", pick(~lace)), ("lace_texcoords_scrolled", pick(lace))):
        if instance is not None:
            out[name] = dict(instance=instance, mesh=scene.model_info(int(instances[instance, 14]) & 0x3FFFFFFF)["mesh"], triangles=int(counts[instance]))
    return out


def rows_of(scene, mesh, name):
    d, r = scene.desc, scene.mesh_range(mesh)
    if name == "geometry":
        words = np.ctypeslib.as_array(C.cast(d.geometry, C.POINTER(C.c_uint32)), shape=(d.vertex_count, 4))[r["vertex_offset"]:r["vertex_offset"] + r["vertex_count"]].copy()
        return words.view(capi.vertex_geometry_dtype()).reshape(-1)
    return np.ctypeslib.as_array(d.texcoords, shape=(d.vertex_count * 2,)).reshape(-1, 2)[r["vertex_offset"]:r["vertex_offset"] + r["vertex_count"]].copy()


def alternatives(scene, name, mesh):
    """The two states the repeats alternate between, as edit lists."""
    if name == "mesh_deformed":
        rest = rows_of(scene, mesh, "geometry")
        bent = rest.copy()
        extent = float(np.ptp(rest["position"], axis=0).max()) or 1.0
        bent["position"] = rest["position"] + np.float32(0.02 * extent) * np.sin(np.float32(5.0 / extent) * rest["position"][:, [1, 2, 0]]).astype(np.float32)
        return [[dict(mesh=mesh, first=0, geometry=bent)], [dict(mesh=mesh, first=0, geometry=rest)]]
    rest = rows_of(scene, mesh, "texcoords")
    return [[dict(mesh=mesh, first=0, texcoords=rest + np.float32(0.125))], [dict(mesh=mesh, first=0, texcoords=rest)]]


def measure(triangles, seed, warmup, repeats):
    scene = Scene("atrium", param0=triangles, param1=seed, textured=True)
    ctx = Context(0)
    t0 = time.perf_counter()
    ctx.upload_scene(scene)
    ctx.synchronize()
    upload_ms = (time.perf_counter() - t0) * 1e3
    desc = scene.desc
    med = statistics.median
    out = dict(triangles=desc.triangle_count, vertices=desc.vertex_count, slots=desc.wide8_slot_count, upload_ms=upload_ms, edits={})
    for name, chosen in plan(scene).items():
        states = alternatives(scene, name, chosen["mesh"])
        vertices = scene.mesh_range(chosen["mesh"])["vertex_count"]
        rebuilt, refitted, device, catch_up, passes, answers = [], [], [], [], [], []
        note = None
        for k in range(warmup + repeats):      # the path of the parent commit: the edit is in the builder, then a new scene
            assert scene.update_vertices(states[k % 2], NEVER_REBUILD) is not None
            t0 = time.perf_counter()
            scene.rebuild()
            t1 = time.perf_counter()
            ctx.upload_scene(scene)
            ctx.synchronize()
            t2 = time.perf_counter()
            if k >= warmup:
                rebuilt.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
        for k in range(warmup + repeats):      # the host refit
            t0 = time.perf_counter()
            kept = scene.update_vertices(states[k % 2], NEVER_REBUILD)
            t1 = time.perf_counter()
            if kept is not True:
                note = "the host refit does not suffice: the builder rebuilt (a pair parted)"
                ctx.upload_scene(scene)
                break
            ctx.update_scene_geometry(scene)
            ctx.synchronize()
            t2 = time.perf_counter()
            if k >= warmup:
                refitted.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
        for k in range(warmup + repeats if note is None else 0):      # the device path
            t0 = time.perf_counter()
            pooled = scene.stage_vertex_edits(states[k % 2])
            t1 = time.perf_counter()
            answer = ctx.update_scene_vertices(pooled)
            ctx.synchronize()
            t2 = time.perf_counter()
            assert answer["status"] == capi.HIPR_OK and not answer["needs_rebuild"], answer
            scene.apply_staged(NEVER_REBUILD)
            t3 = time.perf_counter()
            if k >= warmup:
                device.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
                catch_up.append((t3 - t2) * 1e3)
                passes.append(ctx.vertex_update_times())
                answers.append((answer["moved_triangles"], answer["candidate_triangles"], answer["changed_triangles"]))
        out["edits"][name] = dict(chosen, vertices=vertices, note=note, rebuilt=rebuilt, refitted=refitted, device=device, catch_up=med(catch_up) if catch_up else None,
                                  passes={key: med(t[key] for t in passes) for key in passes[0]} if passes else None, answers=sorted(set(answers)))
        print(f"  ... {name} measured", file=sys.stderr, flush=True)
    ctx.close()
    return out


def leg(label, rows, parts):
    if not rows:
        return f"    {label:<13}not measured"
    total = [r[0] for r in rows]
    return (f"    {label:<13}{statistics.median(total):10.3f} ms  [{min(total):.3f} .. {max(total):.3f}]   = {parts[0]} {statistics.median(r[1] for r in rows):.3f} ms + "
            f"{parts[1]} {statistics.median(r[2] for r in rows):.3f} ms")


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scenes", nargs="+", default=list(SCENES), choices=list(SCENES))
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=10)
    p.add_argument("--out", default=str(ROOT / "profiles" / "vertex_update_device_vs_host.txt"))
    args = p.parse_args()
    lines = ["Vertices of a resident mesh of the textured procedural atrium edited: SceneBuilder::rebuild + hipr_upload_scene (the path every vertex edit took), the host refit",
             "(SceneBuilder::update_vertices + hipr_update_scene_geometry) and the device path (SceneBuilder::stage_vertex_edits + hipr_update_scene_vertices)",
             "(tools/vertex_update_probe.py).",
             f"Wall time around the calls, stream synchronised inside; median of {args.repeats} repeats after {args.warmup} warm-up repeats, [min .. max].",
             "passes: hipr_debug_vertex_update_times, medians -- the table and rows packed and their staging copy queued (host clock), the pool writes with the marks, the moved",
             "triangles with the refit passes and the records, the flag pass with the leaf pass. catch-up: SceneBuilder::apply_staged_transforms, due before the builder's",
             "description is next handed out, not per edit.", ""]
    for name in args.scenes:
        r = measure(*SCENES[name], args.warmup, args.repeats)
        lines += [f"{name}: {r['triangles']} triangles, {r['vertices']} vertices, {r['slots']} slots of the 8-wide tree (first scene upload: {r['upload_ms']:.1f} ms)"]
        for edit in EDITS:
            e = r["edits"].get(edit)
            if e is None:
                lines += [f"  {edit}: not measured (the scene has no such model)"]
                continue
            lines += [f"  {edit}: mesh {e['mesh']}, {e['vertices']} vertices, {e['triangles']} triangles of instance {e['instance']}; (moved, decided again, changed) per repeat: {e['answers']}",
                      leg("rebuild path", e["rebuilt"], ("rebuild", "hipr_upload_scene")), leg("host refit", e["refitted"], ("Scene.update_vertices", "hipr_update_scene_geometry")),
                      leg("device path", e["device"], ("Scene.stage_vertex_edits", "hipr_update_scene_vertices"))]
            if e["note"]:
                lines += [f"    note         {e['note']}"]
            if e["passes"]:
                q = e["passes"]
                lines += [f"    passes       staging {q['staging']:.3f} ms, writes {q['writes']:.3f} ms, refit {q['refit']:.3f} ms, flags {q['flags']:.3f} ms; catch-up {e['catch_up']:.3f} ms",
                          f"    rebuild / device = {statistics.median(x[0] for x in e['rebuilt']) / statistics.median(x[0] for x in e['device']):.1f}, "
                          f"host refit / device = {statistics.median(x[0] for x in e['refitted']) / statistics.median(x[0] for x in e['device']):.1f}"]
        lines.append("")
        print("\n".join(lines), flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")      # after every scene: a later one that runs out of time leaves the earlier figures


if __name__ == "__main__":
    main()
