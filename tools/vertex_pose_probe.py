#!/usr/bin/env python3
"""A rigged mesh of the resident scene posed, four ways: on the device -- SceneBuilder::stage_rig_poses + hipr_pose_scene_rigs (csrc/vertex_pose.h), after which the
builder catches up with apply_staged_transforms whenever its description is next wanted (timed apart); host-skinned rows through the vertex update --
SceneBuilder::posed_geometry on one host thread + stage_vertex_edits + hipr_update_scene_vertices (posed_geometry checks and packs the rig on every call, which a
caller that keeps its rig would do once: the leg's host figure is somewhat above what such a caller pays); the host refit -- SceneBuilder::pose_rigs +
hipr_update_scene_geometry; and a new scene -- the pose in the builder, SceneBuilder::rebuild + hipr_upload_scene.

The rig lies over the mesh of the model with the most triangles of the textured procedural atrium: 32 joints along the mesh's longest axis (two neighbouring joints
per vertex, weights by position, so that coincident vertices stay coincident), 2 morph targets with target normals. The repeats alternate between two poses. All
legs are timed around the calls, with a stream synchronise inside the timed span, as the median of `--repeats` repeats after `--warmup` untimed ones; the device
call's own figures (hipr_debug_vertex_pose_times) are printed with it. The result of the paths is the same bytes (tests/test_gpu_vertex_pose.py).

The kernel alone: its bytes per vertex (counted here) against the device copy rate DESIGN.md section 5 quotes, as a fraction. The LDS budget: the same call with the
matrices staged in LDS and gathered from global memory, on the 32-joint rig and on a 300-joint one (hipr_debug_set_pose_lds_joints).

    python tools/vertex_pose_probe.py --scenes atrium251k atrium10M --out profiles/vertex_pose_device_vs_host.txt
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from bifrost3d_amd import capi      # noqa: E402
from bifrost3d_amd.host import Scene      # noqa: E402
from bifrost3d_amd.renderer import Context      # noqa: E402
from vertex_update_probe import SCENES, leg, plan, rows_of      # noqa: E402

NEVER_REBUILD = 1e30
COPY_RATE = 5.2e12      # bytes per second, DESIGN.md section 5
LDS_CAPACITY = 320      # csrc/vertex_pose.h POSE_LDS_CAPACITY


def decoded_normals(codes):
    """OctahedralNormal::decode, float32 unit vectors of the pool's codes."""
    f = codes.astype(np.float64)
    z = 32767.0 - np.abs(f[:, 0]) - np.abs(f[:, 1])
    t = np.maximum(-z, 0.0)
    n = np.stack([f[:, 0] + np.where(f[:, 0] >= 0, -t, t), f[:, 1] + np.where(f[:, 1] >= 0, -t, t), z], axis=1)
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)


def rig_over(scene, mesh, joints, targets=2):
    """The rig (MESH-relative) and its two poses. Everything is a function of the rest position, so coincident vertices stay coincident."""
    rest = rows_of(scene, mesh, "geometry")
    positions, count = rest["position"].copy(), len(rest)
    has_normals = bool(scene.mesh_range(mesh)["flags"] & 1)
    axis = int(np.argmax(np.ptp(positions, axis=0)))
    lo, extent = float(positions[:, axis].min()), float(np.ptp(positions[:, axis])) or 1.0
    along = np.clip((positions[:, axis] - lo) / extent, 0.0, 1.0) * (joints - 1)
    first = np.minimum(np.floor(along), joints - 2).astype(int)
    upper = (along - first).astype(np.float32)
    rig = dict(mesh=mesh, first=0, rest_positions=positions, joint_count=joints, joints=np.stack([first, first + 1, np.zeros(count, int), np.zeros(count, int)], axis=1).astype(np.uint16),
               weights=np.stack([np.float32(1.0) - upper, upper, np.zeros(count, np.float32), np.zeros(count, np.float32)], axis=1).astype(np.float32),
               target_positions=np.stack([np.float32(0.01 * extent) * np.sin(np.float32((3.0 + t) / extent) * positions[:, [1, 2, 0]]) for t in range(targets)]).astype(np.float32))
    if has_normals:
        rig["rest_normals"] = decoded_normals(rest["oct_normal"])
        rig["target_normals"] = (np.float32(0.1) * rig["target_positions"] / np.float32(0.01 * extent)).astype(np.float32)

    def pose(sign):
        matrices = np.tile(np.eye(3, 4, dtype=np.float32), (joints, 1, 1))
        k = np.arange(joints, dtype=np.float64)
        matrices[:, (axis + 1) % 3, 3] = (sign * 0.02 * extent * np.sin(k / joints * 6.0)).astype(np.float32)      # a wave travelling along the joints
        return dict(rig=0, matrices=matrices, weights=np.array([0.5 * sign, 0.25][:targets], np.float32))
    bytes_per_vertex = 32 + 16 + targets * 12 * (2 if has_normals else 1) + 17      # the rest row, the weights, the targets, the 16 bytes and the mark written
    return rig, [pose(1.0), pose(-1.0)], bytes_per_vertex


def measure(triangles, seed, warmup, repeats, new_scene_repeats):
    scene = Scene("atrium", param0=triangles, param1=seed, textured=True)
    ctx = Context(0)
    t0 = time.perf_counter()
    ctx.upload_scene(scene)
    ctx.synchronize()
    upload_ms = (time.perf_counter() - t0) * 1e3
    desc = scene.desc
    med = statistics.median
    chosen = plan(scene)["mesh_deformed"]
    mesh = chosen["mesh"]
    rig, poses, bytes_per_vertex = rig_over(scene, mesh, 32)
    vertices = len(rig["rest_positions"])
    assert scene.set_rigs([rig]) and ctx.set_scene_rigs(scene.pooled_rigs([rig])) == capi.HIPR_OK, ctx.lib.hipr_last_error()
    out = dict(chosen, scene_triangles=desc.triangle_count, scene_vertices=desc.vertex_count, upload_ms=upload_ms, vertices=vertices, bytes_per_vertex=bytes_per_vertex, note=None)
    device, catch_up, passes, skinned, refitted, rebuilt = [], [], [], [], [], []
    for k in range(warmup + repeats):      # the device path
        t0 = time.perf_counter()
        staged = scene.stage_rig_poses([poses[k % 2]])
        t1 = time.perf_counter()
        answer = ctx.pose_scene_rigs(staged)
        ctx.synchronize()
        t2 = time.perf_counter()
        assert answer["status"] == capi.HIPR_OK, ctx.lib.hipr_last_error()
        if answer["needs_rebuild"]:
            out["note"] = "the pose parts a pair of the tree: the scene awaits a rebuild, nothing is timed"
            ctx.close()
            return out
        scene.apply_staged(NEVER_REBUILD)
        t3 = time.perf_counter()
        if k >= warmup:
            device.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
            catch_up.append((t3 - t2) * 1e3)
            passes.append(ctx.vertex_pose_times())
    out["moved"] = answer["moved_triangles"]
    for k in range(warmup + repeats):      # host-skinned rows through the vertex update: skinned on one host thread, then hipr_update_scene_vertices
        t0 = time.perf_counter()
        rows = scene.posed_geometry(rig, poses[k % 2])
        pooled = scene.stage_vertex_edits([dict(mesh=mesh, first=0, geometry=rows)])
        t1 = time.perf_counter()
        answer = ctx.update_scene_vertices(pooled)
        ctx.synchronize()
        t2 = time.perf_counter()
        assert answer["status"] == capi.HIPR_OK and not answer["needs_rebuild"], answer
        scene.apply_staged(NEVER_REBUILD)
        if k >= warmup:
            skinned.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
    for k in range(warmup + repeats):      # the host refit
        t0 = time.perf_counter()
        assert scene.pose_rigs([poses[k % 2]], NEVER_REBUILD) is True
        t1 = time.perf_counter()
        ctx.update_scene_geometry(scene)
        ctx.synchronize()
        t2 = time.perf_counter()
        if k >= warmup:
            refitted.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
    for k in range(min(warmup, 1) + new_scene_repeats):      # a new scene
        assert scene.pose_rigs([poses[k % 2]], NEVER_REBUILD) is True
        t0 = time.perf_counter()
        scene.rebuild()
        t1 = time.perf_counter()
        ctx.upload_scene(scene)
        ctx.synchronize()
        t2 = time.perf_counter()
        if k >= min(warmup, 1):
            rebuilt.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
    # the LDS budget: the upload dropped the rigs; the 32-joint rig and a 300-joint one, each with its matrices in LDS and gathered
    budgets = {}
    for joints in (32, 300):
        other, other_poses, _ = rig_over(scene, mesh, joints)
        assert ctx.set_scene_rigs(scene.pooled_rigs([other])) == capi.HIPR_OK, ctx.lib.hipr_last_error()
        for label, budget in (("lds", LDS_CAPACITY), ("gathered", 0)):
            assert ctx.lib.hipr_debug_set_pose_lds_joints(ctx.handle, budget) == capi.HIPR_OK
            kernel = []
            for k in range(warmup + repeats):
                assert ctx.pose_scene_rigs([other_poses[k % 2]])["status"] == capi.HIPR_OK
                if k >= warmup:
                    kernel.append(ctx.vertex_pose_times()["pose"])
            budgets[(joints, label)] = (med(kernel), min(kernel), max(kernel))
    ctx.close()
    out.update(device=device, catch_up=med(catch_up), passes={key: med(t[key] for t in passes) for key in passes[0]}, skinned=skinned, refitted=refitted, rebuilt=rebuilt, budgets=budgets)
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scenes", nargs="+", default=list(SCENES), choices=list(SCENES))
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=10)
    p.add_argument("--new-scene-repeats", type=int, default=10, help="repeats of the new-scene leg (seconds each at 10 M triangles)")
    p.add_argument("--out", default=str(ROOT / "profiles" / "vertex_pose_device_vs_host.txt"))
    args = p.parse_args()
    lines = ["A rigged mesh of the textured procedural atrium posed (32 joints, 2 morph targets with normals): the device path (SceneBuilder::stage_rig_poses +",
             "hipr_pose_scene_rigs), host-skinned rows through the vertex update (SceneBuilder::posed_geometry on one host thread + stage_vertex_edits + hipr_update_scene_vertices), the host",
             "refit (SceneBuilder::pose_rigs + hipr_update_scene_geometry) and a new scene (SceneBuilder::rebuild + hipr_upload_scene) (tools/vertex_pose_probe.py).",
             f"Wall time around the calls, stream synchronised inside; median of {args.repeats} repeats after {args.warmup} warm-up repeats, [min .. max]; the new scene: {args.new_scene_repeats} repeats after 1.",
             "passes: hipr_debug_vertex_pose_times, medians -- the block table, matrices and weights packed and their staging copy queued (host clock), the pose kernel with the",
             "marks cleared, the moved triangles with the refit passes and the records. catch-up: SceneBuilder::apply_staged_transforms (it skins on the host), due before the",
             "builder's description is next handed out, not per pose. posed_geometry checks and packs the rig on every call, which a caller that keeps its rig would do once: the",
             "host-skinned leg's host figure is somewhat above what such a caller pays (not separated).",
             "the kernel: the event span holds the memsets of the marks (a byte per pool vertex) and of the words and the launch; it is given twice -- in the timed loop, where the",
             "builder's catch-up leaves the device idle between repeats (27 ms and 1.3 s), and back to back (the 32-joint line, matrices in LDS). Why the first is the slower one",
             "was not separated (supposed: the device's clocks after the pause). Both are a launch floor of about 0.02 ms, not a rate: no rig here is large enough to leave it, so",
             "the two matrix paths are told apart only where staging 14 KB per block costs more than that floor hides.", ""]
    for name in args.scenes:
        r = measure(*SCENES[name], args.warmup, args.repeats, args.new_scene_repeats)
        lines += [f"{name}: {r['scene_triangles']} triangles, {r['scene_vertices']} vertices (first scene upload: {r['upload_ms']:.1f} ms)",
                  f"  the rig: mesh {r['mesh']}, {r['vertices']} vertices, {r['triangles']} triangles of instance {r['instance']}"]
        if r["note"]:
            lines += [f"    note         {r['note']}", ""]
            continue
        q = r["passes"]
        device = statistics.median(x[0] for x in r["device"])
        kernel_bytes = r["vertices"] * r["bytes_per_vertex"]
        back = r["budgets"][(32, "lds")][0]
        lines += [f"  moved triangles per pose: {r['moved']}",
                  leg("device path", r["device"], ("Scene.stage_rig_poses", "hipr_pose_scene_rigs")),
                  leg("host-skinned", r["skinned"], ("Scene.posed_geometry + stage_vertex_edits", "hipr_update_scene_vertices")),
                  leg("host refit", r["refitted"], ("Scene.pose_rigs", "hipr_update_scene_geometry")),
                  leg("new scene", r["rebuilt"], ("rebuild", "hipr_upload_scene")),
                  f"    passes       staging {q['staging']:.3f} ms, pose kernel {q['pose']:.4f} ms, refit {q['refit']:.3f} ms; catch-up {r['catch_up']:.3f} ms",
                  f"    host-skinned / device = {statistics.median(x[0] for x in r['skinned']) / device:.2f}, host refit / device = {statistics.median(x[0] for x in r['refitted']) / device:.1f}, "
                  f"new scene / device = {statistics.median(x[0] for x in r['rebuilt']) / device:.1f}",
                  f"    the kernel   {r['bytes_per_vertex']} bytes per vertex (rest row 32, weights 16, targets {r['bytes_per_vertex'] - 65}, written 17) x {r['vertices']} = {kernel_bytes} bytes: in the timed loop "
                  f"{q['pose']:.4f} ms = {kernel_bytes / (q['pose'] * 1e-3) / 1e9:.1f} GB/s, {kernel_bytes / (q['pose'] * 1e-3) / COPY_RATE:.4f} of the 5.2 TB/s copy rate; back to back "
                  f"{back:.4f} ms = {kernel_bytes / (back * 1e-3) / 1e9:.1f} GB/s, {kernel_bytes / (back * 1e-3) / COPY_RATE:.4f} of it"]
        for joints in (32, 300):
            lds, gathered = r["budgets"][(joints, "lds")], r["budgets"][(joints, "gathered")]
            lines += [f"    {joints:>3} joints   matrices in LDS {lds[0]:.4f} ms [{lds[1]:.4f} .. {lds[2]:.4f}], gathered from global memory {gathered[0]:.4f} ms [{gathered[1]:.4f} .. {gathered[2]:.4f}]"]
        lines.append("")
        print("\n".join(lines), flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")      # after every scene: a later one that runs out of time leaves the earlier figures


if __name__ == "__main__":
    main()
