#!/usr/bin/env python3
"""One moved model, two ways: the host path (SceneBuilder::update_model_transforms + hipr_update_scene_geometry: a host refit of three trees and a re-upload of
nodes, triangles, instances and slots) against the device path (hipr_refit_scene_transforms: kernels over the resident arrays, csrc/wide8_refit.h).

Both legs are timed around the calls, with a stream synchronise inside the timed span, as the median of `--repeats` repeats after `--warmup` untimed ones; the
model alternates between two poses so that every repeat moves it. The result of the two paths is the same bytes (tests/test_gpu_device_refit.py).

    python tools/refit_probe.py --scenes atrium251k atrium10M --out profiles/refit_device_vs_host.txt

The two named scenes are the project's own: the 251 424-triangle atrium of the headline benchmark (param0 = 260000, seed 1) and the 9 961 764-triangle atrium of
BASELINE config 5 (param0 = 10000000, seed 2). Where the device leg loses, its time per pass is the kernel table of

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/refit_probe.py --scenes atrium10M --device-only --out <file>

(k_refit_triangles + k_refit_bounds_final = pass 1, k_refit_leaves = 2, k_refit_nodes = 3, k_refit_area* = 4, k_build_*_triangles = the derived records); what the
wall time holds beyond the kernels is the instance upload and the two read-backs the host waits for.
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from bifrost3d_amd.host import Scene      # noqa: E402
from bifrost3d_amd.renderer import Context      # noqa: E402

SCENES = {"atrium251k": (260000, 1), "atrium10M": (10000000, 2)}      # name: (param0 = target triangle count, param1 = seed) of the procedural atrium
POSES = [dict(translation=(0.05, -0.30, 0.10), rotation=(0.0, float(np.sin(0.4)), 0.0, float(np.cos(0.4))), scale=0.3),
         dict(translation=(0.2, -0.35, -0.2), rotation=(0.0, float(np.sin(np.pi / 12)), 0.0, float(np.cos(np.pi / 12))), scale=0.3)]


def a_model_that_refits(triangles, seed):
    """The first model whose move to both poses keeps the topology on the host (no rebuild), found on a scratch scene. A candidate that does not refit costs a
    build of the scratch scene (seconds at 10 M triangles); --model names the model and skips the search."""
    scratch = Scene("atrium", param0=triangles, param1=seed)      # a move that does not refit rebuilds the scratch scene, which stays a scene of the same models
    for model in range(1, 65):
        if not scratch.model_pose(model, **POSES[0]):
            continue
        if all(scratch.move_model(model, rebuild_threshold=1e30, **pose) for pose in POSES):
            return model
    raise SystemExit("no model of the scene refits under both poses")


def measure(triangles, seed, warmup, repeats, model=0, device_only=False):
    model = model or a_model_that_refits(triangles, seed)
    scene = Scene("atrium", param0=triangles, param1=seed)
    ctx = Context(0)
    t0 = time.perf_counter()
    ctx.upload_scene(scene)
    ctx.synchronize()
    upload_ms = (time.perf_counter() - t0) * 1e3
    desc = scene.desc
    instances_moved = len(scene.model_pose(model, **POSES[0]))
    host, device = [], []
    for k in range(0 if device_only else warmup + repeats):
        pose = POSES[k % 2]
        t0 = time.perf_counter()
        kept = scene.move_model(model, rebuild_threshold=1e30, **pose)
        t1 = time.perf_counter()
        ctx.update_scene_geometry(scene)
        ctx.synchronize()
        t2 = time.perf_counter()
        assert kept
        if k >= warmup:
            host.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
    for k in range(warmup + repeats):
        pose = POSES[(k + 1) % 2]
        t0 = time.perf_counter()
        result = ctx.refit_scene_transforms(scene.model_pose(model, **pose))
        ctx.synchronize()
        t1 = time.perf_counter()
        assert not result["needs_rebuild"]
        if k >= warmup:
            device.append((t1 - t0) * 1e3)
    ctx.close()
    med = statistics.median
    host = host or [(float("nan"),) * 3]
    return dict(triangles=desc.triangle_count, slots=desc.wide8_slot_count, instances=desc.instance_count, model=model, instances_moved=instances_moved, upload_ms=upload_ms,
                host_ms=med(h[0] for h in host), host_refit_ms=med(h[1] for h in host), host_upload_ms=med(h[2] for h in host), host_min=min(h[0] for h in host), host_max=max(h[0] for h in host),
                device_ms=med(device), device_min=min(device), device_max=max(device), repeats=repeats, warmup=warmup)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scenes", nargs="+", default=list(SCENES), choices=list(SCENES))
    p.add_argument("--model", type=int, default=0, help="the model to move (default: the first one that refits under both poses)")
    p.add_argument("--device-only", action="store_true", help="skip the host leg (for a kernel trace of the device leg)")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=10)
    p.add_argument("--out", default=str(ROOT / "profiles" / "refit_device_vs_host.txt"))
    args = p.parse_args()
    lines = ["One model of the procedural atrium moved: host refit + hipr_update_scene_geometry against hipr_refit_scene_transforms (tools/refit_probe.py).",
             f"Wall time around the calls, stream synchronised inside; median of {args.repeats} repeats after {args.warmup} warm-up repeats, [min .. max].", ""]
    for name in args.scenes:
        r = measure(*SCENES[name], args.warmup, args.repeats, args.model, args.device_only)
        lines += [f"{name}: {r['triangles']} triangles, {r['slots']} slots of the 8-wide tree, {r['instances']} instances; model {r['model']} moved (scene upload: {r['upload_ms']:.1f} ms)",
                  f"  host path    {r['host_ms']:10.3f} ms  [{r['host_min']:.3f} .. {r['host_max']:.3f}]   = move_model {r['host_refit_ms']:.3f} ms + hipr_update_scene_geometry {r['host_upload_ms']:.3f} ms",
                  f"  device path  {r['device_ms']:10.3f} ms  [{r['device_min']:.3f} .. {r['device_max']:.3f}]",
                  f"  host / device = {r['host_ms'] / r['device_ms']:.1f}", ""]
        print("\n".join(lines[-5:]), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
