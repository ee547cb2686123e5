#!/usr/bin/env python3
"""One material's roughness edited, two ways: the path every material change used to take -- a new scene: SceneBuilder::rebuild (the triangles flattened again, the
BVH2, the 4-wide and the 8-wide tree built) + hipr_upload_scene of every pool -- against the device path (hipr_update_scene_materials: the changed slot copied
into the resident pool and two short passes over the resident arrays, csrc/material_update.h).

Both legs are timed around the calls, with a stream synchronise inside the timed span, as the median of `--repeats` repeats after `--warmup` untimed ones; the
roughness alternates between two values so that every repeat changes it. The result of the two paths is the same bytes (tests/test_gpu_material_update.py).
The host leg leaves out what HIPRenderer::Renderer's full path does on top -- flattening the Bifrost managers into a new SceneBuilder -- so it flatters the host.

    python tools/material_update_probe.py --scenes atrium251k atrium10M --out profiles/material_update_device_vs_host.txt

The two named scenes are the project's own: the 251 424-triangle atrium of the headline benchmark (param0 = 260000, seed 1) and the 9 961 764-triangle atrium of
BASELINE config 5 (param0 = 10000000, seed 2).
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from bifrost3d_amd.host import Scene      # noqa: E402
from bifrost3d_amd.renderer import Context      # noqa: E402

SCENES = {"atrium251k": (260000, 1), "atrium10M": (10000000, 2)}      # name: (param0 = target triangle count, param1 = seed) of the procedural atrium
ROUGHNESS = (0.35, 0.8)


def a_material_in_use(scene):
    """The material most triangles wear: the edit with the most touched triangles."""
    import numpy as np
    triangles, instances = scene.triangles(), scene.instances_array()
    per_material = np.bincount(instances[triangles[:, 9], 15], minlength=len(scene.materials()))
    return int(per_material.argmax()), int(per_material.max())


def measure(triangles, seed, warmup, repeats, device_only=False):
    scene = Scene("atrium", param0=triangles, param1=seed)
    ctx = Context(0)
    t0 = time.perf_counter()
    ctx.upload_scene(scene)
    ctx.synchronize()
    upload_ms = (time.perf_counter() - t0) * 1e3
    desc = scene.desc
    index, touched = a_material_in_use(scene)
    host, device = [], []
    for k in range(0 if device_only else warmup + repeats):
        material = scene.materials()[index]
        material.roughness = ROUGHNESS[k % 2]
        assert scene.update_materials([(index, material)])      # the edit itself is in the builder either way; the parent's path then builds and uploads a new scene
        t0 = time.perf_counter()
        scene.rebuild()
        t1 = time.perf_counter()
        ctx.upload_scene(scene)
        ctx.synchronize()
        t2 = time.perf_counter()
        if k >= warmup:
            host.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
    for k in range(warmup + repeats):
        material = scene.materials()[index]
        material.roughness = ROUGHNESS[(k + 1) % 2]
        t0 = time.perf_counter()
        scene.update_materials([(index, material)])
        t1 = time.perf_counter()
        ctx.update_scene_materials([(index, material)])
        ctx.synchronize()
        t2 = time.perf_counter()
        if k >= warmup:
            device.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
    ctx.close()
    med = statistics.median
    host = host or [(float("nan"),) * 3]
    return dict(triangles=desc.triangle_count, slots=desc.wide8_slot_count, instances=desc.instance_count, material=index, touched=touched, upload_ms=upload_ms,
                host_ms=med(h[0] for h in host), host_build_ms=med(h[1] for h in host), host_upload_ms=med(h[2] for h in host), host_min=min(h[0] for h in host), host_max=max(h[0] for h in host),
                device_ms=med(d[0] for d in device), device_builder_ms=med(d[1] for d in device), device_call_ms=med(d[2] for d in device), device_min=min(d[0] for d in device),
                device_max=max(d[0] for d in device))


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scenes", nargs="+", default=list(SCENES), choices=list(SCENES))
    p.add_argument("--device-only", action="store_true", help="skip the host leg (for a kernel trace of the device leg)")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=10)
    p.add_argument("--out", default=str(ROOT / "profiles" / "material_update_device_vs_host.txt"))
    args = p.parse_args()
    lines = ["One material's roughness of the procedural atrium edited: SceneBuilder::rebuild + hipr_upload_scene (the path every material change took) against",
             "SceneBuilder::update_materials + hipr_update_scene_materials (tools/material_update_probe.py).",
             f"Wall time around the calls, stream synchronised inside; median of {args.repeats} repeats after {args.warmup} warm-up repeats, [min .. max].", ""]
    for name in args.scenes:
        r = measure(*SCENES[name], args.warmup, args.repeats, args.device_only)
        lines += [f"{name}: {r['triangles']} triangles, {r['slots']} slots of the 8-wide tree, {r['instances']} instances; material {r['material']} edited, worn by {r['touched']} triangles "
                  f"(first scene upload: {r['upload_ms']:.1f} ms)",
                  f"  host path    {r['host_ms']:10.3f} ms  [{r['host_min']:.3f} .. {r['host_max']:.3f}]   = rebuild {r['host_build_ms']:.3f} ms + hipr_upload_scene {r['host_upload_ms']:.3f} ms",
                  f"  device path  {r['device_ms']:10.3f} ms  [{r['device_min']:.3f} .. {r['device_max']:.3f}]   = Scene.update_materials {r['device_builder_ms']:.3f} ms + hipr_update_scene_materials {r['device_call_ms']:.3f} ms",
                  f"  host / device = {r['host_ms'] / r['device_ms']:.1f}", ""]
        print("\n".join(lines[-5:]), flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")      # after every scene: a later one that runs out of time leaves the earlier figures


if __name__ == "__main__":
    main()
