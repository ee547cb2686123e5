#!/usr/bin/env python3
"""A model dragged far, three ways: the resident scene's trees rebuilt on the device from the triangles it holds (hipr_refit_scene_transforms, which asks for the
rebuild, + hipr_rebuild_scene_trees + SceneBuilder::adopt_rebuilt_trees; csrc/scene_rebuild.h) against the paths the same edit takes without it -- the pose staged,
rebuild() + hipr_upload_scene, and the same with both build stages on the device (what HIPR_DEVICE_BUILD=1 gives HIPRenderer::Renderer).

Wall time around the calls with the stream synchronised inside, the median of `--repeats` repeats after `--warmup` untimed ones. The model alternates between two far
poses, so that every repeat stretches the tree of the repeat before past the 1.5 rule and no repeat needs a new scene. The device's split is the library's own
(hipr_debug_rebuild_times) and adds up to the call.

    python tools/device_rebuild_probe.py --scenes atrium251k atrium10M --out profiles/device_rebuild_vs_host.txt
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

# Far enough that the handful of boxes above the model outweigh the summed half area of a tree over ten million triangles (the refit's rule compares sums over all boxes).
POSES = (dict(translation=(400.0, 100.0, -250.0)), dict(translation=(-400.0, 100.0, 250.0)))


def device_path(scene, ctx, model, warmup, repeats):
    ctx.upload_scene(scene)
    rows = []
    for k in range(warmup + repeats):
        pose = POSES[k % 2]
        moved = scene.model_pose(model, **pose)
        with captured_stderr():
            t0 = time.perf_counter()
            refit = ctx.refit_scene_transforms(moved)
            t1 = time.perf_counter()
            rebuilt = ctx.rebuild_scene_trees()
            ctx.synchronize()
            t2 = time.perf_counter()
            assert rebuilt["status"] == capi.HIPR_OK, ctx.lib.hipr_last_error()
            adopted = scene.stage_model(model, **pose) and scene.adopt_trees(rebuilt["nodes"], rebuilt["order"], rebuilt["deepest"], rebuilt["slots"], rebuilt["raw"].wide8)
            t3 = time.perf_counter()
        assert adopted, "the scene builder refused the device's trees"
        assert refit["needs_rebuild"] or refit["child_half_area"] > 1.5 * refit["uploaded_half_area"], "the move does not ask for a rebuild"
        if k >= warmup:
            rows.append(dict(total=(t3 - t0) * 1e3, refit=(t1 - t0) * 1e3, rebuild=(t2 - t1) * 1e3, adoption=(t3 - t2) * 1e3, **ctx.rebuild_times()))
    same = all(np.array_equal(ctx.read_scene_buffer(which), expected) for which, expected in
               ((capi.SCENE_BUFFER_TRIANGLES, scene.triangles()), (capi.SCENE_BUFFER_WIDE8_SLOTS, scene.wide8_slots()), (capi.SCENE_BUFFER_NODES, scene.nodes())))
    med = statistics.median
    out = {key: med(r[key] for r in rows) for key in rows[0]}
    out.update(low=min(r["total"] for r in rows), high=max(r["total"] for r in rows), same=same, nodes=rebuilt["node_count"], slots=rebuilt["wide8"]["slot_count"])
    return out


def host_path(scene, ctx, model, warmup, repeats):
    """What the renderer class does for the same edit without the device rebuild: the pose staged in the instances, SceneBuilder::rebuild(), hipr_upload_scene."""
    walls = []
    for k in range(warmup + repeats):
        with captured_stderr():
            t0 = time.perf_counter()
            staged = scene.stage_model(model, **POSES[k % 2])
            scene.rebuild()
            t1 = time.perf_counter()
            ctx.upload_scene(scene)
            ctx.synchronize()
            t2 = time.perf_counter()
        assert staged, "the pose turns the model inside out"
        if k >= warmup:
            walls.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
    med = statistics.median
    return dict(total=med(w[0] for w in walls), rebuild=med(w[1] for w in walls), upload=med(w[2] for w in walls), low=min(w[0] for w in walls), high=max(w[0] for w in walls))


def measure(triangles, seed, model, warmup, repeats):
    os.environ.pop("HIPR_DEVICE_COLLAPSE", None)
    ctx = Context(0)
    scene = Scene("atrium", param0=triangles, param1=seed)
    count = scene.desc.triangle_count
    device = device_path(scene, ctx, model, warmup, repeats)
    host = host_path(scene, ctx, model, warmup, repeats)
    scene.use_device_builder(ctx)
    both = host_path(scene, ctx, model, warmup, repeats)
    counts = dict(scene.build_counts(), **scene.collapse_counts())
    scene.use_device_builder(None)
    ctx.close()
    return dict(triangles=count, device=device, host=host, both=both, counts=counts)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scenes", nargs="+", default=list(SCENES), choices=list(SCENES))
    p.add_argument("--model", type=int, default=10, help="the model that is dragged (1-based, in creation order)")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=10)
    p.add_argument("--out", default=str(ROOT / "profiles" / "device_rebuild_vs_host.txt"))
    args = p.parse_args()
    lines = ["Output of tools/device_rebuild_probe.py; anything after the line 'Reading' at the end is commentary written by hand.", "",
             f"Model {args.model} of the procedural atrium dragged between two far poses, each move past the 1.5 rule: the trees rebuilt on the device from the resident triangles against the host's rebuild + upload.",
             f"Wall time around the calls, stream synchronised inside; median of {args.repeats} repeats after {args.warmup} warm-up repeats, [min .. max].",
             "The device split is the library's own (hipr_debug_rebuild_times) and adds up to hipr_rebuild_scene_trees.", ""]
    for name in args.scenes:
        r = measure(*SCENES[name], args.model, args.warmup, args.repeats)
        d, h, b = r["device"], r["host"], r["both"]
        kernels = d["flatten"] + d["bvh2"] + d["collapse"] + d["install"]
        lines += [f"{name}: {r['triangles']} triangles -> {d['nodes']} BVH2 nodes, {d['slots']} slots; the resident triangles, nodes and slots {'equal' if d['same'] else 'DIFFER FROM'} the adopted description's",
                  f"  device rebuild                    {d['total']:10.3f} ms  [{d['low']:.3f} .. {d['high']:.3f}]  = refit {d['refit']:.3f} + hipr_rebuild_scene_trees {d['rebuild']:.3f} + adoption {d['adoption']:.3f} ms",
                  f"      hipr_rebuild_scene_trees      = flatten order {d['flatten']:.3f} + BVH2 {d['bvh2']:.3f} + hand-over, collapse and the slots copied to the host {d['collapse']:.3f} + new resident arrays {d['install']:.3f}"
                  f" (together {kernels:.3f}) + read-back of nodes, order and slots {d['readback']:.3f} ms",
                  f"  host: stage + rebuild() + upload  {h['total']:10.3f} ms  [{h['low']:.3f} .. {h['high']:.3f}]  = rebuild {h['rebuild']:.3f} + upload {h['upload']:.3f} ms",
                  f"  the same, both stages on device   {b['total']:10.3f} ms  [{b['low']:.3f} .. {b['high']:.3f}]  = rebuild {b['rebuild']:.3f} + upload {b['upload']:.3f} ms"
                  f"  (BVH2 builds through the device {r['counts']['device_builds']}, declined {r['counts']['declined_builds']}; collapses {r['counts']['device_collapses']}, declined {r['counts']['declined_collapses']})",
                  f"  host / device rebuild = {h['total'] / d['total']:.2f}, both stages on device / device rebuild = {b['total'] / d['total']:.2f}", ""]
        print("\n".join(lines[-7:]), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
