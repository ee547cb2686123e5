#!/usr/bin/env python3
"""A model destroyed and a copy of another created, three ways: the resident scene edited on the device (SceneBuilder::remove_model / insert_model staged,
hipr_edit_scene_instances, SceneBuilder::adopt_edited_trees; csrc/instance_edit.h) against the paths the same edit takes without it -- remove_model / insert_model,
rebuild() + hipr_upload_scene, and the same with both build stages on the device (what HIPR_DEVICE_BUILD=1 gives HIPRenderer::Renderer).

Wall time around the calls with the stream synchronised inside, the median of `--repeats` repeats after `--warmup` untimed ones. Every repeat removes the copy the repeat
before created and creates one at the other of two poses, so the scene keeps its size and no repeat needs a new scene. The device's split is the library's own
(hipr_debug_rebuild_times) and adds up to the call.

    python tools/instance_edit_probe.py --scenes atrium251k atrium10M --out profiles/instance_edit_device_vs_host.txt
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

POSES = (dict(translation=(0.6, 0.4, -0.8), scale=0.7), dict(translation=(-1.5, 0.2, 1.1), scale=1.0))
FIRST_COPY = 1000      # the model indices of the copies: FIRST_COPY + the repeat that created them


def stage(scene, source, k):
    """The edit of repeat k: the copy of repeat k - 1 goes, a copy of `source`'s mesh comes at the other pose, in the middle of the instance list."""
    if k > 0:
        assert scene.remove_model(FIRST_COPY + k - 1)
    scene.insert_model(source["position"] + 1, source["mesh"], source["material"], model_index=FIRST_COPY + k, **POSES[k % 2])


def device_path(scene, ctx, source, first, warmup, repeats):
    rows = []
    for k in range(first, first + warmup + repeats):
        with captured_stderr():
            t0 = time.perf_counter()
            stage(scene, source, k)
            edits = scene.staged_instance_edits()
            t1 = time.perf_counter()
            edited = ctx.edit_scene_instances(edits)
            ctx.synchronize()
            t2 = time.perf_counter()
            assert edited["status"] == capi.HIPR_OK, ctx.lib.hipr_last_error()
            adopted = scene.adopt_edited_trees(edited["nodes"], edited["order"], edited["deepest"], edited["slots"], edited["raw"].wide8)
            t3 = time.perf_counter()
        assert adopted, "the scene builder refused the device's trees"
        if k >= first + warmup:
            rows.append(dict(total=(t3 - t0) * 1e3, staging=(t1 - t0) * 1e3, edit=(t2 - t1) * 1e3, adoption=(t3 - t2) * 1e3, **ctx.rebuild_times()))
    same = all(np.array_equal(ctx.read_scene_buffer(which), expected) for which, expected in
               ((capi.SCENE_BUFFER_TRIANGLES, scene.triangles()), (capi.SCENE_BUFFER_WIDE8_SLOTS, scene.wide8_slots()), (capi.SCENE_BUFFER_NODES, scene.nodes()),
                (capi.SCENE_BUFFER_INSTANCES, scene.instances_array())))
    med = statistics.median
    out = {key: med(r[key] for r in rows) for key in rows[0]}
    out.update(low=min(r["total"] for r in rows), high=max(r["total"] for r in rows), same=same, triangles=edited["triangle_count"], nodes=edited["node_count"], slots=edited["wide8"]["slot_count"])
    return out


def host_path(scene, ctx, source, first, warmup, repeats):
    """What the renderer class does for the same edit without the device path, given a scene builder that keeps its pools: the edit, SceneBuilder::rebuild(), hipr_upload_scene."""
    walls = []
    for k in range(first, first + warmup + repeats):
        with captured_stderr():
            t0 = time.perf_counter()
            stage(scene, source, k)
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
    per = warmup + repeats
    ctx.upload_scene(scene)
    device = device_path(scene, ctx, source, 0, warmup, repeats)
    host = host_path(scene, ctx, source, per, warmup, repeats)
    scene.use_device_builder(ctx)
    both = host_path(scene, ctx, source, 2 * per, warmup, repeats)
    counts = dict(scene.build_counts(), **scene.collapse_counts())
    scene.use_device_builder(None)
    ctx.close()
    return dict(device=device, host=host, both=both, counts=counts)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scenes", nargs="+", default=list(SCENES), choices=list(SCENES))
    p.add_argument("--model", type=int, default=10, help="the model whose mesh is drawn again (1-based, in creation order)")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=10)
    p.add_argument("--out", default=str(ROOT / "profiles" / "instance_edit_device_vs_host.txt"))
    args = p.parse_args()
    lines = ["Output of tools/instance_edit_probe.py; anything after the line 'Reading' at the end is commentary written by hand.", "",
             f"A copy of model {args.model} of the procedural atrium destroyed and another created per repeat: the resident scene edited on the device against the host's rebuild + upload.",
             f"Wall time around the calls, stream synchronised inside; median of {args.repeats} repeats after {args.warmup} warm-up repeats, [min .. max].",
             "The device split is the library's own (hipr_debug_rebuild_times) and adds up to hipr_edit_scene_instances.", ""]
    for name in args.scenes:
        r = measure(*SCENES[name], args.model, args.warmup, args.repeats)
        d, h, b = r["device"], r["host"], r["both"]
        kernels = d["flatten"] + d["bvh2"] + d["collapse"] + d["install"]
        lines += [f"{name}: {d['triangles']} triangles -> {d['nodes']} BVH2 nodes, {d['slots']} slots; the resident triangles, instances, nodes and slots {'equal' if d['same'] else 'DIFFER FROM'} the adopted description's",
                  f"  device edit                        {d['total']:10.3f} ms  [{d['low']:.3f} .. {d['high']:.3f}]  = staging {d['staging']:.3f} + hipr_edit_scene_instances {d['edit']:.3f} + adoption {d['adoption']:.3f} ms",
                  f"      hipr_edit_scene_instances      = count, flatten order and new triangles {d['flatten']:.3f} + BVH2 {d['bvh2']:.3f} + hand-over, collapse and the slots copied to the host {d['collapse']:.3f}"
                  f" + new resident arrays {d['install']:.3f} (together {kernels:.3f}) + read-back of nodes, order and slots {d['readback']:.3f} ms",
                  f"  host: edit + rebuild() + upload    {h['total']:10.3f} ms  [{h['low']:.3f} .. {h['high']:.3f}]  = rebuild {h['rebuild']:.3f} + upload {h['upload']:.3f} ms",
                  f"  the same, both stages on device    {b['total']:10.3f} ms  [{b['low']:.3f} .. {b['high']:.3f}]  = rebuild {b['rebuild']:.3f} + upload {b['upload']:.3f} ms"
                  f"  (BVH2 builds through the device {r['counts']['device_builds']}, declined {r['counts']['declined_builds']}; collapses {r['counts']['device_collapses']}, declined {r['counts']['declined_collapses']})",
                  f"  host / device edit = {h['total'] / d['total']:.2f}, both stages on device / device edit = {b['total'] / d['total']:.2f}", ""]
        print("\n".join(lines[-7:]), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
