#!/usr/bin/env python3
"""The 8-wide collapse of a scene's BVH2, two ways: the host's build_wide8 (host/Wide8Builder.cpp) against the device collapse that produces the same slots byte for
byte (hipr_build_wide8, csrc/wide8_build.h).

Two measurements per scene, both wall time around the calls with the stream synchronised inside, the median of `--repeats` repeats after `--warmup` untimed ones:

  (a) the collapse stage: hipr_build_wide8 in total, with its index walk / upload / kernels / read-back split (hipr_debug_collapse_times), against the 8-wide collapse
      stage of build_bvh as HIPR_BVH_TIMING=1 prints it in the same run;
  (b) the whole rebuild: SceneBuilder::rebuild() + hipr_upload_scene in three configurations -- the host builds everything, the BVH2 comes from the device
      (HIPR_DEVICE_COLLAPSE=0), both stages come from the device -- with the stage split as HIPR_BVH_TIMING=1 prints it.

    python tools/device_collapse_probe.py --scenes atrium251k atrium10M --out profiles/device_collapse_vs_host.txt
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
from device_build_probe import SCENES, captured_stderr, rebuild_and_upload      # noqa: E402
import device_collapse_bindings as collapse      # noqa: E402


def measure(triangles, seed, warmup, repeats):
    os.environ["HIPR_BVH_TIMING"] = "1"
    os.environ.pop("HIPR_DEVICE_COLLAPSE", None)
    with captured_stderr():
        scene = Scene("atrium", param0=triangles, param1=seed)
        host_trees = collapse.host_collapse(scene.triangles())      # the BVH2, the order and the host's slots over the scene's triangles: the stand-alone input of (a)
    ctx = Context(0)
    device, split = [], []
    room = np.zeros((2 * len(host_trees["triangles"]), 16), np.uint32)      # the caller's room for the slots, allocated (and paged in) once: build_bvh's is untouched memory
    for k in range(warmup + repeats):
        with captured_stderr():
            t0 = time.perf_counter()
            status, slots, result = ctx.build_wide8(host_trees["nodes"], host_trees["triangles"], host_trees["order"], slots=room)
            ctx.synchronize()
            t1 = time.perf_counter()
        assert status == capi.HIPR_OK, ctx.lib.hipr_last_error()
        if k >= warmup:
            device.append((t1 - t0) * 1e3)
            split.append(ctx.collapse_times())
    same = result["slot_count"] == len(host_trees["wide8"]["slots"]) and bool((slots == host_trees["wide8"]["slots"]).all())
    host = rebuild_and_upload(scene, ctx, warmup, repeats)
    os.environ["HIPR_DEVICE_COLLAPSE"] = "0"
    scene.use_device_builder(ctx)
    bvh2_only = rebuild_and_upload(scene, ctx, warmup, repeats)
    os.environ["HIPR_DEVICE_COLLAPSE"] = "1"
    scene.use_device_builder(ctx)
    both = rebuild_and_upload(scene, ctx, warmup, repeats)
    counts = dict(scene.build_counts(), **scene.collapse_counts())
    os.environ.pop("HIPR_DEVICE_COLLAPSE", None)
    ctx.close()
    med = statistics.median
    return dict(triangles=len(host_trees["triangles"]), nodes=len(host_trees["nodes"]), result=result, same=same, device_ms=med(device), device_low=min(device), device_high=max(device),
                validate=med(s["validate"] for s in split), upload=med(s["upload"] for s in split), kernels=med(s["kernels"] for s in split), readback=med(s["readback"] for s in split),
                host=host, bvh2_only=bvh2_only, both=both, counts=counts)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scenes", nargs="+", default=list(SCENES), choices=list(SCENES))
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=10)
    p.add_argument("--out", default=str(ROOT / "profiles" / "device_collapse_vs_host.txt"))
    args = p.parse_args()
    lines = ["Output of tools/device_collapse_probe.py; anything after the line 'Reading' at the end is commentary written by hand.", "",
             "The 8-wide collapse of the procedural atrium's BVH2: the host's build_wide8 against hipr_build_wide8, which collapses to the same slots on the device (tools/device_collapse_probe.py).",
             f"Wall time around the calls, stream synchronised inside; median of {args.repeats} repeats after {args.warmup} warm-up repeats, [min .. max]. Host stages as HIPR_BVH_TIMING=1 prints them, in the same run.",
             "The device split is the library's own (hipr_debug_collapse_times) and adds up to the call.", ""]
    for name in args.scenes:
        r = measure(*SCENES[name], args.warmup, args.repeats)
        h, b, d, w = r["host"], r["bvh2_only"], r["both"], r["result"]
        faster = r["device_ms"] < h["wide8"]
        lines += [f"{name}: {r['triangles']} triangles, {r['nodes']} BVH2 nodes -> {w['slot_count']} slots ({w['node_count']} nodes, {w['leaf_count']} records of which {w['paired_leaves']} hold two triangles, height {w['height']});"
                  f" the device's slots {'equal' if r['same'] else 'DIFFER FROM'} the host's",
                  f"  (a) 8-wide collapse   host   {h['wide8']:10.3f} ms  ({int(h['threads'])} threads; the median of the same repeats of a figure printed in whole milliseconds, and so are the stages below)",
                  f"                        device {r['device_ms']:10.3f} ms  [{r['device_low']:.3f} .. {r['device_high']:.3f}]  = index walk and checks {r['validate']:.3f} + allocation and upload {r['upload']:.3f} + kernels {r['kernels']:.3f} + read-back {r['readback']:.3f} ms"
                  f" (transfers {100 * (r['upload'] + r['readback']) / max(r['validate'] + r['upload'] + r['kernels'] + r['readback'], 1e-9):.0f} %)",
                  f"                        host / device = {h['wide8'] / r['device_ms']:.2f}" + ("" if faster else "   -- the device stage is NOT faster than the host stage here"),
                  "  (b) rebuild() + hipr_upload_scene"]
        for label, v in (("host only       ", h), ("BVH2 on device  ", b), ("both on device  ", d)):
            lines += [f"        {label} {v['total']:10.3f} ms  [{v['low']:.3f} .. {v['high']:.3f}]  = rebuild {v['rebuild']:.3f} + upload {v['upload']:.3f} ms;"
                      f" flatten {v['flatten']:.3f}, BVH2 {v['bvh2']:.3f}{' (device)' if v['source'] == 'used' else ''}, 4-wide collapse {v['wide4']:.3f}, 8-wide collapse {v['wide8']:.3f} ms"]
        lines += [f"        host only / both on device = {h['total'] / d['total']:.2f}, BVH2 on device / both on device = {b['total'] / d['total']:.2f};"
                  f" BVH2 builds through the device {r['counts']['device_builds']} (declined {r['counts']['declined_builds']}), collapses {r['counts']['device_collapses']} (declined {r['counts']['declined_collapses']})", ""]
        print("\n".join(lines[-9:]), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
