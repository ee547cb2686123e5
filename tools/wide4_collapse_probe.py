#!/usr/bin/env python3
"""The 4-wide collapse of a scene's BVH2, two ways: the host's WideCollapse (host/BvhBuilder.cpp) against the device collapse that produces the same nodes byte for
byte (hipr_build_wide4, csrc/wide4_build.h).

Three measurements per scene, all wall time around the calls with the stream synchronised inside, the median of `--repeats` repeats after `--warmup` untimed ones:

  (a) the collapse stage: hipr_build_wide4 in total, with its index walk / upload / kernels / read-back split (hipr_debug_collapse4_times), against the host's collapse
      alone over the same BVH2 on 16 threads (hiprh_wide4_collapse), timed in the same run;
  (b) the whole rebuild: SceneBuilder::rebuild() + hipr_upload_scene with two device stages (BVH2, 8-wide collapse) against three, with the stage split as
      HIPR_BVH_TIMING=1 prints it;
  (c) the instance-edit tick -- a model destroyed and a copy created, hipr_edit_scene_instances, SceneBuilder::adopt_edited_trees -- with the adoption's 4-wide collapse
      on the host against on the device.

The default of HIPR_DEVICE_COLLAPSE4 follows (b): on where three stages are faster than two at both sizes, beyond the spread of the repeats (the median with three stages
below the fastest repeat with two).

    python tools/wide4_collapse_probe.py --scenes atrium251k atrium10M --out profiles/wide4_collapse_vs_host.txt
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
from bifrost3d_amd.host import Scene, load_host_library      # noqa: E402
from bifrost3d_amd.renderer import Context      # noqa: E402
from device_build_probe import SCENES, captured_stderr, rebuild_and_upload      # noqa: E402
from instance_edit_probe import device_path      # noqa: E402

HOST_THREADS = 16
EDITED_MODEL = 10


def words(pointer, rows):
    import ctypes as C
    return np.ctypeslib.as_array(C.cast(pointer, C.POINTER(C.c_uint32)), shape=(rows, 16)).copy()


def measure(triangles, seed, warmup, repeats):
    os.environ["HIPR_BVH_TIMING"] = "1"
    os.environ["HIPR_DEVICE_COLLAPSE"] = "1"
    os.environ["HIPR_DEVICE_COLLAPSE4"] = "0"
    lib = load_host_library()
    with captured_stderr():
        scene = Scene("atrium", param0=triangles, param1=seed)
    nodes = scene.nodes()
    d = scene.desc
    host_wide = words(d.wide_nodes, d.wide_node_count)
    ctx = Context(0)
    # (a)
    room = np.zeros((len(nodes), 16), np.uint32)      # the caller's room for the nodes, allocated (and paged in) once
    device, split, host = [], [], []
    for k in range(warmup + repeats):
        with captured_stderr():
            t0 = time.perf_counter()
            status, wide, result = ctx.build_wide4(nodes, d.triangle_count, wide=room)
            ctx.synchronize()
            t1 = time.perf_counter()
            handle = lib.hiprh_wide4_collapse(nodes.ctypes.data, len(nodes), HOST_THREADS, None)
            t2 = time.perf_counter()
        assert status == capi.HIPR_OK, ctx.lib.hipr_last_error()
        assert handle
        lib.hiprh_bvh_destroy(handle)
        if k >= warmup:
            device.append((t1 - t0) * 1e3)
            split.append(ctx.collapse4_times())
            host.append((t2 - t1) * 1e3)
    same = result["node_count"] == len(host_wide) and result["stack_entries"] == d.wide_stack_entries and bool((wide == host_wide).all())
    # (b)
    scene.use_device_builder(ctx)
    two = rebuild_and_upload(scene, ctx, warmup, repeats)
    os.environ["HIPR_DEVICE_COLLAPSE4"] = "1"
    scene.use_device_builder(ctx)
    three = rebuild_and_upload(scene, ctx, warmup, repeats)
    counts = dict(scene.build_counts(), **scene.collapse_counts())
    counts4 = scene.wide4_collapse_counts()
    # (c): the sources stay installed for the adoption; the tick itself is the device edit either way
    source = scene.model_info(EDITED_MODEL)
    per = warmup + repeats
    ctx.upload_scene(scene)
    scene.use_device_wide4(None)
    edit_host = device_path(scene, ctx, source, 0, warmup, repeats)
    scene.use_device_wide4(ctx)
    before = scene.wide4_collapse_counts()["device_collapses"]
    edit_device = device_path(scene, ctx, source, per, warmup, repeats)
    adopted_on_device = scene.wide4_collapse_counts()["device_collapses"] - before
    scene.use_device_builder(None)
    os.environ.pop("HIPR_DEVICE_COLLAPSE", None)
    os.environ.pop("HIPR_DEVICE_COLLAPSE4", None)
    ctx.close()
    med = statistics.median
    return dict(triangles=d.triangle_count, nodes=len(nodes), result=result, same=same, device_ms=med(device), device_low=min(device), device_high=max(device),
                host_ms=med(host), host_low=min(host), host_high=max(host),
                validate=med(s["validate"] for s in split), upload=med(s["upload"] for s in split), kernels=med(s["kernels"] for s in split), readback=med(s["readback"] for s in split),
                two=two, three=three, counts=counts, counts4=counts4, edit_host=edit_host, edit_device=edit_device, adopted_on_device=adopted_on_device, per=per)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scenes", nargs="+", default=list(SCENES), choices=list(SCENES))
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=10)
    p.add_argument("--out", default=str(ROOT / "profiles" / "wide4_collapse_vs_host.txt"))
    args = p.parse_args()
    lines = ["Output of tools/wide4_collapse_probe.py; anything after the line 'Reading' at the end is commentary written by hand.", "",
             "The 4-wide collapse of the procedural atrium's BVH2: the host's WideCollapse against hipr_build_wide4, which collapses to the same nodes on the device (tools/wide4_collapse_probe.py).",
             f"Wall time around the calls, stream synchronised inside; median of {args.repeats} repeats after {args.warmup} warm-up repeats, [min .. max]. The host's collapse is timed in the same run, on {HOST_THREADS} threads.",
             "The device split is the library's own (hipr_debug_collapse4_times) and adds up to the call.", ""]
    faster_everywhere = True
    for name in args.scenes:
        r = measure(*SCENES[name], args.warmup, args.repeats)
        two, three, w = r["two"], r["three"], r["result"]
        faster = three["total"] < two["low"]      # beyond the spread of the repeats: the median with three stages below the fastest repeat with two
        faster_everywhere = faster_everywhere and faster
        block = [f"{name}: {r['triangles']} triangles, {r['nodes']} BVH2 nodes -> {w['node_count']} wide nodes, {w['stack_entries']} stack entries;"
                 f" the device's nodes {'equal' if r['same'] else 'DIFFER FROM'} the host's",
                 f"  (a) 4-wide collapse   host   {r['host_ms']:10.3f} ms  [{r['host_low']:.3f} .. {r['host_high']:.3f}]  (hiprh_wide4_collapse, {HOST_THREADS} threads)",
                 f"                        device {r['device_ms']:10.3f} ms  [{r['device_low']:.3f} .. {r['device_high']:.3f}]  = index walk and checks {r['validate']:.3f} + allocation and upload {r['upload']:.3f} + kernels {r['kernels']:.3f} + read-back {r['readback']:.3f} ms"
                 f" (transfers {100 * (r['upload'] + r['readback']) / max(r['validate'] + r['upload'] + r['kernels'] + r['readback'], 1e-9):.0f} %)",
                 f"                        host / device = {r['host_ms'] / r['device_ms']:.2f}" + ("" if r["device_ms"] < r["host_ms"] else "   -- the device stage is NOT faster than the host stage here"),
                 "  (b) rebuild() + hipr_upload_scene"]
        for label, v in (("two device stages  ", two), ("three device stages", three)):
            block += [f"        {label} {v['total']:10.3f} ms  [{v['low']:.3f} .. {v['high']:.3f}]  = rebuild {v['rebuild']:.3f} + upload {v['upload']:.3f} ms;"
                      f" flatten {v['flatten']:.3f}, BVH2 {v['bvh2']:.3f}{' (device)' if v['source'] == 'used' else ''}, 4-wide collapse {v['wide4']:.3f}, 8-wide collapse {v['wide8']:.3f} ms"]
        block += [f"        two / three = {two['total'] / three['total']:.2f}" + ("" if faster else "   -- three stages are NOT faster than two here beyond the spread of the repeats") +
                  f"; BVH2 builds through the device {r['counts']['device_builds']} (declined {r['counts']['declined_builds']}), 8-wide collapses {r['counts']['device_collapses']} (declined {r['counts']['declined_collapses']}),"
                  f" 4-wide collapses {r['counts4']['device_collapses']} (declined {r['counts4']['declined_collapses']})",
                  "  (c) the instance-edit tick: staging + hipr_edit_scene_instances + adopt_edited_trees"]
        for label, v in (("adoption collapses on the host  ", r["edit_host"]), ("adoption collapses on the device", r["edit_device"])):
            block += [f"        {label} {v['total']:10.3f} ms  [{v['low']:.3f} .. {v['high']:.3f}]  = staging {v['staging']:.3f} + device edit {v['edit']:.3f} + adoption {v['adoption']:.3f} ms;"
                      f" the resident arrays {'equal' if v['same'] else 'DIFFER FROM'} the host's"]
        block += [f"        host / device = {r['edit_host']['total'] / r['edit_device']['total']:.2f}, adoption {r['edit_host']['adoption'] / r['edit_device']['adoption']:.2f};"
                  f" {r['adopted_on_device']} of {r['per']} adoptions collapsed on the device", ""]
        lines += block
        print("\n".join(block), flush=True)
    lines += ["rebuild() + hipr_upload_scene with three device stages is faster than with two, beyond the spread of the repeats, at every size measured here: the 4-wide source may follow the BVH2 source by default." if faster_everywhere else
              "rebuild() + hipr_upload_scene with three device stages is not faster than with two, beyond the spread of the repeats, at every size measured here: the 4-wide source stays opt-in (HIPR_DEVICE_COLLAPSE4=1).", ""]
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
