#!/usr/bin/env python3
"""The BVH2 of a scene, two ways: the host's binned-SAH builder (host/BvhBuilder.cpp) against the device build that produces the same tree byte for byte
(hipr_build_bvh2, csrc/bvh2_build.h).

Two measurements per scene, both wall time around the calls with the stream synchronised inside, the median of `--repeats` repeats after `--warmup` untimed ones:

  (a) the BVH2 stage: hipr_build_bvh2 in total, with its upload / kernels / read-back split (hipr_get_build_times), against the BVH2 stage of build_bvh as
      HIPR_BVH_TIMING=1 prints it;
  (b) the whole rebuild: SceneBuilder::rebuild() + hipr_upload_scene with and without the device as the BVH2 source, with the stage split of the host rebuild
      (flatten, BVH2, 4-wide collapse, 8-wide collapse) as HIPR_BVH_TIMING=1 prints it.

    python tools/device_build_probe.py --scenes atrium251k atrium10M --out profiles/device_build_vs_host.txt
"""
import argparse
import os
import re
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from bifrost3d_amd import capi      # noqa: E402
from bifrost3d_amd.host import Scene      # noqa: E402
from bifrost3d_amd.renderer import Context      # noqa: E402

SCENES = {"atrium251k": (260000, 1), "atrium10M": (10000000, 2)}      # name: (param0 = target triangle count, param1 = seed) of the procedural atrium
STAGES = re.compile(r"build_bvh: (\d+) triangles, (\d+) threads: BVH2 ([\d.]+) s, 4-wide collapse ([\d.]+) s, 8-wide collapse ([\d.]+) s")
FLATTEN = re.compile(r"finalize: \d+ triangles: flatten ([\d.]+) s, build_bvh ([\d.]+) s \(BVH2 source: (\w+), ([\d.]+) s\)")


class captured_stderr:
    """What the libraries print on file descriptor 2 while the block runs."""

    def __enter__(self):
        sys.stderr.flush()
        self.file = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.file.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.file.seek(0)
        self.text = self.file.read().decode(errors="replace")
        self.file.close()


def rebuild_and_upload(scene, ctx, warmup, repeats):
    """Median wall time of rebuild() + upload, and the stages the last repeat printed, in ms."""
    walls, stages, source = [], [], "none"
    for k in range(warmup + repeats):
        with captured_stderr() as err:
            t0 = time.perf_counter()
            scene.rebuild()
            t1 = time.perf_counter()
            ctx.upload_scene(scene)
            ctx.synchronize()
            t2 = time.perf_counter()
        if k >= warmup:
            walls.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
        m, f = STAGES.search(err.text), FLATTEN.search(err.text)
        if m and f and k >= warmup:
            stages.append(dict(threads=int(m.group(2)), bvh2=float(m.group(3)) * 1e3, wide4=float(m.group(4)) * 1e3, wide8=float(m.group(5)) * 1e3, flatten=float(f.group(1)) * 1e3,
                               source_ms=float(f.group(4)) * 1e3))
            source = f.group(3)
    med = statistics.median
    assert len(stages) == repeats, "HIPR_BVH_TIMING printed no stage line"
    return dict(total=med(w[0] for w in walls), rebuild=med(w[1] for w in walls), upload=med(w[2] for w in walls), low=min(w[0] for w in walls), high=max(w[0] for w in walls),
                source=source, **{key: med(st[key] for st in stages) for key in stages[0]})      # the stages: medians over the same repeats, of figures printed to the millisecond


def measure_stage_only(triangles, seed, warmup, repeats, library):
    """(a)'s device leg with another build of the library (the cut between the regimes: see --library)."""
    world = Scene("atrium", param0=triangles, param1=seed).triangles()
    ctx = Context(0, library=library)
    walls, kernels = [], []
    for k in range(warmup + repeats):
        t0 = time.perf_counter()
        status, nodes, order, deepest = ctx.build_bvh2(world)
        ctx.synchronize()
        t1 = time.perf_counter()
        assert status == capi.HIPR_OK, ctx.lib.hipr_last_error()
        if k >= warmup:
            walls.append((t1 - t0) * 1e3)
            kernels.append(ctx.build_times()["kernels"])
    ctx.close()
    return dict(triangles=len(world), nodes=len(nodes), wall=statistics.median(walls), kernels=statistics.median(kernels))


def measure(triangles, seed, warmup, repeats):
    os.environ["HIPR_BVH_TIMING"] = "1"
    with captured_stderr():
        scene = Scene("atrium", param0=triangles, param1=seed)
    ctx = Context(0)
    world = scene.triangles()      # the scene's triangles (in the leaf order of its own tree) as the stand-alone input of (a)
    device, split = [], []
    for k in range(warmup + repeats):
        with captured_stderr():
            t0 = time.perf_counter()
            status, nodes, order, deepest = ctx.build_bvh2(world)
            ctx.synchronize()
            t1 = time.perf_counter()
        assert status == capi.HIPR_OK, ctx.lib.hipr_last_error()
        if k >= warmup:
            device.append((t1 - t0) * 1e3)
            split.append(ctx.build_times())
    host = rebuild_and_upload(scene, ctx, warmup, repeats)
    used = scene.use_device_builder(ctx)
    with_device = rebuild_and_upload(scene, ctx, warmup, repeats)
    counts = scene.build_counts()
    ctx.close()
    med = statistics.median
    return dict(triangles=len(world), nodes=len(nodes), deepest=deepest, device_ms=med(device), device_low=min(device), device_high=max(device),
                validate=med(s["validate"] for s in split), upload=med(s["upload"] for s in split), kernels=med(s["kernels"] for s in split), readback=med(s["readback"] for s in split), host=host, with_device=with_device,
                used=used, counts=counts)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scenes", nargs="+", default=list(SCENES), choices=list(SCENES))
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=10)
    p.add_argument("--out", default=str(ROOT / "profiles" / "device_build_vs_host.txt"))
    p.add_argument("--library", nargs="+", default=[], metavar="LABEL=PATH",
                   help="other builds of libhiprenderer.so whose hipr_build_bvh2 is timed as in (a) and appended, e.g. the cut between the two regimes: "
                        "make -C bifrost3d_amd csrc/scene.o HIPFLAGS='<the Makefile's HIPFLAGS> -DHIPR_BUILD_SHORT_RANGE=32', link it as the Makefile links the product, "
                        "and pass --library 32=<that library>")
    args = p.parse_args()
    lines = ["Output of tools/device_build_probe.py; anything after the line 'Reading' at the end is commentary written by hand.", "",
             "The BVH2 of the procedural atrium: the host's binned-SAH builder against hipr_build_bvh2, which builds the same tree on the device (tools/device_build_probe.py).",
             f"Wall time around the calls, stream synchronised inside; median of {args.repeats} repeats after {args.warmup} warm-up repeats, [min .. max]. Host stages as HIPR_BVH_TIMING=1 prints them.",
             "The device split is the library's own (hipr_debug_build_times) and adds up to the call; what the wall time of (a) holds beyond it is this tool's allocation of the output arrays.", ""]
    for name in args.scenes:
        r = measure(*SCENES[name], args.warmup, args.repeats)
        h, d = r["host"], r["with_device"]
        lines += [f"{name}: {r['triangles']} triangles, {r['nodes']} BVH2 nodes, deepest leaf {r['deepest']}",
                  f"  (a) BVH2 stage   host   {h['bvh2']:10.3f} ms  ({int(h['threads'])} threads; the median of the same repeats of a figure printed in whole milliseconds, and so are the stages below)",
                  f"                   device {r['device_ms']:10.3f} ms  [{r['device_low']:.3f} .. {r['device_high']:.3f}]  = argument checks {r['validate']:.3f} + allocation and upload {r['upload']:.3f} + kernels {r['kernels']:.3f} + read-back {r['readback']:.3f} ms"
                  f" (transfers {100 * (r['upload'] + r['readback']) / max(r['validate'] + r['upload'] + r['kernels'] + r['readback'], 1e-9):.0f} %)",
                  f"                   host / device = {h['bvh2'] / r['device_ms']:.2f}" + ("" if r["device_ms"] < h["bvh2"] else "   -- the device stage is NOT faster than the host stage here"),
                  f"  (b) rebuild() + hipr_upload_scene   host BVH2   {h['total']:10.3f} ms  [{h['low']:.3f} .. {h['high']:.3f}]  = rebuild {h['rebuild']:.3f} + upload {h['upload']:.3f} ms",
                  f"        host rebuild stages: flatten {h['flatten']:.3f}, BVH2 {h['bvh2']:.3f}, 4-wide collapse {h['wide4']:.3f}, 8-wide collapse {h['wide8']:.3f} ms",
                  f"                                      device BVH2 {d['total']:10.3f} ms  [{d['low']:.3f} .. {d['high']:.3f}]  = rebuild {d['rebuild']:.3f} + upload {d['upload']:.3f} ms",
                  f"        stages with the device source ({d.get('source', '?')}): flatten {d['flatten']:.3f}, BVH2 source {d['source_ms']:.3f}, 4-wide collapse {d['wide4']:.3f}, 8-wide collapse {d['wide8']:.3f} ms",
                  f"        host / device = {h['total'] / d['total']:.2f}; builds through the device {r['counts']['device_builds']}, declined {r['counts']['declined_builds']}", ""]
        print("\n".join(lines[-10:]), flush=True)
        for entry in args.library:
            label, path = entry.split("=", 1)
            v = measure_stage_only(*SCENES[name], args.warmup, args.repeats, path)
            lines += [f"  (a) with the library '{label}': hipr_build_bvh2 {v['wall']:10.3f} ms, kernels {v['kernels']:.3f} ms ({v['nodes']} nodes)"]
            print(lines[-1], flush=True)
        if args.library:
            lines += [""]
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
