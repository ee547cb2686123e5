#!/usr/bin/env python3
"""Pixels of a resident image edited, two ways: the path every pixel edit used to take -- a new scene: SceneBuilder::rebuild (the triangles flattened again, the
BVH2, the 4-wide and the 8-wide tree built) + hipr_upload_scene of every pool -- against the device path (hipr_update_scene_texels: the rectangle's rows copied into
the resident texel pool and, where the texture decides triangle flags, the coverage pass of csrc/texel_update.h).

Three edits of the textured procedural atrium: a 64 x 64 rectangle of a tint texture, a 16 x 16 hole punched into the lace coverage texture (and filled again by the
next repeat, so that every repeat changes flags), and the whole lace texture replaced (by one with the holes elsewhere, and back). Both legs are timed around the
calls, with a stream synchronise inside the timed span, as the median of `--repeats` repeats after `--warmup` untimed ones. The result of the two paths is the same
bytes (tests/test_gpu_texel_update.py). The host leg leaves out what HIPRenderer::Renderer's full path does on top -- flattening the Bifrost managers into a new
SceneBuilder -- so it flatters the host.

The device call's own figures (hipr_debug_texel_update_times) are printed with it: the rows packed and their staging copy queued, the rectangle writes, the coverage
pass -- one thread per triangle, the triangles of the materials the texture decides flags for scan their boxes of texels again -- and the leaf pass. (A two-pass form
of the coverage pass, a wave per triangle whose box meets a rectangle, was measured against it with an earlier state of this probe and removed:
profiles/texel_update_wave_per_candidate_rejected.txt.)

    python tools/texel_update_probe.py --scenes atrium251k atrium10M --out profiles/texel_update_device_vs_host.txt
"""
import argparse
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
EDITS = ("tint_64x64", "lace_hole_16x16", "lace_whole")


def texels_of(scene, index):
    """The texture's image as the pool holds it: (height, width[, channels]) of uint8 or float32."""
    d = scene.desc
    t = d.textures[index]
    channels, dtype = {capi.TEXEL_R8: (1, np.uint8), capi.TEXEL_RGBA8: (4, np.uint8), capi.TEXEL_R32F: (1, np.float32), capi.TEXEL_RGBA32F: (4, np.float32)}[t.format]
    count = t.width * t.height * channels * np.dtype(dtype).itemsize
    flat = np.ctypeslib.as_array(d.texels, shape=(d.texel_bytes,))[t.texel_offset:t.texel_offset + count].copy().view(dtype)
    return flat.reshape((t.height, t.width) if channels == 1 else (t.height, t.width, channels))


def plan(scene):
    """The lace texture and the materials it decides flags for, a tint texture of at least 64 x 64, and per edit the two rectangles the repeats alternate between."""
    materials = scene.materials()
    lace = next(m.coverage_texture_ID for m in materials if m.coverage_texture_ID > 0)
    lace_materials = [k for k, m in enumerate(materials) if m.coverage_texture_ID == lace]
    d = scene.desc
    tint = next(m.tint_roughness_texture_ID for m in materials if m.tint_roughness_texture_ID > 0 and d.textures[m.tint_roughness_texture_ID].width >= 64 and d.textures[m.tint_roughness_texture_ID].height >= 64)
    tint_image, lace_image = texels_of(scene, tint), texels_of(scene, lace)
    triangles, instances = scene.triangles(), scene.instances_array()
    worn = int(np.isin(instances[triangles[:, 9], 15], lace_materials).sum())
    return dict(lace=lace, tint=tint, lace_materials=lace_materials, lace_triangles=worn, lace_size=lace_image.shape[:2], alternatives={
        "tint_64x64": (tint, 0, 0, [np.ascontiguousarray(255 - tint_image[:64, :64]), np.ascontiguousarray(tint_image[:64, :64])]),
        "lace_hole_16x16": (lace, 24, 24, [np.zeros_like(lace_image[24:40, 24:40]), np.ascontiguousarray(lace_image[24:40, 24:40])]),
        "lace_whole": (lace, 0, 0, [np.ascontiguousarray(np.roll(lace_image, 3, axis=(0, 1))), lace_image]),
    })


def measure(triangles, seed, warmup, repeats, device_only=False):
    scene = Scene("atrium", param0=triangles, param1=seed, textured=True)
    ctx = Context(0)
    t0 = time.perf_counter()
    ctx.upload_scene(scene)
    ctx.synchronize()
    upload_ms = (time.perf_counter() - t0) * 1e3
    desc = scene.desc
    p = plan(scene)
    med = statistics.median
    out = dict(triangles=desc.triangle_count, slots=desc.wide8_slot_count, upload_ms=upload_ms, lace_triangles=p["lace_triangles"], lace_size=p["lace_size"], edits={})
    for name in EDITS:
        texture, x, y, pixels = p["alternatives"][name]
        host, device, passes, answers = [], [], [], []
        for k in range(0 if device_only else warmup + repeats):
            assert scene.update_texels([(texture, x, y, pixels[k % 2])])      # the edit itself is in the builder either way; the parent's path then builds and uploads a new scene
            t0 = time.perf_counter()
            scene.rebuild()
            t1 = time.perf_counter()
            ctx.upload_scene(scene)
            ctx.synchronize()
            t2 = time.perf_counter()
            if k >= warmup:
                host.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
        for k in range(warmup + repeats):
            edit = [(texture, x, y, pixels[k % 2])]
            t0 = time.perf_counter()
            assert scene.update_texels(edit)
            t1 = time.perf_counter()
            answer = ctx.update_scene_texels(edit)
            ctx.synchronize()
            t2 = time.perf_counter()
            assert answer["status"] == capi.HIPR_OK
            if k >= warmup:
                device.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
                passes.append(ctx.texel_update_times())
                answers.append((answer["candidate_triangles"], answer["changed_triangles"]))
        host = host or [(float("nan"),) * 3]
        out["edits"][name] = dict(
            host_ms=med(h[0] for h in host), host_build_ms=med(h[1] for h in host), host_upload_ms=med(h[2] for h in host), host_min=min(h[0] for h in host), host_max=max(h[0] for h in host),
            device_ms=med(d[0] for d in device), device_builder_ms=med(d[1] for d in device), device_call_ms=med(d[2] for d in device), device_min=min(d[0] for d in device),
            device_max=max(d[0] for d in device), passes={key: med(t[key] for t in passes) for key in passes[0]}, candidates=sorted(set(answers)),
            rectangle=f"{pixels[0].shape[1]} x {pixels[0].shape[0]} texels of texture {texture}")
        print(f"  ... {name} measured", file=sys.stderr, flush=True)
    ctx.close()
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scenes", nargs="+", default=list(SCENES), choices=list(SCENES))
    p.add_argument("--device-only", action="store_true", help="skip the host leg")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=10)
    p.add_argument("--out", default=str(ROOT / "profiles" / "texel_update_device_vs_host.txt"))
    args = p.parse_args()
    lines = ["Pixels of a resident image of the textured procedural atrium edited: SceneBuilder::rebuild + hipr_upload_scene (the path every pixel edit took) against",
             "SceneBuilder::update_texels + hipr_update_scene_texels (tools/texel_update_probe.py).",
             f"Wall time around the calls, stream synchronised inside; median of {args.repeats} repeats after {args.warmup} warm-up repeats, [min .. max].",
             "passes: hipr_debug_texel_update_times, medians -- the rows packed and their staging copy queued (host clock), the rectangle writes, the coverage pass, the leaf pass.", ""]
    for name in args.scenes:
        r = measure(*SCENES[name], args.warmup, args.repeats, args.device_only)
        lines += [f"{name}: {r['triangles']} triangles, {r['slots']} slots of the 8-wide tree; the lace texture is {r['lace_size'][1]} x {r['lace_size'][0]} and decides the flags of "
                  f"{r['lace_triangles']} triangles (first scene upload: {r['upload_ms']:.1f} ms)"]
        for edit in EDITS:
            e = r["edits"][edit]
            lines += [f"  {edit}: {e['rectangle']}; (triangles decided again, changed) per repeat: {e['candidates']}",
                      f"    host path    {e['host_ms']:10.3f} ms  [{e['host_min']:.3f} .. {e['host_max']:.3f}]   = rebuild {e['host_build_ms']:.3f} ms + hipr_upload_scene {e['host_upload_ms']:.3f} ms",
                      f"    device path  {e['device_ms']:10.3f} ms  [{e['device_min']:.3f} .. {e['device_max']:.3f}]   = Scene.update_texels {e['device_builder_ms']:.3f} ms + hipr_update_scene_texels {e['device_call_ms']:.3f} ms",
                      f"    passes       staging {e['passes']['staging']:.3f} ms, writes {e['passes']['writes']:.3f} ms, coverage {e['passes']['coverage']:.3f} ms, leaves {e['passes']['leaves']:.3f} ms",
                      f"    host / device = {e['host_ms'] / e['device_ms']:.1f}"]
        lines.append("")
        print("\n".join(lines[-(2 + 5 * len(EDITS)):]), flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")      # after every scene: a later one that runs out of time leaves the earlier figures


if __name__ == "__main__":
    main()
