#!/usr/bin/env python3
"""A lamp added and the sky set, two ways each: the resident scene edited on the device (hipr_update_scene_lighting with SceneBuilder::staged_environment_build and
adopt_lighting; csrc/environment_build.h) against the only path the same edit had before -- SceneBuilder::add_light, or InfiniteAreaLight + presample_environment +
add_texture + set_environment, then rebuild() + hipr_upload_scene. The library splits its call into allocation + uploads, kernels, the host's finish of the samples and
read-back (hipr_debug_lighting_times).

The sky is procedural, `--sky` texels of RGBA32F with a bilinear sampler: a gradient, a dark ground and a sun disc. On the device path its texture is resident before
the timed repeats (bringing a new texture is hipr_append_scene_pools' business, tools/pool_growth_probe.py), and every repeat builds the environment of that texture
again; on the host path every repeat adds the image again, as the scene builder's only call does, so its texel pool grows by one sky per repeat.

Wall time around the calls with the stream synchronised inside, the median of `--repeats` repeats after `--warmup` untimed ones.

    python tools/lighting_update_probe.py --scenes atrium251k atrium10M --out profiles/lighting_update_device_vs_host.txt
"""
import argparse
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


def sky(width, height) -> np.ndarray:
    v = (np.arange(height, dtype=np.float32) + 0.5) / height
    u = (np.arange(width, dtype=np.float32) + 0.5) / width
    up = -np.cos(v * np.float32(np.pi))[:, None] * np.ones((1, width), np.float32)
    pixels = np.zeros((height, width, 4), np.float32)
    pixels[..., 0] = np.where(up > 0, 0.35 + 0.25 * (1 - up), 0.08)
    pixels[..., 1] = np.where(up > 0, 0.55 + 0.2 * (1 - up), 0.07)
    pixels[..., 2] = np.where(up > 0, 0.9, 0.06)
    sun = np.exp(-(((u[None, :] - 0.3) * 2 * width / height) ** 2 + (v[:, None] - 0.7) ** 2) * 900.0).astype(np.float32)
    pixels[..., :3] += 60.0 * sun[..., None]
    pixels[..., 3] = 1.0
    return pixels


def lamp(k) -> capi.HiprLight:
    light = capi.HiprLight()
    light.data[0:7] = [30.0, 25.0, 20.0, 0.5 + 0.01 * k, 1.5, -0.5, 0.05]
    light.flags = 1      # HIPR_LIGHT_SPHERE
    return light


def own_lights(scene) -> list:
    return [light for light in scene.lights() if (light.flags & 7) != 4]


def summary(rows) -> dict:
    out = {key: statistics.median(r[key] for r in rows) for key in rows[0]}
    out.update(low=min(r["total"] for r in rows), high=max(r["total"] for r in rows))
    return out


def timed(repeat, warmup, repeats) -> dict:
    rows = []
    for k in range(warmup + repeats):
        with captured_stderr():
            row = repeat(k)
        if k >= warmup:
            rows.append(row)
    return summary(rows)


def measure(triangles, seed, sky_extent, samples, warmup, repeats) -> dict:
    ms = lambda a, b: (b - a) * 1e3
    pixels = sky(*sky_extent)
    texture = dict(pixels=pixels, width=sky_extent[0], height=sky_extent[1], texel_format=capi.TEXEL_RGBA32F, repeat=(True, False), linear=(True, True))
    ctx = Context(0)
    scene = Scene("atrium", param0=triangles, param1=seed)
    index = scene.add_texture(**texture)
    scene.rebuild()
    ctx.upload_scene(scene)
    base = own_lights(scene)
    stagings = []      # of every repeat of the sky on the device, the warm-up ones included: the first makes the draw points

    def device_light(k):
        t0 = time.perf_counter()
        lights = base + [lamp(j) for j in range(k + 1)]
        updated = ctx.update_scene_lighting(lights, capi.ENVIRONMENT_KEEP)
        ctx.synchronize()
        t1 = time.perf_counter()
        assert updated["status"] == capi.HIPR_OK and scene.adopt_lighting(lights, capi.ENVIRONMENT_KEEP, updated=updated)
        t2 = time.perf_counter()
        return dict(total=ms(t0, t2), call=ms(t0, t1), adoption=ms(t1, t2))

    def device_sky(k):
        t0 = time.perf_counter()
        build = scene.staged_environment_build(index, samples)
        t1 = time.perf_counter()
        lights = own_lights(scene)
        updated = ctx.update_scene_lighting(lights, capi.ENVIRONMENT_BUILD, build)
        ctx.synchronize()
        t2 = time.perf_counter()
        assert updated["status"] == capi.HIPR_OK and not updated["disabled"] and scene.adopt_lighting(lights, capi.ENVIRONMENT_BUILD, index, updated)
        t3 = time.perf_counter()
        stagings.append(ms(t0, t1))
        return dict(total=ms(t0, t3), staging=ms(t0, t1), call=ms(t1, t2), adoption=ms(t2, t3), **ctx.lighting_times())

    def host_light(k):
        t0 = time.perf_counter()
        scene.add_light(lamp(100 + k))
        scene.rebuild()
        t1 = time.perf_counter()
        ctx.upload_scene(scene)
        ctx.synchronize()
        t2 = time.perf_counter()
        return dict(total=ms(t0, t2), rebuild=ms(t0, t1), upload=ms(t1, t2))

    def host_sky(k):
        t0 = time.perf_counter()
        scene.add_environment(sample_count=samples, **texture)
        t1 = time.perf_counter()
        scene.rebuild()
        t2 = time.perf_counter()
        ctx.upload_scene(scene)
        ctx.synchronize()
        t3 = time.perf_counter()
        return dict(total=ms(t0, t3), presample=ms(t0, t1), rebuild=ms(t1, t2), upload=ms(t2, t3))

    out = dict(triangles=scene.desc.triangle_count)
    out["device_light"] = timed(device_light, warmup, repeats)
    out["device_sky"] = timed(device_sky, warmup, repeats)
    out["first_staging"] = stagings[0]
    # the device's environment against the host path's over the same texels: the check of the run
    resident = [ctx.read_scene_buffer(which) for which in (capi.SCENE_BUFFER_ENVIRONMENT_PDF, capi.SCENE_BUFFER_ENVIRONMENT_SAMPLES)]
    out["host_light"] = timed(host_light, warmup, repeats)
    out["host_sky"] = timed(host_sky, warmup, repeats)
    theirs = [ctx.read_scene_buffer(which) for which in (capi.SCENE_BUFFER_ENVIRONMENT_PDF, capi.SCENE_BUFFER_ENVIRONMENT_SAMPLES)]
    out["same"] = all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(resident, theirs))
    ctx.close()
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scenes", nargs="+", default=list(SCENES), choices=list(SCENES))
    p.add_argument("--sky", nargs=2, type=int, default=[2048, 1024], metavar=("WIDTH", "HEIGHT"))
    p.add_argument("--samples", type=int, default=8192, help="presampled light samples (presample_environment's default)")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=10)
    p.add_argument("--out", default=str(ROOT / "profiles" / "lighting_update_device_vs_host.txt"))
    args = p.parse_args()
    lines = ["Output of tools/lighting_update_probe.py; anything after the line 'Reading' at the end is commentary written by hand.", "",
             f"Per repeat a lamp added, and a procedural {args.sky[0]} x {args.sky[1]} RGBA32F sky set with {args.samples} samples: the resident scene edited on the device",
             "(hipr_update_scene_lighting + the builder's adoption) against the host's rebuild + upload, which was the only path for either edit.",
             f"Wall time around the calls, stream synchronised inside; median of {args.repeats} repeats after {args.warmup} warm-up repeats, [min .. max].",
             "The split of the device's call is the library's own (hipr_debug_lighting_times).", ""]
    for name in args.scenes:
        r = measure(*SCENES[name], tuple(args.sky), args.samples, args.warmup, args.repeats)
        dl, ds, hl, hs = r["device_light"], r["device_sky"], r["host_light"], r["host_sky"]
        lines += [f"{name}: {r['triangles']} triangles; the environment's PDF image and samples on the device {'equal' if r['same'] else 'DIFFER FROM'} the host path's over the same texels",
                  f"  a lamp added, device               {dl['total']:10.3f} ms  [{dl['low']:.3f} .. {dl['high']:.3f}]  = hipr_update_scene_lighting {dl['call']:.3f} + adoption {dl['adoption']:.3f} ms",
                  f"  a lamp added, host                 {hl['total']:10.3f} ms  [{hl['low']:.3f} .. {hl['high']:.3f}]  = add_light + rebuild {hl['rebuild']:.3f} + upload {hl['upload']:.3f} ms",
                  f"  the sky set, device                {ds['total']:10.3f} ms  [{ds['low']:.3f} .. {ds['high']:.3f}]  = staging {ds['staging']:.3f} + hipr_update_scene_lighting {ds['call']:.3f} + adoption {ds['adoption']:.3f} ms",
                  f"      hipr_update_scene_lighting     = allocation + uploads {ds['upload']:.3f} + kernels {ds['kernels']:.3f} + the host's finish {ds['finish']:.3f} + read-back {ds['readback']:.3f} ms (the rest: the checks, the light list)",
                  f"      staging of the first repeat    = {r['first_staging']:.3f} ms: the draw points of a sample count are made once and kept by the builder",
                  f"  the sky set, host                  {hs['total']:10.3f} ms  [{hs['low']:.3f} .. {hs['high']:.3f}]  = InfiniteAreaLight + presample_environment + add_texture {hs['presample']:.3f} + rebuild {hs['rebuild']:.3f}"
                  f" + upload {hs['upload']:.3f} ms",
                  f"  host / device: a lamp {hl['total'] / dl['total']:.1f}, the sky {hs['total'] / ds['total']:.1f}; the host's presampling alone / the device's whole tick {hs['presample'] / ds['total']:.1f}", ""]
        print("\n".join(lines[-10:]), flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")      # after every scene: a run cut short keeps what it has


if __name__ == "__main__":
    main()
