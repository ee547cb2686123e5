"""A plain statement of what a texture lookup IS, in numpy and float64: the yardstick of tests/test_texture_lookups_cpu.py and tests/test_gpu_texture_lookups.py.

It calls neither the oracle nor the libraries, and it shares no text with them: the definitions are the header comments of csrc/kernels.h and the reference renderer lines
they cite (OptiXRenderer/Renderer.cpp:703-751, Types.h:389-414, Utils.h:288-292, PresampledEnvironmentLightImpl.h:18-41).

  * nearest: the texel (floor(u W), floor(v H));
  * bilinear (bit 0 of `filter`, and only that bit): taps at texel centres -- xb = u W - 0.5, x0 = floor(xb), fx = xb - x0 --, the neighbours x0 and x0 + 1 addressed each on
    its own, blended in x, then in y;
  * addressing per axis: repeat is the mathematical (floor) modulo on integers, clamp goes to [0, N - 1];
  * formats: R8 -> (r / 255, 0, 0, 1), RGBA8 -> every channel / 255, R32F -> (r, 0, 0, 1), RGBA32F as it is;
  * sRGB: decoded per texel BEFORE filtering: r, and g and b of the four-channel formats; never alpha.

DOMAIN: |uv| <= 8 and sizes <= 64. Non-finite and huge coordinates are out of scope here (their conversion to an integer is not defined by this text).

Tolerances:
  * a NEAREST sample is left out where its float64 uv * size lies within 2^-12 texel of a texel edge (excluded()): for |uv| <= 8 and size <= 64 the five f32 roundings of
    the interpolation of the corner coordinates and of the product stay below 2^-13 texel; at most 1 % of a case may be left out (uniform inputs: ~0.1 %);
  * a FILTERED value gets 2^-11 (max - min texel of the texture), absolute: the same 2^-13 texel on each of two axes, with a factor 2 of margin;
  * an sRGB texel of an exact path gets 4 ulp (f32) of the float64 formula rounded once, the fast unit's 1e-5 relative."""
import numpy as np

TEXEL_R8, TEXEL_RGBA8, TEXEL_R32F, TEXEL_RGBA32F = 1, 4, 17, 20
TEXEL_BYTES = {TEXEL_R8: 1, TEXEL_RGBA8: 4, TEXEL_R32F: 4, TEXEL_RGBA32F: 16}
MATERIAL_CUTOUT = 2
EDGE_MARGIN = 2.0 ** -12      # texels
FILTER_TOLERANCE = 2.0 ** -11      # of the texture's value range


def srgb_to_linear(c):
    c = np.asarray(c, np.float64)
    return np.where(c <= 0.04045, c / 12.92, np.power((np.maximum(c, 0.04045) + 0.055) / 1.055, 2.4))


def decoded_texels(texture, texel_bytes) -> np.ndarray:
    """The texture's texels as (height, width, 4) float64 RGBA, sRGB decoded. `texture`: anything with width, height, texel_offset, format, is_sRGB; `texel_bytes`: the
    texel pool as uint8."""
    w, h, fmt = int(texture.width), int(texture.height), int(texture.format)
    raw = np.asarray(texel_bytes, np.uint8)[int(texture.texel_offset): int(texture.texel_offset) + w * h * TEXEL_BYTES[fmt]]
    out = np.zeros((h, w, 4), np.float64)
    out[..., 3] = 1.0
    if fmt == TEXEL_R8:
        out[..., 0] = raw.reshape(h, w).astype(np.float64) / 255.0
    elif fmt == TEXEL_RGBA8:
        out[...] = raw.reshape(h, w, 4).astype(np.float64) / 255.0
    elif fmt == TEXEL_R32F:
        out[..., 0] = raw.view(np.float32).reshape(h, w).astype(np.float64)
    elif fmt == TEXEL_RGBA32F:
        out[...] = raw.view(np.float32).reshape(h, w, 4).astype(np.float64)
    else:
        raise ValueError(f"texel format {fmt}")
    if texture.is_sRGB:
        decoded = 3 if fmt in (TEXEL_RGBA8, TEXEL_RGBA32F) else 1
        out[..., :decoded] = srgb_to_linear(out[..., :decoded])
    return out


def value_range(texture, texel_bytes) -> float:
    """max - min over the texture's decoded texels (every channel the format stores)."""
    t = decoded_texels(texture, texel_bytes)
    stored = t if int(texture.format) in (TEXEL_RGBA8, TEXEL_RGBA32F) else t[..., :1]
    return float(stored.max() - stored.min())


def address(i, n: int, repeat: bool):
    i = np.asarray(i, np.int64)
    return np.mod(i, n) if repeat else np.clip(i, 0, n - 1)      # numpy's integer mod is the floor modulo, as Python's % on ints


def is_bilinear(texture) -> bool:
    return (int(texture.filter) & 1) != 0


def sample(texture, texel_bytes, uv) -> np.ndarray:
    """RGBA (n, 4) float64 of the texture at uv (n, 2)."""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    texels = decoded_texels(texture, texel_bytes)
    w, h = int(texture.width), int(texture.height)
    repeat_u, repeat_v = bool(texture.wrap_u), bool(texture.wrap_v)
    if not is_bilinear(texture):
        x = address(np.floor(uv[:, 0] * w).astype(np.int64), w, repeat_u)
        y = address(np.floor(uv[:, 1] * h).astype(np.int64), h, repeat_v)
        return texels[y, x]
    xb, yb = uv[:, 0] * w - 0.5, uv[:, 1] * h - 0.5
    x0, y0 = np.floor(xb).astype(np.int64), np.floor(yb).astype(np.int64)
    fx, fy = (xb - x0)[:, None], (yb - y0)[:, None]
    xa, xc = address(x0, w, repeat_u), address(x0 + 1, w, repeat_u)
    ya, yc = address(y0, h, repeat_v), address(y0 + 1, h, repeat_v)
    low = texels[ya, xa] * (1.0 - fx) + texels[ya, xc] * fx
    high = texels[yc, xa] * (1.0 - fx) + texels[yc, xc] * fx
    return low * (1.0 - fy) + high * fy


def excluded(texture, uv) -> np.ndarray:
    """The samples of a NEAREST lookup that lie within EDGE_MARGIN of a texel edge (nothing of a bilinear one: its value is continuous across the edge)."""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    if is_bilinear(texture):
        return np.zeros(len(uv), bool)
    near = np.zeros(len(uv), bool)
    for axis, n in ((0, int(texture.width)), (1, int(texture.height))):
        p = uv[:, axis] * n
        near |= np.abs(p - np.round(p)) < EDGE_MARGIN
    return near


def coverage(material, texture, texel_bytes, uv) -> np.ndarray:
    """get_coverage (OptiXRenderer/Types.h:405-414): a cut-out gives 0 or 1 from the threshold comparison, anything else coverage * tex.x. `texture`: None when the material
    names no coverage texture."""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    tex = sample(texture, texel_bytes, uv)[:, 0] if texture is not None else np.ones(len(uv))
    if int(material.flags) & MATERIAL_CUTOUT:
        return np.where(tex < float(material.coverage), 0.0, 1.0)
    return float(material.coverage) * tex


def transmittance(cover) -> np.ndarray:
    """What one hit leaves of a shadow ray (shadow_any_hit, MonteCarlo.cu:278-285): 1 - coverage, the ray ended below 1e-7."""
    t = 1.0 - np.asarray(cover, np.float64)
    return np.where(t < 1e-7, 0.0, t)


# ---- the latitude-longitude environment (Utils.h:288-292, PresampledEnvironmentLightImpl.h:18-41) ----
def latlong_texcoord(directions) -> np.ndarray:
    d = np.asarray(directions, np.float64).reshape(-1, 3)
    u = (np.arctan2(d[:, 2], d[:, 0]) + np.pi) / (2.0 * np.pi)
    v = (np.arcsin(np.clip(d[:, 1], -1.0, 1.0)) + np.pi / 2.0) / np.pi
    return np.stack([u, v], axis=1)


def environment_evaluate(tint, texture, texel_bytes, directions) -> np.ndarray:
    return np.asarray(tint, np.float64)[None, :] * sample(texture, texel_bytes, latlong_texcoord(directions))[:, :3]


def environment_pdf(per_pixel_PDF, width: int, height: int, directions, displaced_texels=(0.0, 0.0)) -> np.ndarray:
    """per_pixel_PDF[clamped nearest] / sqrt(1 - y^2); at sin(theta) = 0 the delta PDF -0, which is not used for MIS. `displaced_texels`: the lookup moved by that
    much of a texel, for the directions environment_pdf_excluded() names: there either neighbour is a right answer."""
    d = np.asarray(directions, np.float64).reshape(-1, 3)
    uv = latlong_texcoord(d) + np.array([displaced_texels[0] / width, displaced_texels[1] / height])
    x = np.clip(np.floor(uv[:, 0] * width).astype(np.int64), 0, width - 1)
    y = np.clip(np.floor(uv[:, 1] * height).astype(np.int64), 0, height - 1)
    sin_theta = np.sqrt(np.maximum(1.0 - d[:, 1] * d[:, 1], 0.0))
    table = np.asarray(per_pixel_PDF, np.float64).reshape(height, width)
    with np.errstate(divide="ignore", invalid="ignore"):
        pdf = table[y, x] / sin_theta
    return np.where(sin_theta == 0.0, -0.0, pdf)


def environment_pdf_excluded(width: int, height: int, directions) -> np.ndarray:
    """Directions whose PDF texel is decided within EDGE_MARGIN of a texel edge of the PDF image (the clamped outer edges decide nothing)."""
    uv = latlong_texcoord(directions)
    near = np.zeros(len(uv), bool)
    for axis, n in ((0, width), (1, height)):
        p = uv[:, axis] * n
        edge = np.round(p)
        near |= (np.abs(p - edge) < EDGE_MARGIN) & (edge > 0) & (edge < n)
    return near


def balance_heuristic(p, q):
    return p / (p + q)
