"""What the tests of hipr_update_scene_texels share (csrc/texel_update.h, SceneBuilder::update_texels): the scene -- the Cornell box with walls of 4 x 4 quads (184
triangles: the 8-wide tree exists) plus a tessellated quad with a cut-out material whose coverage texture follows an unrelated 16 x 16 texture in the pool -- its
variants, the cases of pixel edits, and ctypes access to the host build of the update's kernel bodies (tests/native/TexelUpdateHost.hip). Test infrastructure: built
by bifrost3d_amd/Makefile, loaded by tests only.

The yardstick of every case is SceneBuilder: update_texels on the built scene, and a scene made anew from the edited images."""
import ctypes as C
from pathlib import Path

import numpy as np

import material_update_bindings as mu
import pool_growth_bindings as pg
from bifrost3d_amd import capi
from bifrost3d_amd.host import Scene

R8, RGBA8, R32F, RGBA32F = capi.TEXEL_R8, capi.TEXEL_RGBA8, capi.TEXEL_R32F, capi.TEXEL_RGBA32F

# The texture coordinates of the quad's corners: the image once; a quarter beyond it on every side, where repeating and clamping matter; and its inner half, the one
# set that leaves texels of a 32 x 32 image outside every triangle's box -- the case "one texel further out changes nothing" needs such texels, and under the other two
# every texel lies in some box.
UNIT, BEYOND, INNER = (0.0, 1.0), (-0.25, 1.25), (0.25, 0.75)

UNRELATED = (np.arange(16 * 16 * 4, dtype=np.uint32) * 37 % 251).astype(np.uint8).reshape(16, 16, 4)      # the 16 x 16 RGBA8 texture before the coverage texture


def variant(fmt=R8, linear=False, repeat=True, srgb=False, cutout=True, coverage=0.5, coords=UNIT, cells=8, size=32, tint=None):
    """fmt, linear, repeat, srgb, size: the coverage texture; cutout, coverage: the quad's material; coords, cells: the quad; tint: the format of a third, float texture
    the material takes as its tint texture (None: none)."""
    return dict(fmt=fmt, linear=linear, repeat=repeat, srgb=srgb, cutout=cutout, coverage=coverage, coords=coords, cells=cells, size=size, tint=tint)


def solid(v, value=255):
    """The coverage image every case starts from: every byte `value`."""
    shape = (v["size"], v["size"]) if v["fmt"] == R8 else (v["size"], v["size"], 4)
    return np.full(shape, value, np.uint8)


def tint_image(v):
    rng = np.random.default_rng(5)
    return rng.uniform(0.2, 1.0, (8, 8) if v["tint"] == R32F else (8, 8, 4)).astype(np.float32)


def tessellated_quad(cells, coords):
    """pool_growth_bindings' quad (corners at +-0.5 in x and y, facing -z) as cells x cells cells of two triangles; texture coordinates `coords` from corner to corner."""
    steps = np.arange(cells + 1, dtype=np.float32) / np.float32(cells)
    lo, hi = np.float32(coords[0]), np.float32(coords[1])
    grid = [(i, j) for j in range(cells + 1) for i in range(cells + 1)]
    positions = np.array([[steps[i] - 0.5, steps[j] - 0.5, 0.0] for i, j in grid], np.float32)
    texcoords = np.array([[lo + (hi - lo) * steps[i], lo + (hi - lo) * steps[j]] for i, j in grid], np.float32)
    at = lambda i, j: j * (cells + 1) + i
    primitives = []
    for j in range(cells):
        for i in range(cells):
            primitives += [[at(i, j), at(i + 1, j + 1), at(i + 1, j)], [at(i, j), at(i, j + 1), at(i + 1, j + 1)]]      # QUAD_PRIMITIVES' winding
    return dict(positions=positions, primitives=np.array(primitives, np.uint32), normals=np.tile(pg.QUAD_NORMALS[0], (len(grid), 1)), texcoords=texcoords)


def make_scene(v, images=None):
    """The scene of variant `v` built on the host. `images`: {"coverage": ..., "tint": ...} in place of the images the variant starts from. Returns (scene, info) with
    info = the texture indices by name, the material, the quad's triangles (indices into scene.triangles()) and the images as given."""
    images = dict(images or {})
    images.setdefault("coverage", solid(v))
    if v["tint"] is not None:
        images.setdefault("tint", tint_image(v))
    scene = Scene("cornell", param0=4)
    textures = {"unrelated": scene.add_texture(UNRELATED, 16, 16, RGBA8, is_sRGB=True, linear=(True, True))}
    textures["coverage"] = scene.add_texture(images["coverage"], v["size"], v["size"], v["fmt"], is_sRGB=v["srgb"], repeat=(v["repeat"], v["repeat"]), linear=(v["linear"], v["linear"]))
    if v["tint"] is not None:
        textures["tint"] = scene.add_texture(images["tint"], 8, 8, v["tint"], linear=(True, True))
    material = scene.add_material(pg.material(flags=capi.MATERIAL_THIN_WALLED | (capi.MATERIAL_CUTOUT if v["cutout"] else 0), coverage=v["coverage"], coverage_texture=textures["coverage"],
                                              tint_texture=textures.get("tint", 0)))
    mesh = scene.add_mesh(**tessellated_quad(v["cells"], v["coords"]))
    assert scene.insert_model(1000, mesh, material, model_index=202, **pg.BESIDE_IT) == 202
    scene.rebuild()
    triangles = scene.triangles()
    quad = np.nonzero(triangles[:, 9] == scene.desc.instance_count - 1)[0]
    assert len(quad) == 2 * v["cells"] ** 2
    return scene, dict(textures=textures, material=material, quad=quad, images=images)


def opaque(scene, info):
    """HIPR_TRIANGLE_OPAQUE of the quad's triangles, in the order of info["quad"]."""
    return (scene.triangles()[info["quad"], 11] & capi.TRIANGLE_OPAQUE) != 0


def patch(v, value, width=1, height=1, channels=None):
    """A rectangle of texels of the coverage texture's format: every byte `value`, or -- RGBA8 -- `channels` = (r, g, b, a)."""
    if v["fmt"] == R8:
        return np.full((height, width), value, np.uint8)
    return np.tile(np.array(channels if channels is not None else [value] * 4, np.uint8), (height, width, 1))


def painted(image, x, y, pixels):
    """`image` with the rectangle of `pixels` at (x, y): what the pool must hold afterwards."""
    out = image.copy()
    out[y:y + pixels.shape[0], x:x + pixels.shape[1]] = pixels
    return out


# ---- the cases: (id, variant, steps); a step = (edits of the coverage texture as (x, y, pixels), what the quad's flags must do) with
#      "some": some but not all of the quad's triangles change; "none": no triangle changes; "back": every triangle is opaque again ----
def _cases():
    nearest, linear = variant(), variant(linear=True, coords=INNER)
    repeat, clamp = variant(coords=BEYOND), variant(coords=BEYOND, repeat=False)
    plain, rgba = variant(cutout=False, coverage=1.0), variant(fmt=RGBA8)
    hole = lambda v, x, y, value=0: (x, y, patch(v, value))
    cases = [
        # 1, 2: a 1 x 1 hole, and the hole filled again
        ("hole_nearest_r8", nearest, [([hole(nearest, 13, 13)], "some"), ([hole(nearest, 13, 13, 255)], "back")]),
        # 3: cell i of the inner half spans texels [8 + 2 i, 10 + 2 i]; bilinear, its box is [6 + 2 i, 11 + 2 i]: column 25 is the last cell's slack column past its
        # bilinear neighbour 24, and column 26 lies in no box
        ("linear_slack_column", linear, [([hole(linear, 26, 16)], "none"), ([hole(linear, 25, 16)], "some")]),
        ("linear_slack_row", linear, [([hole(linear, 16, 5)], "none"), ([hole(linear, 16, 6)], "some")]),
        # 4: the boxes of the second and the seventh column of cells cross the seam
        ("repeat_seam", repeat, [([hole(repeat, 0, 16), hole(repeat, 31, 16)], "some")]),
        # 5: every box that lies outside the image on that side reads the corner texel
        ("clamp_corner", clamp, [([hole(clamp, 0, 0)], "some")]),
        # 6: float(value) / 255.0f > 0.5f + 1e-5f -- 127 fails, 128 and 129 pass
        ("threshold", nearest, [([hole(nearest, 9, 20, 128)], "none"), ([hole(nearest, 9, 20, 129)], "none"), ([hole(nearest, 9, 20, 127)], "some"), ([hole(nearest, 9, 20, 128)], "back")]),
        # 7: plain coverage wants every texel exactly 1
        ("plain_coverage", plain, [([hole(plain, 20, 7, 254)], "some"), ([hole(plain, 20, 7, 255)], "back")]),
        # 8: the sampler's .x alone decides
        ("rgba8_red_decides", rgba, [([(5, 22, patch(rgba, 0, channels=(255, 0, 0, 0)))], "none"), ([(5, 22, patch(rgba, 0, channels=(0, 255, 255, 255)))], "some")]),
        # 9: textures that never change a flag: the edit must still land in the pool
        ("srgb_coverage", variant(srgb=True), [([hole(nearest, 13, 13)], "none")]),
        ("box_over_64_texels", variant(cells=2, size=256), [([(100, 100, np.zeros((3, 3), np.uint8))], "none")]),
    ]
    # 10: rectangle shapes, all on the R8 texture, whose rows begin at any byte
    ramp = lambda w, h, first: ((np.arange(w * h, dtype=np.uint32) * 7 + first) % 120).astype(np.uint8).reshape(h, w)      # every value below the cut-off
    shapes = [
        ("shape_1x1", [(7, 9, ramp(1, 1, 3))]), ("shape_last_row", [(0, 31, ramp(32, 1, 5))]), ("shape_last_column", [(31, 0, ramp(1, 32, 9))]), ("shape_full_image", [(0, 0, ramp(32, 32, 1))]),
        ("shape_odd_x_odd_width", [(3, 5, ramp(7, 5, 11))]), ("shape_overlapping_later_wins", [(4, 4, ramp(10, 10, 2)), (9, 9, np.full((10, 10), 255, np.uint8))]),
    ]
    cases += [(name, nearest, [(edits, "some" if name != "shape_full_image" else "all")]) for name, edits in shapes]
    return cases


CASES = _cases()
CASE_IDS = [c[0] for c in CASES]


def case(name):
    return CASES[CASE_IDS.index(name)]


def check_expectation(what, before, after):
    """`before`, `after`: opaque() around a step."""
    changed = before != after
    if what == "some":
        assert 0 < changed.sum() < len(changed), changed.sum()      # neither none nor all: the case cannot pass vacuously
    elif what == "all":
        assert before.all() and not after.any()
    elif what == "none":
        assert not changed.any()
    else:
        assert what == "back" and changed.any() and after.all()


def coverage_edits(info, edits):
    """A step's edits as Scene.update_texels / Context.update_scene_texels take them."""
    return [(info["textures"]["coverage"], x, y, pixels) for x, y, pixels in edits]


# ---- the host build of the kernel bodies (tests/native/TexelUpdateHost.hip) ----
LIB_PATH = Path(__file__).resolve().parent / "native" / "libtexel_update_host.so"
_lib = None


def library():
    global _lib
    if _lib is None:
        assert LIB_PATH.exists(), f"{LIB_PATH} is missing: run __graft_entry__.build()"
        _lib = C.CDLL(str(LIB_PATH))
        vp = C.c_void_p
        _lib.texel_update_host_scene.argtypes = [vp, C.c_uint32, vp, C.c_uint32, vp, vp, vp, vp, C.c_uint32, vp, C.POINTER(capi.HiprTexelEdit), C.c_uint32, vp, vp, vp, vp, C.c_uint32, vp]
    return _lib


def arrays_of(scene):
    """Copies of what the passes rewrite or must leave alone, as the device holds them after an upload: the triangles, the trace and shading records (a pattern but for
    the words a material shows in) and the class bytes (material_update_bindings.derived_arrays), the slots, the texel pool."""
    trace, shade, classes = mu.derived_arrays(scene)
    d = scene.desc
    return dict(triangles=scene.triangles(), trace=trace, shade=shade, classes=classes, slots=scene.wide8_slots(), texels=np.ctypeslib.as_array(d.texels, shape=(d.texel_bytes,)).copy())


def run_kernel_bodies(scene, held, edits):
    """The host build of the three passes over `held` (an arrays_of dict, in place); the other pools come from `scene`, which a texel edit leaves alone. Returns
    dict(all_opaque, decided, changed)."""
    d = scene.desc
    array, keep = capi.texel_edits(edits)
    out = np.zeros(3, np.uint32)
    pointer = lambda a: C.c_void_p(a.ctypes.data)
    address = lambda p: C.cast(p, C.c_void_p)
    status = library().texel_update_host_scene(pointer(held["triangles"]), len(held["triangles"]), address(d.instances), d.instance_count, address(d.materials), address(d.indices),
                                               address(d.texcoords), address(d.textures), d.texture_count, pointer(held["texels"]), array, len(keep), pointer(held["trace"]),
                                               pointer(held["shade"]), pointer(held["classes"]), pointer(held["slots"]), len(held["slots"]), pointer(out))
    assert status == 0
    return dict(all_opaque=bool(out[0]), decided=int(out[1]), changed=int(out[2]))
