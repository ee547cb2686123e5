"""What tests/test_texture_lookups_cpu.py and tests/test_gpu_texture_lookups.py share: tiny textures of every format, addressing mode and filter value, quads that carry
them under texture-coordinate ranges inside and far outside [0, 1], the rays aimed at them, and the walk from a hit back to the texture through the description's pools.
Everything is made through the host API (Scene("cornell") emptied of its models + add_texture / add_material / add_mesh / insert_model + rebuild()); the yardstick is
tests/texture_reference.py, which shares no text with the libraries or the oracle."""
import ctypes as C
import itertools

import numpy as np

import texture_reference as ref
from bifrost3d_amd import capi
from bifrost3d_amd.host import Scene, make_camera

SIZES = ((8, 8), (5, 7), (1, 6), (6, 1), (1, 1))      # width x height
FORMATS = (capi.TEXEL_R8, capi.TEXEL_RGBA8, capi.TEXEL_R32F, capi.TEXEL_RGBA32F)
WRAPS = ((True, True), (True, False), (False, True), (False, False))      # repeat in u, v
FILTERS = (0, 1, 2, 3)      # only bit 0 selects bilinear
RANGES = {"unit": (0.0, 1.0), "signed": (-3.25, 2.5), "far": (5.0, 8.0)}      # the texture coordinates across a quad, both axes
TESSELLATION = 12      # 12 x 12 x 2 = 288 triangles
QUADS_PER_SMALL_SCENE = 30      # 60 triangles: the exhaustive search serves up to 64


def pixels_of(width, height, texel_format, salt=0) -> np.ndarray:
    """Texels that are all distinct (in every channel), as the bytes add_texture takes."""
    n = width * height
    i = np.arange(n)
    if texel_format == capi.TEXEL_R8:
        return ((37 * i + 11 + 5 * salt) % 256).astype(np.uint8)
    if texel_format == capi.TEXEL_RGBA8:
        return np.stack([(37 * i + 11 + 67 * c + 5 * salt) % 256 for c in range(4)], axis=1).astype(np.uint8).reshape(-1)
    order = (29 * i + 3 + salt) % 64      # a permutation of 0 .. 63: n <= 64
    if texel_format == capi.TEXEL_R32F:
        return (0.03 + 0.94 * order / 63.0).astype(np.float32).view(np.uint8).reshape(-1)
    return np.stack([0.03 + 0.94 * ((order + 17 * c) % 64) / 63.0 for c in range(4)], axis=1).astype(np.float32).view(np.uint8).reshape(-1)


def texture_specs(formats=FORMATS, srgb=(False, True)) -> list:
    """Every size under every wrap combination and every filter value (80), the formats and the sRGB switch dealt round so that each (format, sRGB) meets nearest and bilinear
    lookups, every size and every wrap combination."""
    kinds = [(f, s) for f in formats for s in srgb]
    specs = []
    for k, (size, wrap, filter_value) in enumerate(itertools.product(SIZES, WRAPS, FILTERS)):
        texel_format, is_srgb = kinds[(k + k // 4 + k // 16) % len(kinds)]
        specs.append(dict(width=size[0], height=size[1], texel_format=texel_format, is_sRGB=is_srgb, repeat=wrap, linear=(bool(filter_value & 1), bool(filter_value & 2)), salt=k))
    return specs


def add_spec(scene, spec) -> int:
    return scene.add_texture(pixels_of(spec["width"], spec["height"], spec["texel_format"], spec.get("salt", 0)) if "pixels" not in spec else spec["pixels"],
                             spec["width"], spec["height"], spec["texel_format"], spec["is_sRGB"], spec["repeat"], spec["linear"])


def material(coverage=1.0, flags=capi.MATERIAL_THIN_WALLED, coverage_texture=0, tint_texture=0, tint=(1.0, 1.0, 1.0), roughness=1.0) -> capi.HiprMaterial:
    m = capi.HiprMaterial()
    m.flags, m.shading_model = flags, capi.SHADING_DEFAULT
    m.tint[:] = tint
    m.roughness, m.specularity, m.metallic, m.coverage = roughness, 0.04, 0.0, coverage
    m.tint_roughness_texture_ID, m.coverage_texture_ID = tint_texture, coverage_texture
    return m


def corner_triangle_mesh(corners) -> dict:
    """One triangle in the plane z = 0 whose corners carry the texture coordinates (0, 0), (A, 0), (0, B): with A and B powers of two (of either sign) the coordinates of
    the hit (u, v) are (A u, B v) EXACTLY in f32, whatever the compiler contracts."""
    a, b = corners
    return dict(positions=np.array([[-0.5, -0.5, 0.0], [0.5, -0.5, 0.0], [-0.5, 0.5, 0.0]], np.float32), primitives=np.array([[0, 1, 2]], np.uint32),
                normals=np.array([[0.0, 0.0, 1.0]] * 3, np.float32), texcoords=np.array([[0.0, 0.0], [a, 0.0], [0.0, b]], np.float32))


def quad_mesh(u_range, v_range=None, cells=1) -> dict:
    """A unit quad in the plane z = 0 facing -z, (cells x cells x 2) triangles, the texture coordinates running over `u_range` along x and `v_range` along y."""
    v_range = v_range or u_range
    steps = np.arange(cells + 1, dtype=np.float64) / cells
    positions, texcoords = [], []
    for j in range(cells + 1):
        for i in range(cells + 1):
            positions.append([steps[i] - 0.5, steps[j] - 0.5, 0.0])
            texcoords.append([u_range[0] + (u_range[1] - u_range[0]) * steps[i], v_range[0] + (v_range[1] - v_range[0]) * steps[j]])
    primitives = []
    at = lambda i, j: j * (cells + 1) + i
    for j in range(cells):
        for i in range(cells):
            primitives += [[at(i, j), at(i + 1, j + 1), at(i + 1, j)], [at(i, j), at(i, j + 1), at(i + 1, j + 1)]]
    return dict(positions=np.array(positions, np.float32), primitives=np.array(primitives, np.uint32), normals=np.array([[0.0, 0.0, -1.0]] * len(positions), np.float32),
                texcoords=np.array(texcoords, np.float32))


def empty_cornell() -> Scene:
    """The Cornell box's lights and camera without its models: the quads of a case are the only triangles."""
    scene = Scene("cornell")
    removed = sum(1 for model in range(1, 64) if scene.remove_model(model))
    assert removed >= 1
    return scene


COLUMNS = 16


def place(k):
    return (float(k % COLUMNS) - 0.5 * (COLUMNS - 1), float(k // COLUMNS), 0.0)


class QuadScene:
    """A host scene of quads, one per (texture spec, material, mesh): quads[k] = dict(spec, texture, material, mesh, centre)."""

    def __init__(self, entries, cells=1, extra=None):
        """`entries`: a list of (spec, make_material(texture index) -> HiprMaterial, mesh arguments for quad_mesh). `extra`: called with the scene before the build, for
        whatever else the pools shall hold."""
        self.scene = empty_cornell()
        self.quads, meshes, textures = [], {}, {}
        for k, (spec, make_material, mesh_arguments) in enumerate(entries):
            key = tuple(sorted((name, repr(value)) for name, value in mesh_arguments.items()))
            if key not in meshes:
                meshes[key] = self.scene.add_mesh(**(corner_triangle_mesh(**mesh_arguments) if "corners" in mesh_arguments else quad_mesh(cells=cells, **mesh_arguments)))
            if id(spec) not in textures:
                textures[id(spec)] = add_spec(self.scene, spec)
            texture = textures[id(spec)]
            material_index = self.scene.add_material(make_material(texture))
            self.scene.insert_model(100000, meshes[key], material_index, translation=place(k), model_index=1000 + k)
            self.quads.append(dict(spec=spec, texture=texture, material=material_index, mesh=mesh_arguments, centre=place(k)))
        if extra is not None:
            extra(self.scene)
        self.scene.rebuild()
        self.cells = cells

    # what Context.upload_scene, the oracle and DeviceShadeOnHost read of a scene
    @property
    def desc(self):
        return self.scene.desc

    @property
    def state(self):
        return self.scene.state

    def camera(self, *args, **kwargs):
        return self.scene.camera(*args, **kwargs)


class Pools:
    """The pools of a description as numpy arrays, and the walk from a triangle of it to its corners' texture coordinates, its material and its textures."""

    def __init__(self, desc):
        d = desc
        words = lambda pointer, rows, width, dtype=np.uint32: (np.ctypeslib.as_array(C.cast(pointer, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(rows, width)).copy()
                                                               if rows and pointer else np.zeros((0, width), dtype))
        self.triangles = words(d.triangles, d.triangle_count, 12)
        self.instances = words(d.instances, d.instance_count, 20)
        self.indices = words(d.indices, d.index_count, 1).reshape(-1)
        self.texcoords = words(d.texcoords, d.vertex_count, 2, np.float32)
        self.materials = [capi.HiprMaterial.from_buffer_copy(bytes(d.materials[k])) for k in range(d.material_count)]
        self.textures = [capi.HiprTexture.from_buffer_copy(bytes(d.textures[k])) for k in range(d.texture_count)]
        self.texels = words(d.texels, d.texel_bytes, 1, np.uint8).reshape(-1)

    def instance_of(self, triangles):
        return self.triangles[np.asarray(triangles, np.int64), 9]

    def material_of(self, triangles):
        return self.instances[self.instance_of(triangles), 15].astype(np.int64)

    def flags_of(self, triangles):
        return self.triangles[np.asarray(triangles, np.int64), 11]

    def corner_texcoords(self, triangles) -> np.ndarray:
        """(n, 3, 2) float64: the texture coordinates of the triangles' corners through instance, index triple and the pooled attribute."""
        triangles = np.asarray(triangles, np.int64)
        instance = self.instances[self.instance_of(triangles)]
        first = 3 * (instance[:, 12].astype(np.int64) + self.triangles[triangles, 10].astype(np.int64))
        corners = np.stack([self.indices[first + c].astype(np.int64) for c in range(3)], axis=1) + instance[:, 13].astype(np.int64)[:, None]
        return self.texcoords[corners].astype(np.float64)

    def texcoord(self, triangles, u, v) -> np.ndarray:
        """t1 u + t2 v + t0 (1 - u - v), in float64."""
        t = self.corner_texcoords(triangles)
        u, v = np.asarray(u, np.float64)[:, None], np.asarray(v, np.float64)[:, None]
        return t[:, 1] * u + t[:, 2] * v + t[:, 0] * (1.0 - u - v)


def rays_at_quads(quads, per_quad, seed, half=0.47) -> np.ndarray:
    """Rays from in front of the quads' plane (z < 0), each aimed at a random point of one quad; every other one ends behind the plane at a finite tmax."""
    rng = np.random.default_rng(seed)
    n = per_quad * len(quads)
    centres = np.repeat(np.array([q["centre"] for q in quads], np.float64), per_quad, axis=0)
    target = centres + np.concatenate([rng.uniform(-half, half, (n, 2)), np.zeros((n, 1))], axis=1)
    origin = target + np.concatenate([rng.uniform(-0.6, 0.6, (n, 2)), -rng.uniform(1.0, 3.0, (n, 1))], axis=1)
    direction = target - origin
    length = np.linalg.norm(direction, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 4:7] = origin, direction / length
    rays[:, 7] = np.inf
    rays[1::2, 7] = (length[1::2, 0] * rng.uniform(1.2, 2.0, len(rays[1::2]))).astype(np.float32)
    return rays


def same_bits(a, b) -> np.ndarray:
    """Per f32 word: the same bits, or a NaN on both sides."""
    return (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def lookup_tolerance(texture, texels, values, arithmetic_roundings=2, srgb_relative=None) -> np.ndarray:
    """The absolute tolerance of looked-up `values` (see texture_reference's docstring): 2^-11 of the value range for a filtered lookup, 4 ulp of the value for the sRGB
    decode (`srgb_relative`: the fast unit's relative bound instead) or the one division of a linear texel, and half an ulp of 1 for each of the `arithmetic_roundings`
    that follow the lookup (coverage * tex, 1 - coverage, tint * tex: operands at most 1)."""
    values = np.asarray(values, np.float64)
    tolerance = 4.0 * ulp32(values) + arithmetic_roundings * 2.0 ** -24
    if texture is not None and ref.is_bilinear(texture):
        tolerance = tolerance + ref.FILTER_TOLERANCE * ref.value_range(texture, texels)
    if srgb_relative is not None and texture is not None and texture.is_sRGB:
        tolerance = tolerance + srgb_relative * np.abs(values)
    return tolerance


def free_camera(width, height, position, accumulations=0, max_bounce_count=0):
    return make_camera(width, height, position=position, accumulations=accumulations, max_bounce_count=max_bounce_count)


def expected_coverage(pools, triangles, u, v, srgb_relative=None):
    """The reference's coverage at the hits (triangle, u, v) of a description, through the pools: -> (coverage, tolerance, excluded), each (n,). Excluded: nearest lookups
    within 2^-12 texel of a texel edge, and cut-out decisions whose filtered texel lies within its tolerance of the threshold (either answer is then right)."""
    triangles = np.asarray(triangles, np.int64)
    uv = pools.texcoord(triangles, u, v)
    materials = pools.material_of(triangles)
    cover, tolerance, excluded = np.ones(len(triangles)), np.zeros(len(triangles)), np.zeros(len(triangles), bool)
    for index in np.unique(materials):
        chosen = materials == index
        m = pools.materials[index]
        texture = pools.textures[m.coverage_texture_ID] if m.coverage_texture_ID else None
        cover[chosen] = ref.coverage(m, texture, pools.texels, uv[chosen])
        if texture is None:
            continue
        tex = ref.sample(texture, pools.texels, uv[chosen])[:, 0]
        tolerance[chosen] = lookup_tolerance(texture, pools.texels, tex, srgb_relative=srgb_relative)
        excluded[chosen] = ref.excluded(texture, uv[chosen])
        if m.flags & capi.MATERIAL_CUTOUT:
            excluded[chosen] |= np.abs(tex - float(m.coverage)) <= tolerance[chosen]
    return cover, tolerance, excluded


def held_to_reference(tag, got, expected, tolerance, excluded, allowed_share=0.01):
    """Prints the tagged line of a leg -- its worst error over the kept samples, against the tolerance there, and the share left out -- and asserts both."""
    got, expected = np.asarray(got, np.float64), np.asarray(expected, np.float64)
    if got.ndim > 1:
        tolerance, excluded = np.broadcast_to(np.asarray(tolerance)[..., None] if np.ndim(tolerance) < got.ndim else tolerance, got.shape), np.asarray(excluded)
    kept = ~excluded
    error = np.abs(got - expected)[kept]
    allowed = np.broadcast_to(tolerance, got.shape)[kept]
    worst = int(np.argmax(error - allowed)) if error.size else 0
    share = float(excluded.mean()) if excluded.size else 0.0
    print(f"LOOKUPS {tag}: {int(kept.sum())} samples, worst error {float(error.max()) if error.size else 0.0:.3e} (largest excess over its tolerance {float((error - allowed).max()) if error.size else 0.0:.3e}, "
          f"tolerance there {float(np.ravel(allowed)[worst]) if error.size else 0.0:.3e}), excluded share {share:.5f}")
    if allowed_share is not None:      # None: constructed inputs that sit on texel edges on purpose, held to whatever a nearest lookup leaves of them
        assert share <= allowed_share, (tag, share)
    assert error.size, (tag, "every sample was left out")
    assert (error <= allowed).all(), (tag, float(error.max()), int((error > allowed).sum()))
    return share


def expected_transmittance(trace_closest, pools, rays, srgb_relative=None):
    """1 - the reference's coverage where each of `rays` (every one aimed at a quad, which it reaches before its tmax) hits; `trace_closest`: rays -> hits (n, 4)."""
    unbounded = rays.copy()
    unbounded[:, 7] = np.inf
    hits = trace_closest(unbounded)
    triangles = hits[:, 3].view(np.uint32)
    assert (triangles < len(pools.triangles)).all(), "every ray is aimed at a quad"
    cover, tolerance, excluded = expected_coverage(pools, triangles, hits[:, 1], hits[:, 2], srgb_relative)
    return ref.transmittance(cover), tolerance, excluded


def coverage_entries(specs):
    """One quad per (texture, range of texture coordinates); the materials alternate between coverage 1 and 0.75, every fifth is a cut-out at 0.5."""
    entries = []
    for k, spec in enumerate(specs):
        for r, name in enumerate(RANGES):
            kind = (k + r) % 5
            make = (lambda t, kind=kind: material(coverage=0.5, flags=capi.MATERIAL_THIN_WALLED | capi.MATERIAL_CUTOUT, coverage_texture=t) if kind == 4
                    else material(coverage=(1.0, 0.75)[kind % 2], coverage_texture=t))
            entries.append((spec, make, dict(u_range=RANGES[name])))
    return entries


def coverage_scenes(specs=None, seed=7, per_small_quad=100, per_tessellated_quad=16) -> dict:
    """{"two_triangle_quads": [(QuadScene, rays)] of at most 60 triangles each (the exhaustive search's scenes), "tessellated_quads": [(QuadScene, rays)] (the trees')}."""
    entries = coverage_entries(specs if specs is not None else texture_specs())
    small = [QuadScene(entries[k: k + QUADS_PER_SMALL_SCENE]) for k in range(0, len(entries), QUADS_PER_SMALL_SCENE)]
    tessellated = QuadScene(entries, cells=TESSELLATION)
    return {"two_triangle_quads": [(s, rays_at_quads(s.quads, per_small_quad, seed + k)) for k, s in enumerate(small)],
            "tessellated_quads": [(tessellated, rays_at_quads(tessellated.quads, per_tessellated_quad, seed + 100))]}


# ---- the cases of the upload-time rule covered_everywhere (csrc/material_rules.h) ----
SOLID, THRESHOLD = 255, 128      # a plain material is opaque where every texel is 1; the cut-outs' threshold is 128 / 255, their field one step above it, their hole one below
HOLES = {"interior": (3, 4), "left_border": (0, 3), "right_border": (7, 3), "bottom_border": (3, 0), "top_border": (3, 7), "none": None}
RULE_RANGES = {"unit": (0.0, 1.0), "across_the_seams": (-0.25, 1.25)}      # the second shows the border texels again on the far side of the repeat seam


def rule_entries():
    """Quads of an 8 x 8 coverage texture that is solid but for one open texel -- inside, at each border, and (under texture coordinates that pass 0 and 1) just across the
    repeat seam --, nearest and bilinear, under three wrap combinations; for plain materials of coverage 1 (R8, some RGBA8) and for cut-outs at threshold +- 1 / 255."""
    entries = []
    for cutout in (False, True):
        field, hole_value = (THRESHOLD + 1, THRESHOLD - 1) if cutout else (SOLID, 0)
        for name, hole in HOLES.items():
            if cutout and name not in ("interior", "left_border", "none"):
                continue
            for wrap in ((True, True), (False, False), (True, False)):
                if name in ("interior", "none") and wrap != (True, True) and not cutout:
                    continue
                for bilinear in (False, True):
                    for range_name, uv_range in RULE_RANGES.items():
                        four = (len(entries) % 3 == 2)      # every third as RGBA8: the rule reads the sampler's .x
                        pixels = np.full((8, 8), field, np.uint8)
                        if hole is not None:
                            pixels[hole[1], hole[0]] = hole_value
                        if four:
                            pixels = np.stack([pixels, np.full((8, 8), 7, np.uint8), np.full((8, 8), 9, np.uint8), np.full((8, 8), 0, np.uint8)], axis=-1)
                        spec = dict(width=8, height=8, texel_format=capi.TEXEL_RGBA8 if four else capi.TEXEL_R8, is_sRGB=False, repeat=wrap, linear=(bilinear, False),
                                    pixels=pixels.reshape(-1), hole=hole, cutout=cutout, name=f"{'cutout' if cutout else 'plain'} {name} wrap {wrap} bilinear {bilinear} {range_name}")
                        make = (lambda t, cutout=cutout: material(coverage=np.float32(THRESHOLD) / np.float32(255.0) if cutout else 1.0,
                                                                    flags=capi.MATERIAL_THIN_WALLED | (capi.MATERIAL_CUTOUT if cutout else 0), coverage_texture=t))
                        entries.append((spec, make, dict(u_range=uv_range)))
    return entries


def barycentric_lattice(n=32) -> np.ndarray:
    """(u, v) of an (n + 1)-point-per-edge lattice over a triangle, with the corners and the edge midpoints."""
    points = [(i / n, j / n) for i in range(n + 1) for j in range(n + 1 - i)]
    points += [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5)]
    return np.array(points, np.float64)


def lattice_coverage(pools, triangles, lattice, displacement_texels=0.0) -> np.ndarray:
    """The reference's coverage of the triangles (all of ONE material) at every lattice point: (triangles, points). `displacement_texels`: the points are also looked up
    displaced by that much along the four diagonals (what the f32 interpolation of the device may make of them), and the smallest coverage is returned."""
    triangles = np.asarray(triangles, np.int64)
    m = pools.materials[int(pools.material_of(triangles[:1])[0])]
    texture = pools.textures[m.coverage_texture_ID]
    t = pools.corner_texcoords(triangles)
    u, v = lattice[None, :, 0, None], lattice[None, :, 1, None]
    uv = t[:, None, 1] * u + t[:, None, 2] * v + t[:, None, 0] * (1.0 - u - v)
    steps = [(0.0, 0.0)] + ([(a, b) for a in (-1.0, 1.0) for b in (-1.0, 1.0)] if displacement_texels else [])
    worst = None
    for a, b in steps:
        moved = uv + np.array([a * displacement_texels / texture.width, b * displacement_texels / texture.height])
        cover = ref.coverage(m, texture, pools.texels, moved.reshape(-1, 2)).reshape(len(triangles), -1)
        worst = cover if worst is None else np.minimum(worst, cover)
    return worst


# ---- the tint / roughness AOVs: a white material shows the tint-roughness texture itself ----
FRAME = (64, 36)


def tint_entries(specs):
    return [(spec, (lambda t: material(tint_texture=t)), dict(u_range=RANGES[name])) for spec in specs for name in RANGES]


def frame_cameras(quad_count, max_bounce_count=0, accumulations=0) -> list:
    """Free cameras in front of the quads' plane, each over a block of 8 x 4 quads of the grid, 64 x 36 pixels."""
    rows = (quad_count + COLUMNS - 1) // COLUMNS
    return [free_camera(FRAME[0], FRAME[1], (float(column) - 0.5 * (COLUMNS - 1) + 3.5, float(row) + 1.5, -6.0), accumulations, max_bounce_count)
            for row in range(0, rows, 4) for column in range(0, COLUMNS, 8)]


def all_pixels():
    ys, xs = np.mgrid[0:FRAME[1], 0:FRAME[0]]
    return np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.uint32)


def expected_tint_roughness(pools, hits, srgb_relative=None):
    """RGBA of the reference at the hits whose triangle is a quad's: -> (on a quad (n,), value (n, 4), tolerance (n, 4), excluded (n,)); a white material of roughness 1
    shows the texture's RGB as its tint and its A as its roughness."""
    triangles = hits[:, 3].view(np.uint32)
    on = triangles < len(pools.triangles)
    value, tolerance, excluded = np.zeros((len(hits), 4)), np.zeros((len(hits), 4)), np.zeros(len(hits), bool)
    uv = pools.texcoord(np.where(on, triangles, 0), hits[:, 1], hits[:, 2])
    materials = pools.material_of(np.where(on, triangles, 0))
    for index in np.unique(materials[on]):
        chosen = on & (materials == index)
        texture = pools.textures[pools.materials[index].tint_roughness_texture_ID]
        value[chosen] = ref.sample(texture, pools.texels, uv[chosen])
        tolerance[chosen] = lookup_tolerance(texture, pools.texels, value[chosen], srgb_relative=srgb_relative)
        excluded[chosen] = ref.excluded(texture, uv[chosen])
    return on, value, tolerance, excluded


# ---- cut-out decisions of the shade stage: hits with chosen barycentrics ----
CORNERS = ((1.0, 1.0), (-4.0, 2.0), (8.0, -8.0), (0.5, 4.0))      # (A, B): the texture coordinates of a hit are (A u, B v), exactly


def threshold_of(spec) -> float:
    """A cut-out threshold between the two middle values of the texture's .x (a lone texel: 0.2 to its other side), as an f32."""
    from types import SimpleNamespace
    texture = SimpleNamespace(width=spec["width"], height=spec["height"], texel_offset=0, format=spec["texel_format"], is_sRGB=spec["is_sRGB"])
    values = np.unique(ref.decoded_texels(texture, pixels_of(spec["width"], spec["height"], spec["texel_format"], spec.get("salt", 0)))[..., 0])
    if len(values) == 1:
        return float(np.float32(values[0] + (0.2 if values[0] < 0.5 else -0.2)))
    return float(np.float32(0.5 * (values[len(values) // 2 - 1] + values[len(values) // 2])))


def cutout_entries(specs):
    """One triangle per texture, the pairs (A, B) dealt round; each a cut-out at a threshold in the middle of its texture's values."""
    return [(spec, (lambda t, spec=spec: material(coverage=threshold_of(spec), flags=capi.MATERIAL_THIN_WALLED | capi.MATERIAL_CUTOUT, coverage_texture=t)),
             dict(corners=CORNERS[(k + k // 4) % len(CORNERS)])) for k, spec in enumerate(specs)]


def chosen_hits(quads, per_triangle, seed):
    """Queue entries of hipr_debug_shade that hit triangle k of the scene at random barycentrics: -> (rays, throughput_bounces, hits, last_triangle, pixel_hash, accumulation)."""
    rng = np.random.default_rng(seed)
    triangle_count = quads.desc.triangle_count
    n = per_triangle * triangle_count
    u = rng.uniform(0.0, 1.0, n)
    v = rng.uniform(0.0, 1.0, n) * (1.0 - u)
    u, v = u.astype(np.float32), v.astype(np.float32)
    triangles = np.repeat(np.arange(triangle_count, dtype=np.uint32), per_triangle)
    pools = Pools(quads.desc)
    corners = pools.triangles[triangles, :9].view(np.float32).reshape(n, 3, 3).astype(np.float64)
    position = corners[:, 1] * u[:, None] + corners[:, 2] * v[:, None] + corners[:, 0] * (1.0 - u - v)[:, None]
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = position - np.array([0.0, 0.0, 2.0])
    rays[:, 4:7] = (0.0, 0.0, 1.0)
    rays[:, 7] = -1.0      # the BSDF PDF of the ray: a delta
    hits = np.zeros((n, 4), np.float32)
    hits[:, 0], hits[:, 1], hits[:, 2] = 2.0, u, v
    hits[:, 3] = triangles.view(np.float32)
    throughput = np.zeros((n, 4), np.float32)
    throughput[:, :3] = 1.0
    return rays, throughput, hits, np.full(n, 0xFFFFFFFF, np.uint32), rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32), np.full(n, 3, np.uint32)


def decisions(records) -> np.ndarray:
    """Per record of hipr_debug_shade: True where the hit was shaded, False where it was rejected and the same ray goes on; anything else is an error."""
    flags = np.ascontiguousarray(records[:, 0]).view(np.uint32)
    shaded, continues = (flags & 4) != 0, (flags & 1) != 0
    assert (shaded | continues).all(), "a hit on a cut-out is shaded or sends its ray on"
    return shaded


# ---- environment lookups through the miss program ----
class EnvironmentScene:
    """A scene's description with textures, texels and an environment of its own (a copy: the scene stays as it is), and a tint of its own in the state."""

    def __init__(self, scene, spec, pixels, pdf_size, per_pixel_PDF, tint=(0.9, 0.6, 0.3)):
        self.scene = scene
        self.textures = (capi.HiprTexture * 2)()
        t = self.textures[1]
        t.width, t.height, t.texel_offset, t.format = spec["width"], spec["height"], 0, spec["texel_format"]
        t.wrap_u, t.wrap_v, t.filter, t.is_sRGB = int(spec["repeat"][0]), int(spec["repeat"][1]), int(spec["linear"][0]) | 2 * int(spec["linear"][1]), int(spec["is_sRGB"])
        self.texels = np.ascontiguousarray(pixels).view(np.uint8).reshape(-1).copy()
        self.per_pixel_PDF = np.ascontiguousarray(per_pixel_PDF, np.float32).reshape(-1)
        self.samples = (capi.HiprLightSample * 1)()
        self.samples[0].direction_to_light[:] = (0.0, 1.0, 0.0)
        self.samples[0].PDF, self.samples[0].distance = 1.0, 1e30
        self.environment = capi.HiprEnvironment(1, pdf_size[0], pdf_size[1], self.per_pixel_PDF.ctypes.data_as(C.POINTER(C.c_float)), self.samples, 1)
        self._desc = capi.HiprSceneDesc.from_buffer_copy(scene.desc)
        self._desc.textures, self._desc.texture_count = C.cast(self.textures, C.POINTER(capi.HiprTexture)), 2
        self._desc.texels, self._desc.texel_bytes = self.texels.ctypes.data_as(C.POINTER(C.c_uint8)), self.texels.nbytes
        self._desc.environment = C.pointer(self.environment)
        self.tint = tint

    @property
    def desc(self):
        return self._desc

    @property
    def state(self):
        s = self.scene.state
        s.environment_tint[:] = self.tint
        return s

    def camera(self, *args, **kwargs):
        return self.scene.camera(*args, **kwargs)


ENVIRONMENT_MAP = (8, 4)
ENVIRONMENT_PDF = (5, 3)


NEAREST_ENVIRONMENT_MAP = (7, 3)      # the named directions (axes, poles, the plane x = 0) lie at u = k / 4, v = k / 2: ON the texel edges of an 8 x 4 map, where a nearest lookup is left out; between them here


def constructed_environment(scene, repeat, bilinear=True, size=ENVIRONMENT_MAP):
    """An 8 x 4 (or `size`) RGBA32F map of distinct texels with radiances up to 6, and a 5 x 3 PDF image of distinct positive values."""
    i = np.arange(size[0] * size[1])
    pixels = np.stack([0.25 + 6.0 * ((13 * i + 5 * c + 1) % 32) / 32.0 for c in range(4)], axis=1).astype(np.float32)
    pdf = (0.05 + 0.11 * ((7 * np.arange(ENVIRONMENT_PDF[0] * ENVIRONMENT_PDF[1]) + 2) % 15)).astype(np.float32)
    spec = dict(width=size[0], height=size[1], texel_format=capi.TEXEL_RGBA32F, is_sRGB=False, repeat=repeat, linear=(bilinear, bilinear))
    return EnvironmentScene(scene, spec, pixels, ENVIRONMENT_PDF, pdf)


def environment_directions(pdf_size, count, seed) -> dict:
    """Unit directions, by kind: random ones with |y| <= 0.99, the named edges (the poles, the seam (-1, 0, +-0), the axes, the plane x = 0), and directions on the texel
    edges of the PDF image."""
    rng = np.random.default_rng(seed)
    y = rng.uniform(-0.99, 0.99, count)
    phi = rng.uniform(-np.pi, np.pi, count)
    r = np.sqrt(1.0 - y * y)
    random = np.stack([r * np.cos(phi), y, r * np.sin(phi)], axis=1)
    named = [[0, 1, 0], [0, -1, 0], [-1, 0, 0.0], [-1, 0, -0.0], [1, 0, 0], [0, 0, 1], [0, 0, -1], [1, 0, -0.0], [-0.0, 0, 1], [-0.0, 0, -1]]
    for angle in np.linspace(-1.4, 1.4, 9):
        named += [[0.0, np.sin(angle), np.cos(angle)], [0.0, np.sin(angle), -np.cos(angle)], [-0.0, np.sin(angle), np.cos(angle)]]
    edges = []
    for k in np.unique(np.linspace(0, pdf_size[0], 9).astype(int)):      # at most nine edges per axis, the outer ones among them
        for j in np.unique(np.linspace(0, pdf_size[1], 9).astype(int)):
            theta, azimuth = np.pi * j / pdf_size[1] - np.pi / 2.0, 2.0 * np.pi * k / pdf_size[0] - np.pi
            edges.append([np.cos(theta) * np.cos(azimuth), np.sin(theta), np.cos(theta) * np.sin(azimuth)])
        edges.append([np.cos(0.3) * np.cos(2.0 * np.pi * k / pdf_size[0] - np.pi), np.sin(0.3), np.cos(0.3) * np.sin(2.0 * np.pi * k / pdf_size[0] - np.pi)])
    out = {"random": random, "named": np.array(named, np.float64), "pdf_texel_edges": np.array(edges, np.float64)}
    for name, d in out.items():      # unit length as f32 sees it; the signs of the zeros stay
        d32 = d.astype(np.float32)
        out[name] = d32
    return out


def miss_entries(directions, bsdf_pdf):
    """Queue entries of hipr_debug_shade for rays that escaped along `directions` with the given BSDF PDFs (negative: a delta)."""
    n = len(directions)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 4:7] = directions
    rays[:, 7] = bsdf_pdf
    hits = np.zeros((n, 4), np.float32)
    hits[:, 3] = np.full(n, 0xFFFFFFFF, np.uint32).view(np.float32)
    throughput = np.zeros((n, 4), np.float32)
    throughput[:, :3] = 1.0
    return rays, throughput, hits, np.full(n, 0xFFFFFFFF, np.uint32), np.arange(n, dtype=np.uint32) * np.uint32(2654435761), np.full(n, 3, np.uint32)


def environment_of(desc):
    """(texture, texel pool, PDF image (h, w)) of a description's environment."""
    e = desc.environment.contents
    texture = capi.HiprTexture.from_buffer_copy(bytes(desc.textures[e.environment_map_ID]))
    texels = np.ctypeslib.as_array(desc.texels, shape=(desc.texel_bytes,)).copy()
    pdf = np.ctypeslib.as_array(e.per_pixel_PDF, shape=(e.pdf_height, e.pdf_width)).copy()
    return texture, texels, pdf


def expected_environment(desc, tint, directions, with_mis, srgb_relative=None, mis_relative=1e-5):
    """What the miss program adds for a ray of throughput 1 along `directions` (f32): -> (BSDF PDFs to give the rays, [radiance (n, 3)] alternatives, tolerance (n, 3),
    excluded (n,)). Without MIS (a delta BSDF PDF, -1) it is evaluate; with it the BSDF PDF is the reference's own environment PDF -- 1 where that is the delta of the
    poles, which weighs nothing -- and the radiance is evaluate * p / (p + pdf). A direction within 2^-12 texel of a texel edge of the PDF image has the PDF of either
    side: one alternative per neighbour. Excluded: nearest lookups of the MAP within 2^-12 texel of an edge."""
    texture, texels, pdf_image = environment_of(desc)
    d = np.asarray(directions, np.float32).astype(np.float64)
    uv = ref.latlong_texcoord(d)
    texel = ref.sample(texture, texels, uv)[:, :3]
    radiance = ref.environment_evaluate(tint, texture, texels, d)
    tolerance = lookup_tolerance(texture, texels, texel, srgb_relative=srgb_relative) * np.maximum(np.asarray(tint, np.float64)[None, :], 1.0) + 4.0 * ulp32(radiance)
    excluded = ref.excluded(texture, uv)
    if not with_mis:
        return np.full(len(d), -1.0, np.float32), [radiance], tolerance, excluded
    width, height = pdf_image.shape[1], pdf_image.shape[0]
    pdf = ref.environment_pdf(pdf_image, width, height, d)
    given = np.where(np.signbit(pdf) | (pdf == 0.0), 1.0, pdf).astype(np.float32)
    alternatives = []
    for a in (0.0, -2.0 * ref.EDGE_MARGIN, 2.0 * ref.EDGE_MARGIN):
        for b in (0.0, -2.0 * ref.EDGE_MARGIN, 2.0 * ref.EDGE_MARGIN):
            weight = ref.balance_heuristic(given.astype(np.float64), np.abs(ref.environment_pdf(pdf_image, width, height, d, (a, b))))
            alternatives.append(radiance * weight[:, None])
    near = ref.environment_pdf_excluded(width, height, d)
    alternatives = [alternatives[0]] + [np.where(near[:, None], alternative, alternatives[0]) for alternative in alternatives[1:]]
    return given, alternatives, tolerance + mis_relative * np.abs(alternatives[0]), excluded


def nearest_alternative(got, alternatives) -> np.ndarray:
    """Per row the alternative whose largest channel error against `got` is smallest."""
    errors = np.stack([np.abs(np.asarray(got, np.float64) - alternative).max(axis=1) for alternative in alternatives])
    return np.stack(alternatives)[np.argmin(errors, axis=0), np.arange(len(got))]
