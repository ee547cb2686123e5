/* hiprenderer_c.h -- C-ABI of the HIPRenderer path-tracing kernels for MI355X (gfx950).
 *
 * This is the drop-in boundary between a Bifrost host renderer and the hand-written HIP
 * wavefront path tracer. Every entry point replaces one interaction the reference
 * OptiXRenderer host code has with the OptiX 6.5 runtime. Paths below are relative to
 * /root/reference/extensions/OptiXRenderer/OptiXRenderer/ ("OR/").
 *
 * Conventions
 *  - All functions return an int status: HIPR_OK (0) or a negative HiprStatus. No exceptions
 *    cross the ABI. hipr_last_error() returns a thread-local human readable message.
 *  - The library never takes ownership of caller memory: uploads copy.
 *  - Pointers named *_device are device (HBM) pointers, everything else is host memory.
 *  - Single-threaded contract per context, as the reference (BF/Core/Engine.cpp:36-49).
 *  - Image rows: row 0 is the bottom row (the reference adaptor flips Y when blitting,
 *    extensions/DX11OptiXAdapter/DX11OptiXAdapter/Adaptor.cpp:113-115).
 */
#ifndef HIPRENDERER_C_H
#define HIPRENDERER_C_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------- */
/* Status codes                                                                                */
/* ------------------------------------------------------------------------------------------- */
typedef enum HiprStatus {
    HIPR_OK = 0,
    HIPR_ERROR_INVALID_ARGUMENT = -1,
    HIPR_ERROR_NO_DEVICE = -2,      /* OR/Renderer.cpp:280-281 returns an invalid renderer */
    HIPR_ERROR_OUT_OF_MEMORY = -3,
    HIPR_ERROR_HIP = -4,            /* a HIP runtime call failed, see hipr_last_error() */
    HIPR_ERROR_NOT_READY = -5,      /* render before tables/scene/frame were set */
    HIPR_ERROR_UNSUPPORTED = -6,
    HIPR_ERROR_TIMEOUT = -7         /* a device group's tile exchange did not finish within its deadline (hipr_group_accumulate_samples); hipr_last_error() names the member */
} HiprStatus;

/* ------------------------------------------------------------------------------------------- */
/* Device PODs. Layouts follow the reference's device structs so the host code fills them the  */
/* same way (OR/Types.h). All are tightly packed little-endian.                                */
/* ------------------------------------------------------------------------------------------- */

/* OR/Types.h:353-383, 64 bytes. flags: 1 = ThinWalled, 2 = Cutout. shading_model: 0 Default,
 * 1 Diffuse, 2 Transmissive. coat / coat_roughness are UNorm16 (OR/Types.h:76-93). Texture IDs
 * are indices into HiprSceneDesc::textures, 0 = none. */
typedef struct HiprMaterial {
    uint16_t flags;
    uint16_t shading_model;
    float tint[3];
    float roughness;
    int32_t tint_roughness_texture_ID;
    int32_t roughness_texture_ID;
    float specularity;
    float metallic;
    int32_t metallic_texture_ID;
    float coverage;
    int32_t coverage_texture_ID;
    float emission[3];
    uint16_t coat;
    uint16_t coat_roughness;
} HiprMaterial;

enum { HIPR_MATERIAL_THIN_WALLED = 1, HIPR_MATERIAL_CUTOUT = 2 };
enum { HIPR_SHADING_DEFAULT = 0, HIPR_SHADING_DIFFUSE = 1, HIPR_SHADING_TRANSMISSIVE = 2 };

/* OR/Types.h:290-312, 48 bytes. `data` is the union payload:
 *   Sphere      : power[0..2] position[3..5] radius[6]
 *   Spot        : power[0..2] position[3..5] radius[6] direction[7..9] cos_angle[10]
 *   Directional : radiance[0..2] direction[3..5]
 * flags & 7 is the light type. */
typedef struct HiprLight {
    float data[11];
    uint32_t flags;
} HiprLight;

enum { HIPR_LIGHT_NONE = 0, HIPR_LIGHT_SPHERE = 1, HIPR_LIGHT_DIRECTIONAL = 2, HIPR_LIGHT_ENVIRONMENT = 3,
       HIPR_LIGHT_PRESAMPLED_ENVIRONMENT = 4, HIPR_LIGHT_SPOT = 5, HIPR_LIGHT_TYPE_MASK = 7 };

/* OR/Types.h:116-119, 16 bytes: float3 position + octahedral SNORM16 normal
 * (encode BF/Math/OctahedralNormal.h:53-83, decode OR/Types.h:62-69). Positions are in
 * OBJECT space, the normal as well. */
typedef struct HiprVertexGeometry {
    float position[3];
    int16_t oct_normal[2];
} HiprVertexGeometry;

/* OR/Types.h:46-52 */
enum { HIPR_MESH_NORMALS = 1, HIPR_MESH_TEXCOORDS = 2, HIPR_MESH_TINTS = 4, HIPR_MESH_EMISSIVE = 8 };

/* One per mesh model. Replaces the OptiX Transform -> GeometryGroup -> GeometryInstance chain
 * and its ModelState / mesh_flags variables (OR/Renderer.cpp:138-182, OR/Types.h:477-480).
 * Offsets index the pooled attribute arrays of HiprSceneDesc; an unused attribute's offset is
 * ignored (gated by mesh_flags exactly as ORS/TriangleAttributes.cu:50-83). */
typedef struct HiprInstance {
    float object_to_world[12];  /* row-major 3x4, to_matrix3x4(Transform) (BF/Math/Conversions.h:69-75) */
    uint32_t index_offset;      /* first uint3 of this mesh in `indices` */
    uint32_t vertex_offset;     /* first vertex of this mesh in `geometry` / `texcoords` / `tints` / `emissions` */
    int32_t instance_id;        /* InstanceID bits: (1 << 30) | mesh model index (OR/Types.h:121-138) */
    int32_t material_index;
    uint32_t mesh_flags;
    uint32_t _pad[3];
} HiprInstance;

/* World-space triangle in BVH leaf order, 48 bytes. Built by the host flattening the
 * instances (replaces the OptiX "Trbvh" build, OR/Renderer.cpp:161-182,471-476). */
typedef struct HiprTriangle {
    float v0[3];
    float v1[3];
    float v2[3];
    uint32_t instance_index;   /* index into HiprSceneDesc::instances */
    uint32_t primitive_index;  /* rtGetPrimitiveIndex() equivalent within the mesh */
    uint32_t flags;            /* HIPR_TRIANGLE_* */
} HiprTriangle;

enum {
    HIPR_TRIANGLE_OPAQUE = 1,    /* shadow rays terminate here: coverage is statically 1 (ORS/MonteCarlo.cu:278-285) */
    /* 2 is taken inside the device library (a flag of the exhaustive-search items) */
    HIPR_TRIANGLE_ONE_SIDED = 4  /* the hit program refuses a closest hit that arrives from behind and the path's ray is traced again from just past it
                                    (ORS/MonteCarlo.cu:147-164: the material is neither thin-walled nor a cut-out nor transmissive). The 8-wide search uses it to
                                    step over such a hit inside the traversal (hipr_set_backface_culling). May only be set where the instance's material is
                                    one-sided (validated); leaving it unset is always correct. */
};

/* BVH2 node, 64 bytes. Child c spans lo/hi boxes stored Aila-Laine style:
 *   c0xy = { c0.lo.x, c0.hi.x, c0.lo.y, c0.hi.y }
 *   c1xy = { c1.lo.x, c1.hi.x, c1.lo.y, c1.hi.y }
 *   cz   = { c0.lo.z, c0.hi.z, c1.lo.z, c1.hi.z }
 * child >= 0 : index of an inner node.
 * child <  0 : leaf, ~child = (first_triangle << 3) | (triangle_count - 1), count in [1, 8]. */
typedef struct HiprBvhNode {
    float c0xy[4];
    float c1xy[4];
    float cz[4];
    int32_t child[2];
    uint32_t _pad[2];
} HiprBvhNode;

/* Compressed 4-wide BVH node, 64 bytes: what the persistent traversal kernels walk in scenes with more than 64 BVH2 nodes.
 * (The traversal is bound by the number of 16-byte gathers it issues, not by arithmetic: one of these replaces ~2.1 BVH2
 * nodes of 64 bytes each.) Built by collapsing the BVH2 (host/BvhBuilder.cpp); child boxes are quantised to 8 bits per bound
 * relative to the node's own box, conservatively (decoded boxes contain the exact ones):
 *   lo_a[k] = origin[a] + qlo_a[k] * 2^(exponent_a - 127),  hi_a[k] = origin[a] + qhi_a[k] * 2^(exponent_a - 127)
 * exponents = ex | ey << 8 | ez << 16 (biased like an IEEE exponent field); byte k of qlo/qhi word a = child k.
 * child[k]: >= 0 inner wide node, < 0 leaf (same encoding as HiprBvhNode), HIPR_WIDE_EMPTY = unused slot. */
typedef struct HiprWideNode {
    float origin[3];
    uint32_t exponents;
    uint32_t qlo[3];
    uint32_t qhi[3];
    uint32_t _pad[2];
    int32_t child[4];
} HiprWideNode;
#define HIPR_WIDE_EMPTY 0x7FFFFFFF

/* 8-wide compressed BVH ("wide8"): what the persistent traversal kernels walk (round 3). Measured on the MI355X, the traversal is bound by the
 * number of 16-byte lane-loads the CU's address / tag pipeline takes (82 % busy with the 4-wide tree) and by the length of a ray's chain of
 * dependent fetches, so the tree is built to need few of both: ONE array of 64-byte SLOTS holds inner nodes and leaf records alike, the children of
 * a node sit in consecutive slots (one base index serves all eight), an inner node carries the 8-bit quantised boxes of up to EIGHT children in
 * four 16-byte loads, and a leaf is one record of one or two triangles sharing an edge in four loads (two triangles used to be six).
 * Node origin: three 21-bit coordinates on a grid over the scene's bounds, origin_a = fma(float(m_a), grid_cell[a], grid_min[a]); child box of
 * position s on axis a: [origin_a + qlo[a][s] * 2^(exponent[a] - 127), origin_a + qhi[a][s] * 2^(exponent[a] - 127)], containing the exact box.
 * Positions are assigned so that position bit a set means "on the + side of the node's centre along axis a": a ray visits the hit children in
 * ascending order of (position XOR the ray's octant bits, bit a = direction[a] < 0) -- near to far without sorting distances. */
typedef struct HiprNode8 {
    uint32_t origin[2];     /* x: bits 0..20, y: bits 21..41, z: bits 42..62 of the 64-bit value */
    uint8_t exponent[3];    /* biased like an IEEE exponent field */
    uint8_t inner_mask;     /* bit s: the child in position s is an inner node, else a leaf record */
    uint32_t base_valid;    /* bits 0..23: slot of the node's first child; bits 24..31: bit s = position s holds a child. The child in position s
                               lives in slot base + popcount(valid & ((1 << s) - 1)) */
    uint8_t qlo[3][8];      /* [axis][position]; an empty position holds qlo = 255, qhi = 0 */
    uint8_t qhi[3][8];
} HiprNode8;

/* Leaf record of the wide8 tree: triangle A = (a, a + e1, a + e2) and, when triangle[1] != HIPR_LEAF8_NONE, triangle B = (a, a + e2, a + e3): two
 * triangles of HiprSceneDesc::triangles that share the edge (a, a + e2). Both are tested with the ray / triangle solve of DESIGN.md on the stored
 * corner and edges (the edges rounded once, at build time), A first. The solve of a record triangle yields the weights (w, u, v) of its corners in
 * record order; `selectors` says which of them are the weights of the scene triangle's vertices 1 and 2, i.e. the (u, v) a hit reports. */
typedef struct HiprLeaf8 {
    float a[3], e1[3], e2[3], e3[3];
    uint32_t triangle[2];   /* indices into HiprSceneDesc::triangles */
    uint32_t flags;         /* bit 0 / bit 1: A / B is HIPR_TRIANGLE_OPAQUE; bit 2 / bit 3: A / B is HIPR_TRIANGLE_ONE_SIDED; bit 4: the scene triangle B is wound
                               against the record's (a, a + e2, a + e3) -- A never is --; bits 8..9, 10..11: which of (w, u, v) = 0, 1, 2 is A's reported u, v;
                               bits 12..13, 14..15: B's */
    float facing_margin;    /* a closest hit on a one-sided record triangle is stepped over when the solve's determinant, signed by the scene triangle's
                               winding, is below -facing_margin: the ray arrives from behind by more than any rounding of this test or of the hit program's
                               own (normalised geometric normal . direction < 0) could turn around. 2^-13 (|e1|^2 + |e2|^2 + |e3|^2) for unit directions. */
} HiprLeaf8;
#define HIPR_LEAF8_NONE 0xFFFFFFFFu
typedef union HiprSlot8 { HiprNode8 node; HiprLeaf8 leaf; uint32_t words[16]; } HiprSlot8;

/* Software replacement for the reference's texture samplers (OR/Renderer.cpp:703-751).
 * Texels live in HiprSceneDesc::texels at `texel_offset` (bytes). */
typedef struct HiprTexture {
    uint32_t width, height;
    uint64_t texel_offset; /* 64 bit: a Sponza-class set of 4K maps exceeds 4 GiB once expanded to RGBA */
    uint8_t format;        /* HIPR_TEXEL_* */
    uint8_t wrap_u, wrap_v;/* 0 clamp, 1 repeat (BF/Assets/Texture.h:21-35) */
    uint8_t filter;        /* bit0: linear magnification, bit1: linear minification */
    uint8_t is_sRGB;       /* RT_TEXTURE_READ_NORMALIZED_FLOAT_SRGB (OR/Renderer.cpp:736-739) */
    uint8_t _pad[3];
} HiprTexture;

enum { HIPR_TEXEL_R8 = 1, HIPR_TEXEL_RGBA8 = 4, HIPR_TEXEL_R32F = 17, HIPR_TEXEL_RGBA32F = 20 };

/* OR/Types.h:265-272 LightSample: what sampling a light returns. The environment light is PRE-sampled on the host. */
typedef struct HiprLightSample {
    float radiance[3];
    float PDF;
    float direction_to_light[3];
    float distance;
} HiprLightSample;

/* Importance sampled latitude-longitude environment map (PresampledEnvironmentLight, OR/Types.h:270-277, built by
 * OR/PresampledEnvironmentMap.cpp:19-101): the image is HiprSceneDesc::textures[environment_map_ID] (RGBA8 or RGBA32F);
 * `per_pixel_PDF` is the solid angle PDF of every PDF texel without its 1 / sin(theta) factor (nearest lookup, clamp);
 * `samples` are sample_count (a power of two >= 2) light samples drawn on the host from progressive multi-jittered points.
 * The environment takes part in next event estimation through a light of type HIPR_LIGHT_PRESAMPLED_ENVIRONMENT in `lights`
 * (the host appends it, OR/Renderer.cpp:1160-1196); its radiance is scaled by HiprSceneState::environment_tint. */
typedef struct HiprEnvironment {
    int32_t environment_map_ID;
    uint32_t pdf_width, pdf_height;
    const float* per_pixel_PDF;
    const HiprLightSample* samples;
    uint32_t sample_count;
} HiprEnvironment;

/* The flat scene the host produces in handle_updates() (OR/Renderer.cpp:578-1205). */
typedef struct HiprSceneDesc {
    const HiprBvhNode* nodes;            uint32_t node_count;
    const HiprTriangle* triangles;       uint32_t triangle_count;
    const HiprInstance* instances;       uint32_t instance_count;
    const uint32_t* indices;             uint32_t index_count;      /* uint3 per primitive, count in uints */
    const HiprVertexGeometry* geometry;  uint32_t vertex_count;
    const float* texcoords;              /* float2 per vertex or NULL */
    const uint32_t* tints;               /* uchar4 (tint rgb, roughness) per vertex or NULL */
    const float* emissions;              /* float3 per vertex or NULL */
    const HiprMaterial* materials;       uint32_t material_count;   /* slot 0 = invalid material */
    const HiprLight* lights;             uint32_t light_count;
    const HiprTexture* textures;         uint32_t texture_count;    /* slot 0 = none */
    const uint8_t* texels;               uint64_t texel_bytes;
    uint32_t bvh_max_depth;              /* deepest leaf, root = 1; selects the LDS stack size */
    const HiprWideNode* wide_nodes;      uint32_t wide_node_count;  /* the same tree collapsed to 4-wide nodes; may be NULL / 0 */
    uint32_t wide_stack_entries;         /* most entries a traversal of wide_nodes can have on its stack */
    const HiprEnvironment* environment;  /* NULL: the environment is the constant HiprSceneState::environment_tint */
    const HiprSlot8* wide8_slots;        uint32_t wide8_slot_count; /* the 8-wide tree over the same triangles, slot 0 = the root node; may be NULL / 0 */
    uint32_t wide8_height;               /* nodes on the longest root-to-leaf chain = most entries a traversal can have on its stack */
    float wide8_grid_min[3], wide8_grid_cell[3];
} HiprSceneDesc;

/* OR/Types.h:507-523 SceneStateGPU, without OptiX buffer ids. */
typedef struct HiprSceneState {
    float environment_tint[3];
    int32_t next_event_sample_count;   /* default 3 (OR/Renderer.cpp:479), clamped to 256 (:1390-1392) */
} HiprSceneState;

/* OR/Types.h:486-501 CameraStateGPU, matrices row-major as Matrix4x4f::begin(). */
typedef struct HiprCameraState {
    float view_to_world_rotation[9];
    float inverse_projection_matrix[16];
    float inverse_view_projection_matrix[16];
    uint32_t accumulations;
    uint32_t max_bounce_count;
    /* PathRegularizationSettings (OR/PublicTypes.h:38-45). The scale applied to the paths of accumulation a is
     * PDF_scale * (1.0f + scale_decay * float(a)), PublicTypes.h:44 PDF_scale_at_accumulation: the reference evaluates it on the
     * host once per launch (OR/Renderer.cpp:1244); a pass here may carry several accumulations, so the kernel evaluates it per path. */
    float path_regularization_PDF_scale;
    float path_regularization_scale_decay;
} HiprCameraState;

/* Precomputed tables uploaded at init (OR/Renderer.cpp:380-467). Float inputs are quantised to
 * unorm16 by the library exactly as the reference (`unsigned short(v * 65535 + 0.5f)`). */
typedef struct HiprTables {
    const float* ggx_with_fresnel_rho;  /* 32x32, F0 = 0, "base" */
    const float* ggx_rho;               /* 32x32, F0 = 1, "full" */
    const float* dielectric_light_rho;  /* 16x16x16 float2 (total, reflected), ior in [0.331492, 0.789474] */
    const float* dielectric_dense_rho;  /* 16x16x16 float2, ior in [1.26667, 3.01667] */
    const float* ggx_alpha_from_max_PDF;/* 32x32, x = encoded PDF, y = cos_theta */
} HiprTables;

/* Which pixels this context renders. The framebuffer is cut into 8x8 pixel tiles (one
 * wavefront of camera rays each), numbered row-major; the context owns tiles with
 * tile_id % tile_stride == tile_phase. tile_stride = 1 is the single GPU case. */
typedef struct HiprFrameDesc {
    uint32_t width, height;
    uint32_t tile_phase, tile_stride;
    uint32_t samples_per_pass;   /* accumulations traced per hipr_render_pass, >= 1 */
} HiprFrameDesc;

/* Ray / traversal counters accumulated since hipr_reset_counters(). */
typedef struct HiprCounters {
    uint64_t camera_rays;        /* P: pixel-samples generated */
    uint64_t closest_rays;       /* R_mc: closest-hit traces incl. retraces */
    uint64_t shadow_rays;        /* R_sh */
    uint64_t shaded_hits;        /* H: accepted surface hits */
    uint64_t closest_nodes;      /* N_mc (only when instrumented counting is enabled) */
    uint64_t closest_triangles;  /* T_mc */
    uint64_t shadow_nodes;       /* N_sh */
    uint64_t shadow_triangles;   /* T_sh */
    uint64_t iterations;         /* trace/shade rounds of the wavefront loop */
} HiprCounters;

/* Per-kernel device time of the passes since hipr_reset_timers(), measured with HIP events
 * on the context's stream. Index with HIPR_KERNEL_*. */
enum { HIPR_KERNEL_GENERATE = 0, HIPR_KERNEL_TRACE_CLOSEST = 1, HIPR_KERNEL_SHADE = 2,
       HIPR_KERNEL_TRACE_SHADOW = 3, HIPR_KERNEL_ACCUMULATE = 4, HIPR_KERNEL_COUNT = 5 };
typedef struct HiprKernelTimes {
    double milliseconds[HIPR_KERNEL_COUNT];
    uint64_t launches[HIPR_KERNEL_COUNT];
} HiprKernelTimes;

typedef struct HiprContext HiprContext;

/* ------------------------------------------------------------------------------------------- */
/* Lifetime: Renderer::initialize / ~Renderer (OR/Renderer.cpp:273-574, 1365-1387)             */
/* ------------------------------------------------------------------------------------------- */
int hipr_create(int device_id, HiprContext** out_context);
int hipr_destroy(HiprContext* context);
const char* hipr_last_error(void);
/* Number of HIP devices visible; 0 mirrors Context::getDeviceCount() == 0 (OR/Renderer.cpp:280). */
int hipr_device_count(void);

/* Use an externally owned hipStream_t (e.g. torch's current stream); NULL = the context's own. */
int hipr_set_stream(HiprContext* context, void* hip_stream);

/* ------------------------------------------------------------------------------------------- */
/* Uploads: the tables of OR/Renderer.cpp:380-467 and the scene of handle_updates :578-1205     */
/* ------------------------------------------------------------------------------------------- */
int hipr_upload_tables(HiprContext* context, const HiprTables* tables);
/* Every refusal -- the checks of hipr_validate_scene, then HIPR_ERROR_UNSUPPORTED for what the kernels cannot serve: a BVH2 deeper than 64, a wide BVH that
 * needs more stack than the traversal kernels have, an environment map that is not RGBA -- comes before the device is touched and leaves the resident scene as
 * it was. The same holds for hipr_update_scene_geometry and hipr_refit_scene_transforms. A call of the three that fails AFTER that (out of memory, a HIP error)
 * leaves no scene: rendering returns HIPR_ERROR_NOT_READY until a hipr_upload_scene succeeds. */
int hipr_upload_scene(HiprContext* context, const HiprSceneDesc* scene);
/* The host-side checks hipr_upload_scene runs before anything reaches the device, on their own (no context, no GPU): every index
 * the kernels follow -- material texture IDs, instance material / pool offsets, triangle instance / primitive / vertex indices,
 * texture extents inside the texel pool, BVH2, wide BVH and 8-wide tree child and leaf ranges -- must be in range; an attribute an
 * instance flags (HIPR_MESH_TEXCOORDS / TINTS / EMISSIVE) must have its pool; an environment description must be complete (a map among
 * the textures, the per-pixel PDF with its extents, the samples with their count). HIPR_ERROR_INVALID_ARGUMENT and a message in
 * hipr_last_error() otherwise. (OptiX validates its node graph in rtContextValidate; this is the counterpart.) */
int hipr_validate_scene(const HiprSceneDesc* scene);
/* Transform-only update: the same scene after its host refitted the BVH to moved instances (the reference refits its root acceleration
 * structure when a node moves, OR/Renderer.cpp:472,1010-1041). Re-uploads nodes, wide nodes, triangles, instances and lights, whose
 * counts and tree topology must equal the uploaded scene's, and rebuilds the per-triangle records derived from them; meshes,
 * materials, textures, environment and tables stay as uploaded. */
int hipr_update_scene_geometry(HiprContext* context, const HiprSceneDesc* scene);
/* The same transform-only update WITHOUT the host refit and the re-upload (OR/Renderer.cpp:472,1010-1041: OptiX refits the root acceleration on the device too):
 * the instances named in `moved` get new object-to-world matrices, and kernels recompute their world-space triangles from the resident object-space pools,
 * rebuild the leaf records of the 8-wide tree, requantise its nodes level by level and rebuild the per-triangle records -- bit for bit what
 * SceneBuilder::update_model_transforms + hipr_update_scene_geometry leave in those arrays (csrc/wide8_refit.h). `lights`: NULL keeps the lights, else
 * `light_count` lights replace the uploaded ones one for one. Checked before anything on the device is touched:
 *   HIPR_ERROR_UNSUPPORTED        the uploaded scene brings no 8-wide tree (at most 64 BVH2 nodes); OR the search the context walks is another one (a tree too
 *                                 high for the 8-wide kernels, a variant forced with hipr_set_trace_variant): the arrays that search reads are the ones this call
 *                                 leaves stale; OR the scene carries the exhaustive search's items, which only the host builds; OR it has more than 0x55555555
 *                                 triangles (the corner ordinal 3 t + k that decides ties among equal bounds is 32 bits wide);
 *   HIPR_ERROR_INVALID_ARGUMENT   an instance index out of range; a matrix with an entry that is not finite (the scene's bounds and with them the grid would not
 *                                 be); a matrix whose handedness differs from the uploaded instance's (a mirrored instance has index triples of its own, which
 *                                 the host path provides); a light count other than the uploaded one; a light that changes its type.
 * Afterwards the BVH2 and 4-wide arrays on the device are stale: hipr_set_trace_variant to HIPR_TRACE_BVH2 / HIPR_TRACE_WIDE_PERSISTENT returns
 * HIPR_ERROR_UNSUPPORTED until the next hipr_upload_scene or hipr_update_scene_geometry. */
typedef struct HiprInstanceTransform { uint32_t instance_index; float object_to_world[12]; } HiprInstanceTransform;
typedef struct HiprRefitResult {
    int32_t needs_rebuild;        /* 1: a leaf record could not be refitted (two object-space vertices that shared a world position at build time parted); the
                                     context's scene is no longer usable until hipr_upload_scene */
    double  child_half_area;      /* sum over all child boxes of all 8-wide nodes after the refit (exact boxes; per box in f32, summed in f64 in a fixed shape) */
    double  uploaded_half_area;   /* the same sum, taken by the same kernels when the scene was uploaded */
    float   grid_min[3], grid_cell[3];      /* the 8-wide tree's grid over the moved scene's bounds (HiprSceneDesc::wide8_grid_*) */
} HiprRefitResult;
int hipr_refit_scene_transforms(HiprContext* context, const HiprInstanceTransform* moved, uint32_t moved_count,
                                const HiprLight* lights /* NULL: keep */, uint32_t light_count, HiprRefitResult* out);
/* Material edits WITHOUT a new upload (the reference rewrites one slot of its material buffer, OR/Renderer.cpp:753-850): `materials` rewrites slots of the
 * uploaded material pool, `assignments` gives uploaded instances another material of that pool. The changed slots and words are copied into the resident pools,
 * and two short passes bring along everything an upload derives from materials -- HiprTriangle::flags of the touched instances' triangles (the flag rules of
 * csrc/material_rules.h, which the host's scene builder runs too), their copies in the trace records, the material index in the shading records, the
 * coat class of the listing pass, bits 0..3 of the 8-wide tree's leaf records -- and the kernel instantiations the context picks by what the pools hold:
 * afterwards the device holds, byte for byte, what hipr_upload_scene of the edited description would put there (csrc/material_update.h). No tree is touched:
 * a material moves no box. Checked before anything on the device is touched:
 *   HIPR_ERROR_NOT_READY          no scene is uploaded;
 *   HIPR_ERROR_INVALID_ARGUMENT   a null array with a non-zero count; a material or instance index outside the uploaded pools; a new material index outside
 *                                 the material pool; a material hipr_validate_scene would refuse (a texture ID outside the uploaded textures, an unknown
 *                                 shading model);
 *   HIPR_ERROR_UNSUPPORTED        the scene carries the exhaustive search's items (at most 64 triangles), which pair triangles of equal flags: there a
 *                                 material edit changes a topology. Upload the scene instead; it costs nothing at that size. */
typedef struct HiprMaterialUpdate   { uint32_t material_index; HiprMaterial material; } HiprMaterialUpdate;
typedef struct HiprInstanceMaterial { uint32_t instance_index; int32_t material_index; } HiprInstanceMaterial;
int hipr_update_scene_materials(HiprContext* context, const HiprMaterialUpdate* materials, uint32_t material_count,
                                const HiprInstanceMaterial* assignments, uint32_t assignment_count);
/* The binned-SAH BVH2 of a triangle set built on the device (the reference asks OptiX for a "Trbvh" build, which runs on the GPU, OR/Renderer.cpp:161-182,471-476):
 * byte for byte the nodes, triangle order and deepest leaf the host builder produces (csrc/bvh2_build.h), for the 4-wide and 8-wide collapses to go on from.
 * Inputs and outputs are host pointers; `node_capacity` of max(count, 1) - 1, or 1, always suffices; max_depth below 8 is taken as 8, as the host builder does.
 * The call owns its device scratch (about 240 B per triangle; up to 128 MiB it is kept with the context and reused, more is freed when the call returns), leaves the resident scene untouched and needs none. Checked before the device is touched:
 *   HIPR_ERROR_INVALID_ARGUMENT   a null pointer, no triangles, too little room for the nodes, a corner that is not finite.
 * A build that meets a range which takes the median path (the depth budget, or coincident centroids) and is longer than one lane sorts DECLINES: it returns
 * HIPR_ERROR_UNSUPPORTED, writes nothing to the outputs and names the range in hipr_last_error(); the host builder serves such a set. */
int hipr_build_bvh2(HiprContext* context, const HiprTriangle* triangles, uint32_t count, uint32_t max_depth,
                    HiprBvhNode* out_nodes, uint32_t node_capacity, uint32_t* out_node_count,
                    uint32_t* out_order /* count words */, uint32_t* out_deepest);
/* The 8-wide tree of a BVH2 collapsed on the device (the reference asks OptiX for a "Trbvh" build, which runs on the GPU, OR/Renderer.cpp:161-182,471-476): byte for
 * byte the slots, height, grid and counters of the host's collapse in its default configuration (csrc/wide8_build.h). `triangles` and `order` (may be NULL:
 * triangles[k]) are the scene's triangles and the order the BVH2's leaves reference them in, element k = triangles[order[k]]; all pointers are host pointers.
 * The call runs on the context's stream, owns its device scratch (kept with the context up to 128 MiB, freed when the call returns beyond that), leaves the
 * resident scene untouched and needs none. Checked on the host, by one pass over the indices, before the device is touched:
 *   HIPR_ERROR_INVALID_ARGUMENT   a null pointer, no nodes or triangles; an order entry, a child index or a leaf range out of bounds; a node referenced twice;
 *                                 more than 64 levels of nodes; `slot_capacity` below the slots the tree needs (known before a slot is written); a triangle
 *                                 corner or a child box that is not finite (found by the first passes on the device, which read them anyway).
 *   HIPR_ERROR_UNSUPPORTED        the tree needs more than 0xFFFFFF slots (the host returns an empty tree there too); or the leaves are not met in ascending
 *                                 order of their first triangle, which every BVH2 of this library is: the host collapses such a tree.
 * Every refusal leaves `out_slots` and `out` untouched. */
typedef struct HiprWide8BuildResult {
    uint32_t slot_count, height;
    float grid_min[3], grid_cell[3];
    uint32_t node_count, leaf_count, paired_leaves;
} HiprWide8BuildResult;
int hipr_build_wide8(HiprContext* context, const HiprBvhNode* nodes, uint32_t node_count, const HiprTriangle* triangles, const uint32_t* order /* may be NULL */,
                     uint32_t triangle_count, HiprSlot8* out_slots, uint32_t slot_capacity, HiprWide8BuildResult* out);
/* The compressed 4-wide tree of a BVH2 (HiprWideNode) collapsed on the device (the reference asks OptiX for a "Trbvh" build, which runs on the GPU,
 * OR/Renderer.cpp:161-182,471-476): byte for byte the nodes, node count and stack entries of the host's collapse (host/BvhBuilder.cpp; csrc/wide4_build.h), which
 * are what HiprSceneDesc::wide_nodes, wide_node_count and wide_stack_entries take. The collapse reads no triangle: `triangle_count` bounds the leaf ranges. All
 * pointers are host pointers; a `node_capacity` of `node_count` always suffices, because every wide node is rooted at a distinct BVH2 node. The call runs on the
 * context's stream, owns its device scratch (about 220 B per BVH2 node; kept with the context up to 128 MiB, freed when the call returns beyond that), leaves the
 * resident scene untouched and needs none. Checked on the host, by one pass over the indices, before the device is touched:
 *   HIPR_ERROR_INVALID_ARGUMENT   a null pointer or no nodes; a child index or a leaf range out of bounds; a node referenced twice; more than 64 levels of nodes.
 *   HIPR_ERROR_UNSUPPORTED        more nodes than a leaf reference addresses (2^28), as hipr_build_wide8.
 * Found on the device, before a node is written:
 *   HIPR_ERROR_INVALID_ARGUMENT   a child box that is not finite (the first pass reads every box anyway); `node_capacity` below the nodes the tree needs.
 * Every refusal leaves `out_nodes` and `out` untouched. */
typedef struct HiprWide4BuildResult { uint32_t node_count, stack_entries; } HiprWide4BuildResult;
int hipr_build_wide4(HiprContext* context, const HiprBvhNode* nodes, uint32_t node_count, uint32_t triangle_count, HiprWideNode* out_nodes, uint32_t node_capacity,
                     HiprWide4BuildResult* out);
/* The trees of the RESIDENT scene rebuilt on the device, in place, from the triangles it holds (the reference asks OptiX for a "Trbvh" build, which runs on the GPU
 * over the geometry the device holds, OR/Renderer.cpp:161-182,471-476; a moved node marks the acceleration dirty and the next launch rebuilds it on the device,
 * OR/Renderer.cpp:472,1010-1041): what a model that was dragged far asks for -- hipr_refit_scene_transforms reports child_half_area past 1.5 x uploaded_half_area, or
 * needs_rebuild -- without a flatten on the host and without an upload. No pool has changed, and after the refit the device holds the host's world-space triangles
 * byte for byte; kernels put them into the order the scene builder flattens in (instances in order, primitives in order), build the BVH2 (csrc/bvh2_build.h),
 * collapse it (csrc/wide8_build.h) and install the result (csrc/scene_rebuild.h). Afterwards the device holds, byte for byte, what SceneBuilder::rebuild() followed
 * by hipr_upload_scene on a fresh context puts into the triangles, the BVH2 nodes, the 8-wide slots and everything derived from them; the 4-wide array is not
 * rebuilt, so the state hipr_refit_scene_transforms describes (hipr_set_trace_variant refuses the other searches) lasts until the next upload or geometry update; that
 * hipr_update_scene_geometry brings the NEW tree's 4-wide array, whose size and stack need it takes instead of comparing them with the uploaded ones.
 * Outputs are host pointers and may be NULL (not read back): `out_nodes` the BVH2, `out_order` triangle_count words -- out_order[k] is the position, in the
 * builder's flatten order, of the triangle that stands at place k afterwards (BvhBuildResult::order) -- `out_slots` the 8-wide tree. max_depth below 8 is taken as 8.
 * The call accepts a scene that is ready, and one whose last writer was a hipr_refit_scene_transforms that returned needs_rebuild (not ready, but whole).
 * Checked before the device is touched:
 *   HIPR_ERROR_NOT_READY          no scene, or a scene a failed call left behind;
 *   HIPR_ERROR_UNSUPPORTED        the conditions hipr_refit_scene_transforms refuses on: no 8-wide tree, another search, the exhaustive search's items;
 *   HIPR_ERROR_INVALID_ARGUMENT   a null `out`; a non-null `out_nodes` with room for fewer than max(count, 1) - 1 (or 1) nodes; a non-null `out_slots` with room
 *                                 for fewer than min(2 x triangle_count, 0xFFFFFF) slots -- what always suffices.
 * Found on the device, before anything resident is replaced, all HIPR_ERROR_UNSUPPORTED with the reason in hipr_last_error(): a decline of the BVH2 build (a
 * median range longer than a lane sorts, as hipr_build_bvh2); a new 8-wide tree higher than the kernels' stacks (33); more than 0xFFFFFF slots; two resident
 * triangles that claim one flatten position. Every refusal leaves the resident scene exactly as the call found it -- not ready included -- and the outputs
 * untouched. A HIP failure once the new arrays are being installed leaves no scene, as with the other writers. */
typedef struct HiprSceneRebuildResult {
    uint32_t node_count, deepest;        /* the BVH2, as hipr_build_bvh2 reports them */
    HiprWide8BuildResult wide8;          /* as hipr_build_wide8 reports it */
    double half_area;                    /* child_half_area of the new tree = the scene's new uploaded_half_area */
} HiprSceneRebuildResult;
int hipr_rebuild_scene_trees(HiprContext* context, uint32_t max_depth, HiprBvhNode* out_nodes /* may be NULL */, uint32_t node_capacity, uint32_t* out_order /* may be NULL */,
                             HiprSlot8* out_slots /* may be NULL */, uint32_t slot_capacity, HiprSceneRebuildResult* out);
/* Models of the RESIDENT scene added and removed on the device (the reference leaves geometry where it lives, adds or removes a child of its root group and marks
 * the acceleration dirty, OR/Renderer.cpp:138-182, :1043-1110): a model destroyed, or created over a mesh whose vertices and index triples the uploaded pools
 * already hold, changes no pool, so no flatten on the host and no upload is needed. `edits` is the NEW instance list, IN ORDER -- the scene builder flattens
 * instances in order and both tree builders depend on that order. An entry with `source` < the resident instance count keeps that resident instance, with the
 * matrix and the material the device holds (`instance` and `primitive_count` are ignored); an entry with `source` == HIPR_EDIT_NEW_INSTANCE brings `instance`, and
 * `primitive_count`, the triangles of its mesh (an instance does not carry its count). Appending, inserting, removing and any mix of them are this one list.
 * Kernels bring the kept triangles into the new list's flatten order and make the new instances' triangles there -- corners, flags and class byte by the scene
 * builder's own expressions over the resident pools (csrc/instance_edit.h) -- then the call goes on as hipr_rebuild_scene_trees does, over the new count, and
 * installs the new triangle and instance arrays with the trees. Afterwards the device holds, byte for byte, what SceneBuilder::remove_model / insert_model,
 * rebuild() and hipr_upload_scene on a fresh context put into the triangles, the instances, the BVH2 nodes, the 8-wide slots and everything derived from them;
 * the 4-wide array is left as hipr_rebuild_scene_trees leaves it. Outputs as hipr_rebuild_scene_trees'; `out_order` receives out->triangle_count words, and
 * `order_capacity` is the room it has. The call accepts the states hipr_rebuild_scene_trees accepts. Checked on the host before anything is written:
 *   HIPR_ERROR_NOT_READY          no scene, or a scene a failed call left behind;
 *   HIPR_ERROR_INVALID_ARGUMENT   a null `edits` or `out`; a `source` that is neither HIPR_EDIT_NEW_INSTANCE nor a resident instance; a resident instance named
 *                                 twice; a new instance whose (index_offset, primitive_count) or vertex_offset lies outside the uploaded index / vertex pools,
 *                                 whose material index lies outside the uploaded material pool or names a material hipr_validate_scene would refuse, which
 *                                 flags an attribute whose pool was not uploaded, or whose matrix is not finite;
 *   HIPR_ERROR_UNSUPPORTED        the conditions hipr_rebuild_scene_trees refuses on; an empty list.
 * Checked once the kept instances' triangles are counted (a kernel over the resident triangles that writes scratch only), before anything else runs:
 *   HIPR_ERROR_UNSUPPORTED        the new list yields no triangle, or more than a leaf reference holds (2^28);
 *   HIPR_ERROR_INVALID_ARGUMENT   a non-null output with less room than the NEW triangle count t asks for: max(t, 1) - 1 (or 1) nodes, t order words,
 *                                 min(2 t, 0xFFFFFF) slots.
 * Found on the device, in scratch, before anything resident is replaced, all HIPR_ERROR_UNSUPPORTED with the reason in hipr_last_error(): an index triple of a
 * new instance that points outside the vertex pool (the index is checked before the vertex is loaded: it is never read through); a flatten position claimed
 * twice or not at all; a decline of the BVH2 build; a BVH2 of at most 64 nodes (a fresh upload would choose another search and build other arrays); trees higher
 * than the kernels walk, or more than 0xFFFFFF slots. Every refusal leaves the resident scene exactly as the call found it -- not ready included -- and the
 * outputs untouched. A HIP failure once the new arrays are being installed leaves no scene, as with the other writers. */
#define HIPR_EDIT_NEW_INSTANCE 0xFFFFFFFFu
typedef struct HiprInstanceEdit {
    uint32_t source;                     /* a resident instance's index (kept), or HIPR_EDIT_NEW_INSTANCE */
    uint32_t primitive_count;            /* new instances: the triangles of the mesh */
    HiprInstance instance;               /* new instances */
} HiprInstanceEdit;
typedef struct HiprSceneEditResult {
    uint32_t triangle_count, instance_count;      /* of the resident scene afterwards */
    uint32_t node_count, deepest;        /* the BVH2, as hipr_build_bvh2 reports them */
    HiprWide8BuildResult wide8;          /* as hipr_build_wide8 reports it */
    uint32_t _pad;
    double half_area;                    /* child_half_area of the new tree = the scene's new uploaded_half_area */
} HiprSceneEditResult;
int hipr_edit_scene_instances(HiprContext* context, const HiprInstanceEdit* edits, uint32_t edit_count, uint32_t max_depth, HiprBvhNode* out_nodes /* may be NULL */,
                              uint32_t node_capacity, uint32_t* out_order /* may be NULL */, uint32_t order_capacity, HiprSlot8* out_slots /* may be NULL */,
                              uint32_t slot_capacity, HiprSceneEditResult* out);
/* The pools of the RESIDENT scene grown at their tails (the reference loads a mesh into buffers of its own, OR/Renderer.cpp:92-136 load_mesh, and a texture or a
 * material into its slot, :703-812 textures and upload_material, and leaves the rest of the scene where it lives): the step before hipr_edit_scene_instances when
 * a model is created over a mesh, a material or a texture the device does not hold yet. Every pool of a HiprSceneDesc that the scene builder makes is
 * append-only, so one description carries what is new in all of them:
 *   vertices     `vertex_count` records appended to `geometry`. The optional per-vertex pools (`texcoords` 2 floats, `tints` 1 word, `emissions` 3 floats per
 *                vertex) each come with the number of vertices their array covers: a pool the device HOLDS takes its tail, `vertex_count` entries, and that tail
 *                is mandatory; a pool the device does not hold stays absent (NULL, 0) or comes WHOLE, resident + `vertex_count` entries, exactly as the scene
 *                builder holds it -- what stands in it for the vertices of meshes without the attribute is the builder's business, not this header's;
 *   indices      an ordered list of segments, which together make the tail of the index pool. A segment with `mirrored_from` == HIPR_SEGMENT_FROM_HOST takes the
 *                next `index_count` words of `indices`; any other segment is a MIRROR: a copy of the `index_count / 3` triples from triple `mirrored_from` on of
 *                the pool AS IT STANDS WHEN THE SEGMENT IS REACHED -- earlier segments of the same call included -- with the second and third corner exchanged
 *                (the triples a mirroring instance is drawn from); it is made by a kernel (csrc/pool_growth.h) and transfers nothing. `index_count` of the
 *                description is the sum of the host segments;
 *   materials    `material_count` records appended to the material pool;
 *   textures     `texture_count` records appended to `textures`, `texel_bytes` bytes appended to `texels`; the records carry ABSOLUTE texel offsets.
 * Afterwards every pool holds, byte for byte, what SceneBuilder::add_mesh / add_material / add_texture, rebuild() and hipr_upload_scene on a fresh context put
 * there, and the switches derived from the pools are derived again. No tree, triangle or instance is touched: no instance references a tail yet. Index VALUES are
 * not checked here: hipr_edit_scene_instances checks every index of a new instance against the vertex pool -- the grown one -- before it loads the vertex. The call
 * accepts the states hipr_edit_scene_instances accepts (ready, or awaiting a rebuild after a refit) and leaves the state it found. Checked on the host before the
 * device is touched:
 *   HIPR_ERROR_NOT_READY          no scene, or a scene a failed call left behind;
 *   HIPR_ERROR_INVALID_ARGUMENT   a null description; a null array with a non-zero count; a segment whose `index_count` is no multiple of 3; host segments that do
 *                                 not add up to `index_count`; a mirror range outside the pool as it stands at that segment; a resident attribute pool without its
 *                                 tail, or an attribute array that is neither the tail nor the whole pool; a sum of counts that does not fit 32 bits (vertices,
 *                                 index words, materials, textures); a texture whose extent, format or texel_offset hipr_validate_scene would refuse against the
 *                                 GROWN texel pool; a material it would refuse against the GROWN texture count.
 *   HIPR_ERROR_UNSUPPORTED        segments for a scene whose uploaded index pool is not one of whole triples.
 * An empty description is HIPR_OK and changes nothing. A pool whose buffer has no room is allocated anew, all of them before anything is written: a failed
 * allocation is HIPR_ERROR_OUT_OF_MEMORY and leaves the scene as found. A HIP failure after that leaves no scene, as with the other writers. */
#define HIPR_SEGMENT_FROM_HOST 0xFFFFFFFFu
typedef struct HiprIndexSegment {
    uint32_t mirrored_from;              /* HIPR_SEGMENT_FROM_HOST, or the first triple of the range a mirror segment copies */
    uint32_t index_count;                /* index words of the segment: whole triples */
} HiprIndexSegment;
typedef struct HiprPoolGrowth {
    const HiprVertexGeometry* geometry;  /* vertex_count */
    const float* texcoords;              /* 2 x texcoord_vertices */
    const uint32_t* tints;               /* tint_vertices */
    const float* emissions;              /* 3 x emission_vertices */
    const uint32_t* indices;             /* index_count: the host segments' words, in order */
    const HiprIndexSegment* segments;    /* segment_count */
    const HiprMaterial* materials;       /* material_count */
    const HiprTexture* textures;         /* texture_count */
    const uint8_t* texels;               /* texel_bytes */
    uint64_t texel_bytes;
    uint32_t vertex_count, texcoord_vertices, tint_vertices, emission_vertices;
    uint32_t index_count, segment_count, material_count, texture_count;
} HiprPoolGrowth;
int hipr_append_scene_pools(HiprContext* context, const HiprPoolGrowth* growth);
/* The lights and the environment of the RESIDENT scene replaced on the device (the reference rewrites its light buffer in place, OR/Renderer.cpp:852-1008, and builds
 * its presampled environment without touching geometry, :1136-1196, OR/PresampledEnvironmentMap.cpp:19-101): a lamp added, removed or changed in kind, the sky set,
 * swapped or taken away move no triangle, no tree, no material and no texel, so no flatten on the host and no upload of any pool is needed. `lights` is the NEW light
 * list, any count and any types, WITHOUT the environment's light. `environment_action`: HIPR_ENVIRONMENT_KEEP leaves the resident environment, _REMOVE takes it away
 * (the environment is the constant tint again), _BUILD makes the per-texel PDF image and the presampled light samples of `build->environment_map_ID` -- a texture the
 * RESIDENT pool holds: hipr_append_scene_pools brings a new one first -- by kernels (csrc/environment_build.h) over the resident texels. The three arrays of
 * `build` carry what the host path evaluates through libm, so that the device evaluates no transcendental: the sine of every PDF row, the linear value of every
 * sRGB byte, the progressive multi-jittered draw points; what is left for the device is + - x /, comparisons and conversions in correctly rounded f32. The
 * direction and the solid angle PDF of each sample are finished on the host inside the call (std::sin / std::cos; sample_count x 32 bytes read back and uploaded).
 * The light of type HIPR_LIGHT_PRESAMPLED_ENVIRONMENT is appended last by the call itself, exactly when the environment resident afterwards has more than one sample
 * (SceneBuilder::set_environment's rule). An image whose integral is below 1e-5 gives presample_environment's disabled form: one PDF texel of 0, one sample with a
 * zero PDF, no light appended. Afterwards the light buffer, the environment's PDF and sample buffers, the environment fields and the light count the kernels take, and
 * the kernel instantiations picked from the pools are, byte for byte, what SceneBuilder::add_light, InfiniteAreaLight + presample_environment + set_environment,
 * rebuild() and hipr_upload_scene on a fresh context leave. `out_per_pixel_PDF` (`pdf_capacity` floats) and `out_samples` (`sample_capacity` records) receive what
 * a BUILD made, for the host's description to follow; `out` the extents as resident. The call accepts the states hipr_append_scene_pools accepts (ready, or awaiting a
 * rebuild after a refit) and leaves the state it found. Checked on the host before the device is touched, each leaving the scene as found:
 *   HIPR_ERROR_NOT_READY          no scene, or a scene a failed call left behind;
 *   HIPR_ERROR_INVALID_ARGUMENT   a null `out`; a null array with a non-zero count; a light of type HIPR_LIGHT_PRESAMPLED_ENVIRONMENT in `lights`; an action outside the
 *                                 enum; _BUILD without `build`, or `build` with another action; a texture index of 0 or outside the resident pool; `pdf_height` other
 *                                 than max(texture height, 128); no `srgb_decode` for an sRGB texture, or one for a linear texture; a sample count that is no power of
 *                                 two >= 2; a draw point outside [0, 1); a table value that is not finite; an output with less room than the build can need;
 *   HIPR_ERROR_UNSUPPORTED        a texture that is neither RGBA8 nor RGBA32F (as at upload); an sRGB texture of floats (a table of bytes cannot serve it); a PDF image
 *                                 of more than 2^30 texels.
 * Scratch (about three PDF images; kept with the context up to 128 MiB, freed when the call returns beyond that) and every new buffer are allocated before anything
 * resident is written: a failed allocation is HIPR_ERROR_OUT_OF_MEMORY and leaves the scene as found. A HIP failure after that leaves no scene, as with the other
 * writers. */
typedef struct HiprEnvironmentBuild {
    int32_t  environment_map_ID;   /* a texture of the RESIDENT pool, RGBA8 or RGBA32F */
    const float* row_sines;        /* pdf_height values: sin(pi (y + 0.5) / pdf_height) as the caller's libm gives them */
    uint32_t pdf_height;           /* must be max(texture height, 128) */
    const float* srgb_decode;      /* 256 values, linear value of byte b; NULL for a texture that is not sRGB */
    const float* draw_points;      /* 2 x sample_count, in the order the samples are stored (the caller has applied the bit reversal) */
    uint32_t sample_count;         /* a power of two >= 2 */
} HiprEnvironmentBuild;
enum { HIPR_ENVIRONMENT_KEEP = 0, HIPR_ENVIRONMENT_REMOVE = 1, HIPR_ENVIRONMENT_BUILD = 2 };
typedef struct HiprLightingResult {
    uint32_t pdf_width, pdf_height, sample_count;      /* the environment as resident afterwards; zeros without one */
    uint32_t importance_sampling_disabled;             /* 1: this call's build met an image integral below 1e-5 and left the disabled form */
    uint32_t light_count;                              /* as resident afterwards, the environment's light included */
    uint32_t switches;                                 /* the kernel instantiations derived from the pools afterwards: HIPR_SWITCH_* */
} HiprLightingResult;
enum { HIPR_SWITCH_TEXTURES = 1, HIPR_SWITCH_ENVIRONMENT = 2 };
int hipr_update_scene_lighting(HiprContext* context, const HiprLight* lights, uint32_t light_count,   /* WITHOUT the environment's light */
                               int environment_action, const HiprEnvironmentBuild* build,
                               float* out_per_pixel_PDF /* may be NULL */, uint64_t pdf_capacity,
                               HiprLightSample* out_samples /* may be NULL */, uint32_t sample_capacity,
                               HiprLightingResult* out);
/* Pixel edits of images the device already holds, applied to the RESIDENT scene on the device (csrc/texel_update.h; the reference asserts "Pixel update not
 * implemented yet", OR/Renderer.cpp:697-698): a painted mask, a video frame on a screen, another lace pattern on a banner move no triangle and no tree, so no
 * flatten on the host, no tree build and no upload of any pool is needed. Each edit is a rectangle of new texels of a texture of the RESIDENT pool, in the texture's
 * resident format (all four HIPR_TEXEL_* are served; RGB24 already expanded, as SceneBuilder::add_texture leaves it); the rectangles are applied in list order, so
 * where two overlap the later one wins. One thing an upload derives depends on texels and follows: HIPR_TRIANGLE_OPAQUE of the triangles whose material leaves the
 * decision to its coverage texture (csrc/material_rules.h covered_everywhere) is decided again for every triangle of the materials whose deciding coverage texture is
 * an edited one, with its copy in the trace records, bits 0..3 of the leaf records and the search instantiation that follows "all triangles opaque". Afterwards the texel pool, the
 * triangles, the trace records, the leaf records and the kernel instantiations the context picks are, byte for byte, what SceneBuilder::update_texels and
 * hipr_upload_scene on a fresh context leave. An empty list is HIPR_OK and changes nothing.
 * The environment is NOT rebuilt: when an edited texture is the resident environment's map, `environment_stale` is 1 and, until a
 * hipr_update_scene_lighting(..., HIPR_ENVIRONMENT_BUILD, ...) of that texture follows, the sky's radiance and the PDF image and samples it is importance sampled
 * with disagree -- images stay unbiased only where the old PDF is non-zero wherever the new sky is, and are noisier at best. HIPRenderer::Renderer never leaves that gap.
 * The call accepts the states hipr_append_scene_pools accepts (ready, or awaiting a rebuild after a refit) and leaves the state it found. Checked on the host before
 * the device is touched, each leaving the scene as found:
 *   HIPR_ERROR_NOT_READY          no scene, or a scene a failed call left behind;
 *   HIPR_ERROR_INVALID_ARGUMENT   a null `out`; null `edits` with a non-zero count; a null `texels`; a texture index of 0 or outside the resident pool; a rectangle
 *                                 with an extent of 0 or one that reaches outside the texture; a `row_pitch_bytes` below the bytes of a row of the rectangle;
 *   HIPR_ERROR_UNSUPPORTED        the scene carries the exhaustive search's items (at most 64 triangles), which pair triangles of equal flags, AND an edited texture
 *                                 is the coverage texture of a resident material: there a flag changes a topology, which only the host builds (as
 *                                 hipr_update_scene_materials). Edits of the other textures of such a scene are served.
 * Scratch (the packed rows, a word per instance) is allocated before anything resident is written: a failed allocation is HIPR_ERROR_OUT_OF_MEMORY and leaves the
 * scene as found. A HIP failure after that leaves no scene, as with the other writers. */
typedef struct HiprTexelEdit {
    uint32_t texture_index;          /* a texture of the RESIDENT pool, > 0 */
    uint32_t x, y, width, height;    /* the rectangle, inside the texture, no extent 0 */
    const void* texels;              /* host, in the texture's RESIDENT format */
    uint64_t row_pitch_bytes;        /* >= width * bytes per texel */
} HiprTexelEdit;
typedef struct HiprTexelUpdateResult {
    uint32_t candidate_triangles;    /* triangles whose coverage was decided again */
    uint32_t changed_triangles;      /* of those, how many changed HIPR_TRIANGLE_OPAQUE */
    uint32_t all_triangles_opaque;   /* as resident afterwards */
    uint32_t environment_stale;      /* 1: an edited texture is the resident environment's map; see above */
} HiprTexelUpdateResult;
int hipr_update_scene_texels(HiprContext* context, const HiprTexelEdit* edits, uint32_t edit_count, HiprTexelUpdateResult* out);
/* Vertex edits of meshes the device already holds, applied to the RESIDENT scene on the device (csrc/vertex_update.h): a skinned character, a cloth step, a sculpt
 * stroke, a scrolled texture coordinate or a repainted vertex tint moves no index triple and changes no topology, so no flatten on the host, no tree build and no
 * upload of any pool is needed. The reference cannot express the edit (Assets/Mesh.h knows meshes created and destroyed only). Each edit is a range of vertices of
 * the RESIDENT pools -- an instance's vertex_offset + the mesh's own index -- with new values for any of the four per-vertex attributes; the edits are applied in
 * list order, so where two overlap the later one wins. What an upload derives from vertex data follows:
 *   positions    the world-space corners of every triangle that reads an edited vertex (through its instance's own index triples: mirrored instances and meshes
 *                worn by several instances are served), the scene's bounds and the 8-wide tree's grid, every leaf record and the quantised boxes above it, the
 *                trace records and the shading records;
 *   normals      the shading records;
 *   texcoords    the shading records, and HIPR_TRIANGLE_OPAQUE of the triangles whose material leaves the decision to its coverage texture (csrc/material_rules.h
 *                covered_everywhere) with its copy in the trace records, bits 0..3 of the leaf records and the search instantiation that follows "all triangles
 *                opaque";
 *   tints        the shading records;
 *   emissions    nothing: they are read from the pool.
 * Afterwards the vertex pools, the triangles, the 8-wide tree, the trace and shading records, the grid, both half areas and the kernel instantiations the context
 * picks are, byte for byte, what SceneBuilder::update_vertices and hipr_upload_scene on a fresh context leave. An empty list is HIPR_OK and changes nothing.
 * When an edit carries geometry the BVH2 and the 4-wide arrays go stale exactly as after hipr_refit_scene_transforms, and `refit.needs_rebuild` = 1 (vertices that
 * shared a world position at build time parted) leaves the scene awaiting hipr_rebuild_scene_trees, exactly as there. HIPRenderer::Renderer does not take this path.
 * Checked on the host before the device is touched, each leaving the scene as found:
 *   HIPR_ERROR_NOT_READY          no scene, a scene a failed call left behind, or a scene awaiting a rebuild;
 *   HIPR_ERROR_INVALID_ARGUMENT   a null `out`; null `edits` with a non-zero count; an edit with `vertex_count` 0 or with all four pointers null; a range past the
 *                                 resident pool; an attribute pointer whose resident pool is absent; a position or a texcoord that is not finite;
 *   HIPR_ERROR_UNSUPPORTED        what hipr_refit_scene_transforms refuses: no 8-wide tree, another search walked, the exhaustive search's items, more than
 *                                 0x55555555 triangles.
 * Scratch (the packed staging buffer, a byte per pool vertex and kind of mark) is allocated before anything resident is written: a failed allocation is
 * HIPR_ERROR_OUT_OF_MEMORY and leaves the scene as found. A HIP failure after that leaves no scene, as with the other writers. */
typedef struct HiprVertexEdit {
    uint32_t first_vertex;                 /* index into the RESIDENT vertex pools (an instance's vertex_offset + the mesh's own index) */
    uint32_t vertex_count;                 /* > 0, first_vertex + vertex_count <= the resident vertex count */
    const HiprVertexGeometry* geometry;    /* vertex_count entries, or NULL: positions and normals stay */
    const float*    texcoords;             /* float2 each, or NULL */
    const uint32_t* tints;                 /* uchar4 each, or NULL */
    const float*    emissions;             /* float3 each, or NULL */
} HiprVertexEdit;
typedef struct HiprVertexUpdateResult {
    HiprRefitResult refit;                 /* as hipr_refit_scene_transforms fills it; areas and grid as resident afterwards also when no position changed */
    uint32_t moved_triangles;              /* triangles with a corner in an edited geometry range */
    uint32_t candidate_triangles, changed_triangles, all_triangles_opaque;   /* as HiprTexelUpdateResult */
} HiprVertexUpdateResult;
int hipr_update_scene_vertices(HiprContext* context, const HiprVertexEdit* edits, uint32_t edit_count, HiprVertexUpdateResult* out);
/* Skinned and morphed meshes of the RESIDENT scene posed on the device (csrc/vertex_pose.h). hipr_update_scene_vertices takes FINISHED vertices: an animated mesh
 * would be skinned, its normals encoded and 16 bytes per vertex copied across every frame. A rig keeps what does not change -- rest positions and normals, joint
 * indices and weights, morph-target deltas -- on the device; a pose is joint_count 3x4 matrices and target_count weights, and one kernel writes the posed vertices
 * into the geometry pool. The arithmetic is the fixed chain of csrc/vertex_pose.h (morph targets in index order, linear-blend skinning over four slots, normals
 * through the upper 3x3 -- not the inverse transpose -- normalised and encoded as add_mesh encodes them), the same text SceneBuilder::pose_rigs runs.
 *
 * hipr_set_scene_rigs REPLACES the resident rig set (count 0 removes all rigs); the device keeps its own copies of every array. A rig is a range of the RESIDENT
 * geometry pool, as in HiprVertexEdit. hipr_upload_scene drops the rigs (ranges are pool coordinates); hipr_update_scene_geometry, the refit, material, lighting,
 * texel, vertex and instance edits, hipr_append_scene_pools and hipr_rebuild_scene_trees keep them: none moves a pool vertex. Refused before anything is touched:
 *   HIPR_ERROR_NOT_READY          no scene, a scene a failed call left behind, or a scene awaiting a rebuild;
 *   HIPR_ERROR_INVALID_ARGUMENT   null `rigs` with a non-zero count; a rig with `vertex_count` 0, a range past the resident pool, neither joints nor targets, more than
 *                                 65536 joints or 256 targets, a null array where a count asks for data; two rigs whose ranges overlap; a joint index >= joint_count;
 *                                 a weight outside [0, 1] or not finite; a vertex whose four weights are all 0 while joint_count > 0; a rest position or a target
 *                                 delta that is not finite or above 2^30 in magnitude; a rest normal that is not finite or whose squared length is not finite and > 0.
 * The new set is allocated and copied before the old one is let go: HIPR_ERROR_OUT_OF_MEMORY leaves the old set bound. */
typedef struct HiprRigDesc {
    uint32_t first_vertex;                 /* index into the RESIDENT vertex pools */
    uint32_t vertex_count;                 /* > 0 */
    uint32_t joint_count;                  /* 0: no skin */
    uint32_t target_count;                 /* 0 .. 256 morph targets */
    const float*    rest_positions;        /* float3 per vertex */
    const float*    rest_normals;          /* float3 per vertex, or NULL: a mesh without HIPR_MESH_NORMALS, oct_normal stays {0, 0} */
    const uint16_t* joints;                /* 4 per vertex, each < joint_count (joint_count > 0) */
    const float*    weights;               /* 4 per vertex, each in [0, 1], not all 0 (joint_count > 0); a slot of weight 0 is skipped */
    const float*    target_positions;      /* target-major float3 deltas: target_count x vertex_count (target_count > 0) */
    const float*    target_normals;        /* the same for normals, or NULL */
} HiprRigDesc;
int hipr_set_scene_rigs(HiprContext* context, const HiprRigDesc* rigs, uint32_t count);
/* hipr_pose_scene_rigs poses bound rigs: ONE launch whatever the number of poses, then exactly what hipr_update_scene_vertices runs after an edit of geometry (the
 * moved triangles, the bounds and the grid, the refit of the 8-wide tree, the records; `out` is filled as there, candidate_triangles and changed_triangles are 0).
 * Afterwards the device holds, byte for byte, what SceneBuilder::pose_rigs and a fresh upload leave, and what hipr_update_scene_vertices leaves when it is given
 * SceneBuilder::posed_geometry. A posed vertex depends on the rest data and the pose alone, never on what the pool held. An empty list is HIPR_OK and reports what
 * is resident. `refit.needs_rebuild` = 1 leaves the scene awaiting hipr_rebuild_scene_trees, as there. Joint matrices map OBJECT space to OBJECT space: the caller
 * has multiplied in the inverse bind matrix and the mesh's inverse world transform. Refused before anything is touched:
 *   HIPR_ERROR_NOT_READY          as above;
 *   HIPR_ERROR_INVALID_ARGUMENT   a null `out`; null `poses` with a non-zero count; a rig index that is not bound; the same rig twice in one call; a null array that
 *                                 the rig needs; a matrix entry that is not finite or above 2^30 in magnitude; a target weight that is not finite or above 2^10 in
 *                                 magnitude (with these bounds no posed position can overflow: csrc/vertex_pose.h);
 *   HIPR_ERROR_UNSUPPORTED        what hipr_refit_scene_transforms refuses, as hipr_update_scene_vertices.
 * Scratch is allocated before anything resident is written: HIPR_ERROR_OUT_OF_MEMORY leaves the scene as found. */
typedef struct HiprRigPose {
    uint32_t rig;                          /* index into the bound rig set */
    uint32_t reserved;                     /* 0 */
    const float* joint_matrices;           /* joint_count x 12 floats, row-major 3x4 (joint_count > 0) */
    const float* target_weights;           /* target_count floats (target_count > 0); a weight of exactly 0 skips its target */
} HiprRigPose;
int hipr_pose_scene_rigs(HiprContext* context, const HiprRigPose* poses, uint32_t pose_count, HiprVertexUpdateResult* out);
int hipr_set_scene_state(HiprContext* context, const HiprSceneState* state);

/* Entry points, numbered like OR/Types.h:33-44. set_backend() of the host renderer maps Backend values onto them
 * (OR/Renderer.cpp:1417-1455). The two AI denoiser entries (1, 2) wrap NVIDIA's proprietary DL denoiser and are not
 * provided: hipr_set_entry_point returns HIPR_ERROR_UNSUPPORTED for them. */
enum { HIPR_ENTRY_PATH_TRACING = 0, HIPR_ENTRY_DEPTH = 3, HIPR_ENTRY_ALBEDO = 4, HIPR_ENTRY_TINT = 5, HIPR_ENTRY_ROUGHNESS = 6,
       HIPR_ENTRY_SHADING_NORMAL = 7, HIPR_ENTRY_PRIMITIVE_ID = 8,
       /* The feature image the reference accumulates next to the radiance for its denoiser (AIDenoiser::path_tracing_RPG, ORS/SimpleRGPs.cu:149-201): at the
        * first accepted surface hit DefaultShading::rho of the material whatever its shading model, at a light hit radiance / (1 + radiance), black on a miss. */
       HIPR_ENTRY_DENOISER_ALBEDO = 9 };
int hipr_set_entry_point(HiprContext* context, int entry);
/* request_auxiliary_buffers (OR/Renderer.cpp:1267-1358) renders AOVs into scratch buffers so the camera's accumulation
 * survives: enable != 0 redirects hipr_render_pass / hipr_read_accumulation to a scratch accumulation buffer. enable == 1 zeroes it;
 * enable == 2 keeps what it holds (a second running mean next to the camera's: the denoiser's albedo feature image). */
int hipr_use_scratch_accumulation(HiprContext* context, int enable);

/* (Re)allocates the f64 accumulation buffer and the wavefront queues for the owned tiles;
 * resets nothing else. Replaces accumulation_buffer->setSize (OR/Renderer.cpp:1215-1219). A bad description is refused with the frame
 * as it was; a failure after that (out of memory) leaves no frame: HIPR_ERROR_NOT_READY until a hipr_set_frame succeeds. */
int hipr_set_frame(HiprContext* context, const HiprFrameDesc* frame);
/* Number of pixels this context owns under the current frame description. */
int hipr_owned_pixel_count(HiprContext* context, uint32_t* out_count);

/* ------------------------------------------------------------------------------------------- */
/* Rendering: context->launch(entry, w, h) of OR/IBackend.h:37-39 / OR/Renderer.cpp:1250-1265   */
/* ------------------------------------------------------------------------------------------- */
/* Traces frame.samples_per_pass accumulations starting at camera->accumulations for every owned
 * pixel, folds them into the f64 running mean (ORS/SimpleRGPs.cu:74-107) and writes half4 pixels.
 * out_half4_device:
 *   tile_stride == 1 : full frame, pixel (x, y) at out[x + y * out_pitch_pixels]  (ORS/SimpleRGPs.cu:106)
 *   tile_stride  > 1 : compact, owned pixel k at out[k] in owned-tile-major order (see hipr_scatter_tiles)
 * May be NULL to skip the half4 output. Asynchronous on the context stream unless `synchronize`. */
int hipr_render_pass(HiprContext* context, const HiprCameraState* camera,
                     void* out_half4_device, uint32_t out_pitch_pixels, int synchronize);

/* hipr_render_pass in its two halves, for hosts that show a progressive image one accumulation at a time (the reference's
 * render() contract, OR/Renderer.cpp:1250-1265) without giving up batched tracing:
 *   hipr_trace_pass           traces frame.samples_per_pass accumulations starting at camera->accumulations and leaves the radiance
 *                             of every sample in the pass's per-sample buffer; the running mean is not touched;
 *   hipr_accumulate_samples   folds samples [first_sample, first_sample + sample_count) of the traced pass into the f64 running mean
 *                             as accumulations first_accumulation, first_accumulation + 1, ... and writes the half4 pixels.
 * Tracing 32 accumulations in one pass and folding them one per frame gives, frame by frame, the bits that 32 one-accumulation
 * passes give (ORS/SimpleRGPs.cu:74-107 is applied per sample either way), at the throughput of the batched pass.
 * hipr_set_samples_per_pass changes the batch size of the current frame without resetting the accumulation (queues only grow). */
int hipr_set_samples_per_pass(HiprContext* context, uint32_t samples_per_pass);
int hipr_trace_pass(HiprContext* context, const HiprCameraState* camera);
int hipr_accumulate_samples(HiprContext* context, uint32_t first_sample, uint32_t sample_count, uint32_t first_accumulation,
                            void* out_half4_device, uint32_t out_pitch_pixels, int synchronize);

/* Copies the f64 accumulation (double4 per owned pixel, compact owned-tile-major order or full
 * frame row-major when tile_stride == 1) to host memory. Blocking. */
int hipr_read_accumulation(HiprContext* context, double* out_rgba, uint64_t capacity_pixels);
/* Scatter `rank_count` compact half4 buffers (as gathered over RCCL, rank r at
 * compact_device + r * pixels_per_rank_stride) into a full frame. Runs on the context stream. */
int hipr_scatter_tiles(HiprContext* context, const void* compact_half4_device, uint64_t pixels_per_rank_stride,
                       uint32_t rank_count, uint32_t width, uint32_t height,
                       void* out_half4_device, uint32_t out_pitch_pixels);

/* ------------------------------------------------------------------------------------------- */
/* Device groups: one frame on several GPUs of a node, from one process.          */
/* The reference is single device (OR/Renderer.cpp:289-291; interop is disabled above one        */
/* device, DX11OptiXAdaptor/Adaptor.cpp:83-90), so these have no counterpart there: they are the  */
/* same calls as above, fanned out over one HiprContext per device, plus the one exchange the    */
/* partition needs. Member i owns the 8x8 tiles with tile % size == i (scene and tables          */
/* replicated, f64 accumulation kept per member: no collective per sample); a frame is assembled */
/* on member 0's device by gathering the members' compact half4 tiles (RCCL send / recv over      */
/* xGMI, or peer-to-peer copies when RCCL is absent or members share a device) and               */
/* hipr_scatter_tiles. The image is bit-identical to the single-device one. A group of one       */
/* device forwards every call to its context.                                                    */
/* ------------------------------------------------------------------------------------------- */
typedef struct HiprGroup HiprGroup;
int hipr_group_create(const int* device_ids, uint32_t count, HiprGroup** out_group);
int hipr_group_destroy(HiprGroup* group);
uint32_t hipr_group_size(HiprGroup* group);
HiprContext* hipr_group_context(HiprGroup* group, uint32_t member);
const char* hipr_group_gather_description(HiprGroup* group);   /* which transport the gather uses (and that it fell back, after an exchange that stalled) */
int hipr_group_upload_tables(HiprGroup* group, const HiprTables* tables);
int hipr_group_upload_scene(HiprGroup* group, const HiprSceneDesc* scene);
int hipr_group_update_scene_geometry(HiprGroup* group, const HiprSceneDesc* scene);
int hipr_group_refit_scene_transforms(HiprGroup* group, const HiprInstanceTransform* moved, uint32_t moved_count,
                                      const HiprLight* lights, uint32_t light_count, HiprRefitResult* out);   /* every member; their results must agree */
int hipr_group_build_bvh2(HiprGroup* group, const HiprTriangle* triangles, uint32_t count, uint32_t max_depth, HiprBvhNode* out_nodes, uint32_t node_capacity,
                          uint32_t* out_node_count, uint32_t* out_order, uint32_t* out_deepest);   /* builds on member 0 */
int hipr_group_build_wide8(HiprGroup* group, const HiprBvhNode* nodes, uint32_t node_count, const HiprTriangle* triangles, const uint32_t* order, uint32_t triangle_count,
                           HiprSlot8* out_slots, uint32_t slot_capacity, HiprWide8BuildResult* out);   /* collapses on member 0 */
int hipr_group_build_wide4(HiprGroup* group, const HiprBvhNode* nodes, uint32_t node_count, uint32_t triangle_count, HiprWideNode* out_nodes, uint32_t node_capacity,
                           HiprWide4BuildResult* out);   /* collapses on member 0 */
int hipr_group_rebuild_scene_trees(HiprGroup* group, uint32_t max_depth, HiprBvhNode* out_nodes, uint32_t node_capacity, uint32_t* out_order, HiprSlot8* out_slots,
                                   uint32_t slot_capacity, HiprSceneRebuildResult* out);   /* every member rebuilds; member 0's arrays are handed out; their results must agree */
int hipr_group_edit_scene_instances(HiprGroup* group, const HiprInstanceEdit* edits, uint32_t edit_count, uint32_t max_depth, HiprBvhNode* out_nodes, uint32_t node_capacity,
                                    uint32_t* out_order, uint32_t order_capacity, HiprSlot8* out_slots, uint32_t slot_capacity,
                                    HiprSceneEditResult* out);   /* every member edits; member 0's arrays are handed out; their results must agree */
int hipr_group_append_scene_pools(HiprGroup* group, const HiprPoolGrowth* growth);   /* every member checks before any member writes */
int hipr_group_update_scene_lighting(HiprGroup* group, const HiprLight* lights, uint32_t light_count, int environment_action, const HiprEnvironmentBuild* build,
                                     float* out_per_pixel_PDF, uint64_t pdf_capacity, HiprLightSample* out_samples, uint32_t sample_capacity,
                                     HiprLightingResult* out);   /* every member checks before any member writes; member 0's arrays are handed out; their results must agree */
int hipr_group_update_scene_texels(HiprGroup* group, const HiprTexelEdit* edits, uint32_t edit_count, HiprTexelUpdateResult* out);   /* every member checks before any member writes */
int hipr_group_update_scene_vertices(HiprGroup* group, const HiprVertexEdit* edits, uint32_t edit_count, HiprVertexUpdateResult* out);   /* every member checks before any member writes */
int hipr_group_set_scene_rigs(HiprGroup* group, const HiprRigDesc* rigs, uint32_t count);   /* every member checks before any member writes */
int hipr_group_pose_scene_rigs(HiprGroup* group, const HiprRigPose* poses, uint32_t pose_count, HiprVertexUpdateResult* out);   /* every member checks before any member writes */
int hipr_group_update_scene_materials(HiprGroup* group, const HiprMaterialUpdate* materials, uint32_t material_count,
                                      const HiprInstanceMaterial* assignments, uint32_t assignment_count);   /* every member checks before any member writes */
int hipr_group_set_scene_state(HiprGroup* group, const HiprSceneState* state);
int hipr_group_set_entry_point(HiprGroup* group, int entry);
int hipr_group_use_scratch_accumulation(HiprGroup* group, int enable);
int hipr_group_set_frame(HiprGroup* group, uint32_t width, uint32_t height, uint32_t samples_per_pass);
int hipr_group_set_samples_per_pass(HiprGroup* group, uint32_t samples_per_pass);
/* One host thread per member runs hipr_trace_pass; returns when every member has queued its last bounce. */
int hipr_group_trace_pass(HiprGroup* group, const HiprCameraState* camera);
/* Every member folds the samples into its running mean; with an output buffer (on member 0's device, full frame, row pitch in
 * pixels) the compact tiles are gathered and the frame is assembled there. */
int hipr_group_accumulate_samples(HiprGroup* group, uint32_t first_sample, uint32_t sample_count, uint32_t first_accumulation,
                                  void* out_half4_device, uint32_t out_pitch_pixels, int synchronize);
/* The full frame's f64 accumulation, row-major, assembled on the host from the members' tiles. */
int hipr_group_read_accumulation(HiprGroup* group, double* out_rgba, uint64_t capacity_pixels);
int hipr_group_get_counters(HiprGroup* group, HiprCounters* out);   /* sums over the members */

/* ------------------------------------------------------------------------------------------- */
/* Presentation side: what DX11OptiXAdaptor::Adaptor does around Renderer::render                */
/* (extensions/DX11OptiXAdapter/DX11OptiXAdaptor/Adaptor.cpp:141-247), so that the host library   */
/* above this ABI links no GPU runtime.                                                          */
/* ------------------------------------------------------------------------------------------- */
/* The render target / back buffer the adaptor owns (Adaptor.cpp:227-247 resize_render_target). */
int hipr_device_malloc(HiprContext* context, uint64_t bytes, void** out_device_pointer);
int hipr_device_free(HiprContext* context, void* device_pointer);   /* waits for the context stream first */
int hipr_device_memset(HiprContext* context, void* device_pointer, int byte_value, uint64_t bytes);   /* on the context stream: the clear of the back buffer before the cameras composite */
/* optix::Buffer::map() of the non-interop path (Adaptor.cpp:159-166). Blocking. */
int hipr_copy_to_host(HiprContext* context, void* host, const void* device_pointer, uint64_t bytes);
/* The adaptor's full-screen blit (Adaptor.cpp:96-100): backbuffer[x + y * backbuffer_pitch] =
 * pixels[x + (height - y - 1) * pitch] for the width x height viewport. Runs on the context stream. */
int hipr_present_flipped(HiprContext* context, const void* pixels_half4_device, uint32_t pitch_pixels, uint32_t width, uint32_t height,
                         void* backbuffer_half4_device, uint32_t backbuffer_pitch_pixels);

int hipr_synchronize(HiprContext* context);
int hipr_get_counters(HiprContext* context, HiprCounters* out);
int hipr_reset_counters(HiprContext* context);
/* Enables per-ray node / triangle visit counting in the trace kernels (slower, off by default). */
/* Number of independent wavefronts a pass is split into (0..4; at most one per 65536 path slots of the frame). Each share of the path
 * slots runs its bounces on its own stream, so one shades while another traces; results are bit-identical for any count. 0 (the default, or
 * HIPR_WAVEFRONTS) chooses by scene: two for scenes traced by the exhaustive / BVH2 kernels (+9 % ... +27 % on the Cornell box), one for the
 * persistent wide-BVH kernels, which fill the machine alone (measured: no gain, and per-kernel timers then time kernels that ran alone). */
int hipr_set_wavefront_count(HiprContext* context, int count);
/* The number of wavefronts the next pass runs as under the current frame, scene and limit: with the limit at 0 the library takes two for the persistent
 * kernels from 2^24 path slots per pass on (where one wavefront's launch drains, the other's blocks move in: profiles/r04_ab_wavefronts.txt), one below,
 * two for the small-scene kernels. 0 before hipr_set_frame. */
int hipr_get_wavefront_count(HiprContext* context, int* out_count);
/* How the uploaded scene is traced (chosen from its size; HIPR_TRACE_VARIANT overrides for experiments):
 *   HIPR_TRACE_BVH2             BVH2 kernels, one ray per lane (k_trace_closest / k_trace_shadow)
 *   HIPR_TRACE_WIDE_PERSISTENT  more than 64 BVH2 nodes: persistent kernels over the compressed 4-wide BVH; from bounce 1 on the
 *                               closest-hit rays of a bounce and the shadow rays of the previous one share one fused launch,
 *                               timed under HIPR_KERNEL_TRACE_CLOSEST
 *   HIPR_TRACE_EXHAUSTIVE       at most 64 triangles: every ray tests every triangle (k_trace_*_small)
 *   HIPR_TRACE_WIDE8_PERSISTENT more than 64 BVH2 nodes and HiprSceneDesc::wide8_slots given (the default then): persistent kernels over the 8-wide
 *                               tree with leaf records (k_trace_wide8), fused launches like HIPR_TRACE_WIDE_PERSISTENT
 * The CPU oracle has the same three searches; parity tests pick the matching one. */
enum { HIPR_TRACE_BVH2 = 0, HIPR_TRACE_WIDE_PERSISTENT = 1, HIPR_TRACE_EXHAUSTIVE = 2, HIPR_TRACE_WIDE8_PERSISTENT = 3 };
int hipr_get_trace_variant(HiprContext* context, int* out_variant);
/* Forces one of the searches above for the scenes uploaded AFTER the call (-1: by scene size, the default). Meant for tests and A/B measurements: every
 * search returns the same hits up to the rounding of its triangle solve; the oracle restates each of them. */
int hipr_set_trace_variant(HiprContext* context, int variant);
/* Pipelined passes (off by default; scenes traced by the persistent kernels only): consecutive hipr_trace_pass calls alternate between two sets of queues,
 * radiance buffers and streams, and a pass whose live paths have dwindled to under 1/64 of its slots queues all bounces that can still follow without waiting
 * for their sizes and returns, so that its tail -- launches that each take as long as one traversal -- drains while the next pass's full-size launches run.
 * Frames and counters are those of unpipelined passes bit for bit (tested). Measured on the MI355X it does not pay: the persistent kernels fill the CUs, the
 * tail's launches wait for their blocks to retire, and the blind bounces add empty launches (material scene, 32 bounces: 23.4 -> 24.1 ms per step). */
int hipr_set_pass_pipelining(HiprContext* context, int enable);
/* Back sides of one-sided surfaces (on by default; scenes traced by the 8-wide search). The reference's hit program refuses a closest hit that reaches a
 * one-sided surface from behind and traces the path's ray again from just past it (ORS/MonteCarlo.cu:147-164); with this on, the traversal steps over such
 * a hit itself -- when the triangle carries HIPR_TRIANGLE_ONE_SIDED and the hit is behind by more than HiprLeaf8::facing_margin -- and goes on to the hit the
 * retrace would have found. Same paths, same frames (tested against the retracing search); one BVH query less per refused hit: 18 % of the closest-hit
 * queries of the atrium. Hits inside the margin still go to the hit program. The one difference: a refused triangle that COINCIDES with another surface at the
 * same distance no longer hides it (the retrace starts past both). 0 restores the retrace for every refused hit. Applies to every closest-hit query of
 * the 8-wide search, the stage-level hipr_debug_trace_closest included. */
int hipr_set_backface_culling(HiprContext* context, int enable);
/* Arithmetic of the shade stage (K3: attribute interpolation, BSDFs, lights, next event estimation; the other kernels are correctly rounded always).
 *   HIPR_ARITHMETIC_FAST  (default) division, square root, sin, cos and pow by the hardware's approximations, contraction allowed, denormals flushed: what the
 *                         reference's shading PTX is built with (nvcc --use_fast_math, extensions/OptiXRenderer/CMakeLists.txt:82-83).
 *   HIPR_ARITHMETIC_EXACT IEEE division and square root, one rounding per operation, sin / cos / pow as the specified binary64 sequences of csrc/spec_math.h:
 *                         every pixel of every frame equals the CPU restatement (oracle/) in every bit, whatever the resolution or sample count -- the mode that
 *                         meets BASELINE.json's RMSE bound by construction (RMSE 0). About 10 % slower per step (bench.py config.exact_mode).
 * Both builds of the shade unit live in this library; the switch takes effect with the next pass (accumulate from zero after changing it: the two modes are
 * different, equally valid estimators of the same image). Environment HIPR_ARITHMETIC=exact|fast sets the default of new contexts.
 * Replaces a build-time choice of the reference (its CMake flag); no run-time counterpart there. */
enum { HIPR_ARITHMETIC_FAST = 0, HIPR_ARITHMETIC_EXACT = 1 };
int hipr_set_arithmetic(HiprContext* context, int arithmetic);
int hipr_get_arithmetic(HiprContext* context);      /* HIPR_ARITHMETIC_*, or a negative status */
int hipr_set_instrumentation(HiprContext* context, int count_traversal_steps);
int hipr_reset_timers(HiprContext* context);
int hipr_get_kernel_times(HiprContext* context, HiprKernelTimes* out);

/* ------------------------------------------------------------------------------------------- */
/* Stage-level entry points used by the parity tests: each runs ONE kernel of the path on       */
/* host-provided inputs and returns its raw output, so the kernels can be compared with the     */
/* CPU oracle bit for bit where the arithmetic is integer or correctly rounded f32.             */
/* ------------------------------------------------------------------------------------------- */
/* K1: camera rays for all owned pixels (ORS/SimpleRGPs.cu:44-72). Outputs host arrays of
 * owned_pixel_count entries: origin_tmin (float4), direction (float4, w unused), pixel (uint2 as x | y << 16). */
int hipr_debug_generate(HiprContext* context, const HiprCameraState* camera, uint32_t accumulation,
                        float* out_origin_tmin, float* out_direction, uint32_t* out_pixel);
/* RNG: PracticalScrambledSobol::sample4ui (OR/RNG.h:280-287) for n (accumulation, pixel_hash, dimension) triples. */
/* The shading models as the shade kernel evaluates them (DefaultShading / DiffuseShading / TransmissiveShading of
 * ORS/ShadingModels/), for the reference's golden vectors (ORT/ShadingModels/DefaultShadingTest.h:410-447,
 * TransmissiveShadingTest.h:203-236). shading_model: HIPR_SHADING_*. params10: tint[3], roughness, specularity, metallic,
 * coat, coat_roughness, cos_theta_o (NaN: wo.z), max_PDF_hint (NaN: none). mode 0: sample(wo, u = in) -> out7 = f[3], pdf,
 * direction[3]; mode 1: evaluate_with_PDF(wo, wi = in) -> out7 = f[3], pdf, 0, 0, 0. Host pointers. */
int hipr_debug_shading(HiprContext* context, int shading_model, const float* params10, const float* wo_n3, const float* in_n3, uint32_t n, int mode,
                       float* out_n7);
/* K3 at stage level: shade_path -- the closest-hit / miss / light-hit programs of ORS/MonteCarlo.cu:129-302 and ORS/SimpleRGPs.cu:349-362 as the shade kernel runs
 * them -- for n given queue entries of the uploaded scene: rays_n8 = origin, tmin, direction, BSDF PDF of the ray (raw: negative = delta dirac); throughput_bounces_n4 =
 * throughput, bits(bounces); hits_n4 = t, u, v, bits(triangle | 0x80000000 + light | 0xFFFFFFFF miss) as hipr_debug_trace_closest returns them; the triangle the ray
 * left from, the pixel's hash (pcg2d(x, y).x) and the accumulation of the sample. out_n32: per entry 0 flags (1 the path continues, 2 a shadow ray was emitted, 4 the hit
 * was shaded), 1-3 radiance added, 4-7 next origin + tmin, 8-11 next direction + BSDF PDF, 12-15 throughput + bits(bounces), 16 bits(last accepted triangle), 17-20
 * shadow origin + tmax, 21-23 direction to the light, 24-26 radiance the shadow ray carries; words of parts that do not apply are zero. Host pointers. The oracle's
 * hit programs write the same record (tests: bit-identical for the verification build, decision by decision statistics for the product). */
int hipr_debug_shade(HiprContext* context, const HiprCameraState* camera, uint32_t n, const float* rays_n8, const float* throughput_bounces_n4, const float* hits_n4,
                     const uint32_t* last_triangle, const uint32_t* pixel_hash, const uint32_t* accumulation, float* out_n32);
/* The light sources as the shade kernel evaluates them, for the reference's light tests (ORT/LightSources/SphereLightTest.h,
 * SpotLightTest.h). mode 0: LightSources::sample_radiance(light, position, u = in.xy) -> out8 = radiance[3], PDF,
 * direction_to_light[3], distance. mode 1 (spot lights only): out8 = evaluate(light, position, direction = in)[3],
 * pdf(light, position, direction), 0, 0, 0, 0. Host pointers; position3 is shared by the n inputs. */
int hipr_debug_light(HiprContext* context, const HiprLight* light, const float* position3, const float* in_n3, uint32_t n, int mode, float* out_n8);
/* The transcendentals of the shade unit in the context's arithmetic mode, over arrays: function 0 sin(x), 1 cos(x), 2 pow(x, y) (y ignored otherwise). In the exact
 * mode the results are csrc/spec_math.h's, bit for bit those of the oracle's restatement (tests/test_gpu_verify_build.py). */
int hipr_debug_math(HiprContext* context, int function, uint32_t n, const float* x, const float* y, float* out);
int hipr_debug_sobol(HiprContext* context, const uint32_t* accumulation_pixelhash_dimension, uint32_t n, uint32_t* out_uint4);
/* The VALU roof of the device the context runs on, measured (bench.py's roofline_valu; no reference counterpart): eight independent chains of one
 * instruction per lane, eight waves per SIMD on every CU, best of three launches. out3[0] = v_fma_f32, out3[1] = v_max_f32, out3[2] = v_cvt_f32_ubyte1,
 * each in wave64 instructions per second device-wide (tools/microbench/issue_rates.hip has the full table: profiles/r03_issue_rates.txt). */
int hipr_debug_valu_issue_rates(HiprContext* context, double* out3);
/* The 256 float4 reverse-Halton offsets the next event estimation candidates are drawn with, read back from the device
 * (g_random_sample_offsets, OR/Renderer.cpp:323-336). out_256x4: host pointer to 1024 floats. */
int hipr_debug_sample_offsets(HiprContext* context, float* out_256x4);
/* K2: closest hit for n rays. rays: float4 origin_tmin + float4 direction_tmax per ray; skip: global triangle index
 * to ignore per ray (0xFFFFFFFF = none). out_hits: float4 {t, u, v, bits(tri_or_light)} per ray. */
int hipr_debug_trace_closest(HiprContext* context, const float* rays, const uint32_t* skip, uint32_t n, float* out_hits);
/* K4: shadow transmittance for n rays (float4 origin_tmin + float4 direction_tmax) -> one float per ray. */
int hipr_debug_trace_shadow(HiprContext* context, const float* rays, uint32_t n, float* out_transmittance);
/* K2 + K4 in ONE fused launch, as a bounce makes it for scenes of the persistent kernels (HIPR_ERROR_UNSUPPORTED for the others): n_closest closest-hit rays and
 * n_shadow shadow rays in the layouts of the two entries above; either count may be 0, and its pointers are then not read. */
int hipr_debug_trace_fused(HiprContext* context, const float* closest_rays, const uint32_t* skip, uint32_t n_closest, const float* shadow_rays, uint32_t n_shadow,
                           float* out_hits, float* out_transmittance);
/* The three launches above over the 8-wide tree (HIPR_ERROR_UNSUPPORTED for other searches), GIVEN A HINT TABLE: the record slot a ray looks at before it starts on the
 * root, `tag | slot` per word, the tag being the resident tree's generation in the top byte (*out_tag when out_tag is not NULL; never 0, and it changes whenever the
 * tree is replaced). mode 0 = closest-only (n_shadow = 0; word = ray index / 64), 1 = shadow-only (n_closest = 0), 2 = fused (1 and 2: word = shadow ray index / 64).
 * hints: hint_words words, at least one per 64 rays of the keyed kind, read and written by the launch and returned as it left them. A word that carries the tree's tag
 * must name a leaf record (HIPR_ERROR_INVALID_ARGUMENT otherwise); any other word is ignored by the kernel. Results do not depend on what the table holds. Launches
 * that have no code for hints (instrumentation on; shadow rays of a scene with coverage) leave the table as given. */
int hipr_debug_trace_hinted(HiprContext* context, int mode, const float* closest_rays, const uint32_t* skip, uint32_t n_closest, const float* shadow_rays, uint32_t n_shadow,
                            uint32_t* hints, uint32_t hint_words, float* out_hits, float* out_transmittance, uint32_t* out_tag);
/* K5c: the listing pass of a bounce on n given hits (hits_n4: float4 {t, u, v, bits(triangle | 0x80000000 + light | 0xFFFFFFFF miss)} per queue entry). out_order[p]
 * = the queue entry the shade kernel takes at place p: every chunk of 4096 places holds that chunk's own entries as [plain surface hits | coated surface hits |
 * everything else], each class in queue order. coat_classes != 0 lists the hits on triangles of a coated material apart (needs an uploaded scene, and every
 * triangle id below its triangle count); 0 lists them with the plain ones. grid: blocks of the launch, 0 = what a pass takes. Host pointers. */
int hipr_debug_classify_hits(HiprContext* context, const float* hits_n4, uint32_t n, int coat_classes, uint32_t grid, uint32_t* out_order);
/* The uploaded (or device-refitted, or material-updated) scene arrays as the device holds them: HiprTriangle[triangle_count], HiprSlot8[wide8_slot_count], the
 * trace records (48 bytes per triangle), the shading records (128 bytes per triangle), the class bytes of the listing pass (one per triangle),
 * HiprMaterial[material_count], HiprInstance[instance_count]; and the pools hipr_append_scene_pools grows, each exactly as long as its count: the index words,
 * HiprVertexGeometry[vertex_count], the texcoords, tints and emissions (an absent pool reads as zero bytes), HiprTexture[texture_count], the texel bytes.
 * hipr_debug_scene_buffer_bytes: the bytes a read of `which` takes. */
enum { HIPR_SCENE_BUFFER_TRIANGLES = 0, HIPR_SCENE_BUFFER_WIDE8_SLOTS = 1, HIPR_SCENE_BUFFER_TRACE_TRIANGLES = 2, HIPR_SCENE_BUFFER_SHADE_TRIANGLES = 3,
       HIPR_SCENE_BUFFER_TRIANGLE_CLASS = 4, HIPR_SCENE_BUFFER_MATERIALS = 5, HIPR_SCENE_BUFFER_INSTANCES = 6, HIPR_SCENE_BUFFER_NODES = 7 /* the BVH2 */,
       HIPR_SCENE_BUFFER_INDICES = 8, HIPR_SCENE_BUFFER_GEOMETRY = 9, HIPR_SCENE_BUFFER_TEXCOORDS = 10, HIPR_SCENE_BUFFER_TINTS = 11, HIPR_SCENE_BUFFER_EMISSIONS = 12,
       HIPR_SCENE_BUFFER_TEXTURES = 13, HIPR_SCENE_BUFFER_TEXELS = 14,
       /* what hipr_update_scene_lighting writes: HiprLight[light_count], the environment's pdf_width x pdf_height floats and its HiprLightSample[sample_count]
          (no environment: zero bytes) */
       HIPR_SCENE_BUFFER_LIGHTS = 15, HIPR_SCENE_BUFFER_ENVIRONMENT_PDF = 16, HIPR_SCENE_BUFFER_ENVIRONMENT_SAMPLES = 17 };
int hipr_debug_read_scene_buffer(HiprContext* context, int which, void* out, uint64_t capacity_bytes);
int hipr_debug_scene_buffer_bytes(HiprContext* context, int which, uint64_t* out_bytes);
/* Milliseconds of the context's last successful hipr_append_scene_pools that did any work: the new allocations (the host's clock), the device-to-device copies of
 * the resident parts into them and the host-to-device tails with the mirror segments (both between events on the stream: the call does not synchronise for them)
 * (tools/pool_growth_probe.py). The old buffers are freed after the third. */
int hipr_debug_append_times(HiprContext* context, double* out3_ms);
/* Milliseconds of the context's last successful hipr_build_bvh2, which add up to the call: the argument checks (the pass over all corners for one that is not
 * finite), scratch allocation + upload, kernels, read-back (tools/device_build_probe.py). */
int hipr_debug_build_times(HiprContext* context, double* out4_ms);
/* The same for the context's last successful hipr_build_wide8: the walk over the indices, allocation + upload, kernels (with the few words read per level), read-back. */
int hipr_debug_collapse_times(HiprContext* context, double* out4_ms);
/* ... and for the context's last successful hipr_build_wide4: the walk over the indices, allocation + upload, kernels (with the few words read per level), read-back
 * (tools/wide4_collapse_probe.py). */
int hipr_debug_collapse4_times(HiprContext* context, double* out4_ms);
/* The same for the context's last successful hipr_rebuild_scene_trees: the flatten order, the BVH2 build, the hand-over and the collapse with its slots copied to the
 * host, the new resident arrays with what is derived from them, the read-back of the outputs (tools/device_rebuild_probe.py). */
int hipr_debug_rebuild_times(HiprContext* context, double* out5_ms);
/* ... and for the context's last successful hipr_update_scene_lighting: the allocations with the uploads of the tables and the lights queued (the host's clock), the
 * kernels (between events on the stream: no synchronise is added for them), the host's finish of the samples, the read-back with the samples' upload. */
int hipr_debug_lighting_times(HiprContext* context, double* out4_ms);
/* ... and for the context's last successful hipr_update_scene_texels that did any work: the rows packed and their staging copy queued (the host's clock), the
 * rectangle writes, the coverage pass (the flags of the affected materials' triangles decided again) and the leaf pass (each between events on the stream: the call
 * does not synchronise for them) (tools/texel_update_probe.py). */
int hipr_debug_texel_update_times(HiprContext* context, double* out4_ms);
/* ... and for the context's last successful hipr_update_scene_vertices that did any work: the segments and rows packed and their staging copy queued (the host's
 * clock), the pool writes with the marks, the moved triangles with the refit passes and the records, the flag pass with the leaf pass (each between events on the
 * stream: the call does not synchronise for them) (tools/vertex_update_probe.py). */
int hipr_debug_vertex_update_times(HiprContext* context, double* out4_ms);
/* ... and for the context's last successful hipr_pose_scene_rigs that did any work: the block table, matrices and weights packed and their staging copy queued (the
 * host's clock), the pose kernel with the marks, the moved triangles with the refit passes and the records (each between events on the stream), and 0
 * (tools/vertex_pose_probe.py). */
int hipr_debug_vertex_pose_times(HiprContext* context, double* out4_ms);
/* The LDS budget of the pose kernel in joints for this context's next poses (32 when the context is made): a rig with more joints gathers its matrices from global
 * memory. 0: every rig gathers. Refuses a value above the kernel's capacity of 320 (HIPR_ERROR_INVALID_ARGUMENT). For measurements and tests: both paths give the
 * same bytes. */
int hipr_debug_set_pose_lds_joints(HiprContext* context, uint32_t joints);

#ifdef __cplusplus
}
#endif

#endif /* HIPRENDERER_C_H */
