// host/SceneBuilder.h -- flattens meshes / models / materials / lights into the HiprSceneDesc the
// kernels consume. This is the host work OptiXRenderer::Renderer::handle_updates() does against the
// OptiX scene graph (OptiXRenderer/Renderer.cpp:92-182 load_mesh / create_model / transformable_model,
// :754-812 upload_material, :855-902 light_creation), re-targeted at flat SoA arrays + a BVH2.
#pragma once

#include "BvhBuilder.h"
#include "Math.h"
#include "../csrc/vertex_pose.h"      // the rigs: ONE text of the pose arithmetic with the device's kernel

#include <cassert>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace HIPRenderer {

using namespace Bifrost::Math;

struct MeshData {
    std::string name;
    std::vector<Vector3f> positions;
    std::vector<Vector3f> normals;      // empty or one per vertex
    std::vector<Vector2f> texcoords;    // empty or one per vertex
    std::vector<uint32_t> tints;        // uchar4 (tint rgb, roughness), empty or one per vertex
    std::vector<Vector3f> emission;     // empty or one per vertex
    std::vector<Vector3ui> primitives;
};

struct ImageData {
    uint32_t width = 0, height = 0;
    uint8_t format = HIPR_TEXEL_RGBA8;  // HIPR_TEXEL_*
    bool is_sRGB = false;
    std::vector<uint8_t> pixels;
};

struct CameraDescription {
    Transform transform = Transform::identity();
    float field_of_view = 3.14159265358979323846f / 4.0f;   // SimpleViewer default, CameraHandlers.cpp:111
    float near_plane = 0.1f, far_plane = 100.0f;
    uint32_t max_bounce_count = 4;
    bool orthographic = false;                               // compute_orthographic_projection, Camera.cpp:268-286
    float ortho_width = 1.0f, ortho_height = 1.0f, ortho_depth = 1000.0f;
};

class SceneBuilder {
public:
    SceneBuilder();
    static constexpr bool takes_textures = true;        // Scenes::build_atrium's textured variant

    uint32_t add_mesh(MeshData mesh);                                   // returns mesh index
    uint32_t add_material(const HiprMaterial& material);                // returns material index (0 is the invalid material)
    uint32_t add_texture(const ImageData& image, bool repeat_u, bool repeat_v, bool linear_magnification, bool linear_minification);
    // model_index: the MeshModel UID index used for InstanceID; 0 = next sequential index. Returns the index used.
    uint32_t add_model(uint32_t mesh, uint32_t material, const Transform& transform, uint32_t model_index = 0);
    void add_light(const HiprLight& light);
    // The lat-long image is texture `texture_index` (add_texture); PDF texels and samples as PresampledEnvironment.h builds them. With two or
    // more samples the environment also joins the light list for next event estimation (OptiXRenderer/Renderer.cpp:1160-1196).
    void set_environment(uint32_t texture_index, uint32_t pdf_width, uint32_t pdf_height, std::vector<float> per_pixel_PDF, std::vector<HiprLightSample> samples);

    static HiprLight sphere_light(Vector3f position, RGB power, float radius);
    static HiprLight spot_light(Vector3f position, Vector3f direction, RGB power, float radius, float cos_angle);
    static HiprLight directional_light(Vector3f direction, RGB radiance);
    static HiprMaterial make_material(RGB tint, float roughness, float specularity, float metallic, uint16_t flags = 0, uint16_t shading_model = HIPR_SHADING_DEFAULT);
    static uint16_t unorm16(float v);

    void set_environment_tint(RGB tint) { m_state.environment_tint[0] = tint.r; m_state.environment_tint[1] = tint.g; m_state.environment_tint[2] = tint.b; }
    void force_shading_model(uint16_t shading_model);   // e.g. the diffuse-only configuration of BASELINE.json

    // Transforms every model to world space, builds the BVH and fills desc().
    void finalize(uint32_t bvh_max_depth = 62);

    // Transform-only update after finalize(): the models named by their model index (add_model's return value) get new object-to-world
    // transforms; their world-space triangles are recomputed in place (BVH leaf order kept) and the BVH is REFIT, not rebuilt -- what the
    // reference does when a node moves (root acceleration refit, OR/Renderer.cpp:472,1010-1041). When the refit tree's box area has grown
    // past `rebuild_threshold` times the built tree's (a badly stretched tree traverses slowly) the scene is rebuilt instead. Returns true when
    // the topology was kept (nodes, triangle order and counts unchanged: hipr_update_scene_geometry suffices), false after a rebuild.
    bool update_model_transforms(const std::vector<std::pair<uint32_t, Transform>>& model_transforms, double rebuild_threshold = 1.5);
    // The same update in two steps, for a renderer whose device refits the tree itself (hipr_refit_scene_transforms): stage_model_transforms records the
    // matrices in the instances, decides flips as update_model_transforms does and appends the instances it touched, with their 3x4 matrices, to
    // `moved_instances` -- the triangles and the trees are NOT touched: while has_staged_transforms() holds, desc() and bounds() are those of the poses before.
    // Whoever needs the description then (a new camera's upload, a rebuild, the fallback) calls apply_staged_transforms() first, which runs the code of
    // update_model_transforms over everything staged; true = topology kept, false = the scene was rebuilt (a flip, the BVH2's ratio rule) and every holder
    // of the old description needs the new one whole. stage_model_transforms returns false when an update turns an instance inside out (the device cannot
    // refit that; apply_staged_transforms will rebuild). rebuild(): a fresh tree over the instances as they stand.
    bool stage_model_transforms(const std::vector<std::pair<uint32_t, Transform>>& model_transforms, std::vector<HiprInstanceTransform>& moved_instances);
    bool apply_staged_transforms(double rebuild_threshold = 1.5);
    bool has_staged_transforms() const { return m_staged; }
    void rebuild();
    // The BVH2 stage of every later finalize() / rebuild() taken from `source` (hipr_build_bvh2 behind a context: the same tree, built on the device). A source that
    // declines or fails is followed by the host's stage, silently: the scene is the same either way. Bvh2Source() removes it. build_counts(): builds whose BVH2 the
    // source made, and builds where it was asked and the host built instead.
    void set_bvh2_source(const Bvh2Source& source) { m_bvh2_source = source; }
    struct BuildCounts { unsigned device_builds = 0, declined_builds = 0; };
    BuildCounts build_counts() const { return m_build_counts; }
    uint32_t longest_median_range() const { return m_bvh.longest_median_range; }
    // The same for the 8-wide collapse (hipr_build_wide8 behind a context: the same slots, collapsed on the device); a source that declines or fails is followed by
    // build_wide8, silently. Wide8Source() removes it. collapse_counts(): builds whose 8-wide tree the source made, and builds where it was asked and the host collapsed.
    void set_wide8_source(const Wide8Source& source) { m_wide8_source = source; }
    struct CollapseCounts { unsigned device_collapses = 0, declined_collapses = 0; };
    CollapseCounts collapse_counts() const { return m_collapse_counts; }
    // The same for the 4-wide collapse (hipr_build_wide4 behind a context: the same nodes, collapsed on the device), which finalize() / rebuild() AND both adoptions
    // below ask -- the adoptions are handed a BVH2 and an 8-wide tree, and the 4-wide collapse is what is left to do. A source that declines or fails is followed by the
    // host's collapse, silently. Wide4Source() removes it. wide4_collapse_counts(): tree builds (adoptions included) whose 4-wide tree the source made, and those where
    // it was asked and the host collapsed.
    void set_wide4_source(const Wide4Source& source) { m_wide4_source = source; }
    CollapseCounts wide4_collapse_counts() const { return m_wide4_collapse_counts; }
    // The trees a device rebuild of the resident scene made (hipr_rebuild_scene_trees: the same trees, built from the triangles the device holds) taken over in place of
    // a rebuild(): everything staged is applied to the builder's own triangles WITHOUT a refit and without a flatten, they are brought into flatten order through the
    // old order and into the new one through `order` (order[k] = the flatten position of the triangle at place k: BvhBuildResult::order), the BVH2 (`nodes`,
    // `deepest`) and the 8-wide tree (`slots`, `wide8`) are installed, the 4-wide tree is collapsed on the host from the adopted BVH2, and desc() is, in every
    // array and scalar, what rebuild() leaves. Returns false, with nothing touched, for counts that do not fit, an `order` that is no permutation, a child or
    // leaf reference out of range, or a staged transform that turns an instance inside out. rebuild_counts(): calls that adopted, calls that refused.
    bool adopt_rebuilt_trees(const HiprBvhNode* nodes, uint32_t node_count, const uint32_t* order, uint32_t deepest, const HiprSlot8* slots, const HiprWide8BuildResult& wide8);
    // Models destroyed and created after finalize() (the reference removes or adds a child of its root group, OR/Renderer.cpp:138-182, :1043-1110). Meshes and pools
    // are never dropped: desc() keeps every pool and offset. Both touch the instance list only -- like a staged transform they leave the triangles and the trees
    // behind, and desc() must not be read until rebuild(), apply_staged_transforms() (which rebuilds) or adopt_edited_trees() has caught up.
    // remove_model: every instance of the model leaves the list; false when the scene has none. insert_model: the new instance stands at `position` of the list
    // (at the end for a position past it; add_model after finalize() is that append); `model_index` as add_model's.
    bool remove_model(uint32_t model_index);
    uint32_t insert_model(uint32_t position, uint32_t mesh, uint32_t material, const Transform& transform, uint32_t model_index = 0);
    bool has_staged_edits() const;
    // What hipr_edit_scene_instances takes for the edits since the last build: the new list in order, kept instances named by their index in the list the trees were
    // built over, new ones with their record and primitive count. False -- "not on the device" -- when nothing is built yet, when a pool has grown since (a new mesh,
    // material or texture; the mirrored index copy of a mirrored new instance), or when a transform is staged as well: the caller takes the full path.
    bool staged_instance_edits(std::vector<HiprInstanceEdit>& edits) const;
    // What hipr_append_scene_pools AND hipr_edit_scene_instances take for everything since the last build or adoption, pool growth included: `growth.growth` carries
    // the tails of the pools -- new vertices, with an optional per-vertex pool's tail where the pool existed at that point and the WHOLE pool where it did not; the
    // index tail as segments, from the log add_mesh and index_offset_for keep: mesh triples from the host, mirrored copies as mirrors of the range they copy; new
    // materials, textures and texels -- and `edits` the instance list as staged_instance_edits makes it. The pointers of `growth.growth` point into the builder's pools
    // and into `growth`: they hold until the next add_* call and as long as `growth` lives. False -- "not on the device" -- when nothing is built yet, when a transform
    // is staged as well, or when an environment was set or a light added since.
    struct StagedGrowth {
        HiprPoolGrowth growth = {};
        std::vector<HiprIndexSegment> segments;
        std::vector<uint32_t> host_indices;      // the host segments' words, when mirrors lie between them in the pool; otherwise `growth.indices` points into the pool
    };
    bool staged_scene_growth(StagedGrowth& growth, std::vector<HiprInstanceEdit>& edits) const;
    // adopt_rebuilt_trees generalised to an edited instance list (the trees hipr_edit_scene_instances made): the builder's own triangles of kept instances go to their
    // place in the new list's flatten order with their new instance index, removed ranges are dropped, ONLY the new instances are flattened -- from the builder's own pools, grown or not -- and everything goes
    // through `order` (`order_count` words) into the new trees' order. desc() is then, in every array and scalar, what rebuild() leaves. Refuses as adopt_rebuilt_trees
    // does, with nothing touched; counted in rebuild_counts().
    bool adopt_edited_trees(const HiprBvhNode* nodes, uint32_t node_count, const uint32_t* order, uint32_t order_count, uint32_t deepest, const HiprSlot8* slots, const HiprWide8BuildResult& wide8);
    // The mesh, the material and the place in the instance list of the (first) instance of a model; false when the scene has none.
    bool model_info(uint32_t model_index, uint32_t& mesh, uint32_t& material, uint32_t& position) const;
    struct RebuildCounts { unsigned adopted = 0, refused = 0; };
    RebuildCounts rebuild_counts() const { return m_rebuild_counts; }
    uint32_t desc_triangle_count() const { return uint32_t(m_triangles.size()); }      // desc().triangle_count, also while transforms are staged
    uint32_t bvh_max_depth_limit() const { return m_bvh_max_depth_limit; }             // what finalize() was given: the depth every rebuild builds to
    const std::vector<uint32_t>& order() const { return m_bvh.order; }      // order()[k] = the flatten position of the triangle desc().triangles[k]
    // Material-only update after finalize(): `changed` rewrites material slots, `assignments` gives instances another material. The builder's own description is
    // kept in step WITHOUT a rebuild -- a material moves no corner and the tree builders read no flag, so the trees and the triangle order are the ones a rebuild
    // would make: the flags of the touched instances' triangles are recomputed (csrc/material_rules.h) and the leaf records of the 8-wide tree follow them. What
    // hipr_update_scene_materials does to the resident scene. Returns false, with nothing done, for an index out of range.
    bool update_materials(const std::vector<HiprMaterialUpdate>& changed, const std::vector<HiprInstanceMaterial>& assignments);
    // Pixel edit of a texture of a BUILT scene without a rebuild (what hipr_update_scene_texels does to the resident scene): the rectangle (x, y, width, height) of
    // texture `texture_index` takes `pixels` -- rows `row_pitch_bytes` apart, in the texture's pooled format (RGB24 already expanded, as add_texture leaves it). No
    // corner moves and the tree builders read no flag, so the trees stay; the flags of the triangles of the materials whose deciding coverage texture this is are
    // recomputed (csrc/material_rules.h) and the leaf records of the 8-wide tree follow them: desc() is then, in every array and scalar but the environment's, what
    // a rebuild() makes of the edited image. Returns false, with nothing touched, where the device call would refuse: before the scene is built, a texture the
    // device does not hold (0, outside the pool, added since the last build), a rectangle with an extent of 0 or reaching outside the texture, a pitch below a
    // row's bytes, a coverage texture of a scene of at most 64 triangles. When the texture is the environment's map, the environment's PDF image and samples are
    // left behind: environment_texels_edited() holds until set_environment or an adopt_lighting that builds or removes it (staged_environment_build makes what
    // hipr_update_scene_lighting takes for that).
    bool update_texels(uint32_t texture_index, uint32_t x, uint32_t y, uint32_t width, uint32_t height, const void* pixels, uint64_t row_pitch_bytes);
    bool environment_texels_edited() const { return m_environment_texels_edited; }
    // Vertex edit of meshes of a BUILT scene without a rebuild (what hipr_update_scene_vertices does to the resident scene): vertices [first_vertex, first_vertex +
    // vertex_count) of mesh `mesh` -- MESH-relative -- take the arrays that are not null, in the pools' own layout (geometry: vertex_geometry() packs a position and
    // a normal as add_mesh does). Edits apply in order. update_vertices is the whole host path: the pools are written, the corners of the instances over those
    // meshes recomputed (move_triangles), the coverage flags of their triangles decided again (csrc/material_rules.h) with the leaf records' bits, and the trees
    // refitted under the rule of update_model_transforms: true = topology kept (desc() is then what hipr_update_scene_vertices leaves on the device), false = the
    // scene was rebuilt (a parted pair, the ratio rule) -- or, with *refused set, nothing was touched: before the scene is built, with an instance edit staged, a
    // mesh or a range the scene does not hold or the device does not hold yet (added since the last build), a count of 0, no array, an attribute whose pool did not
    // exist at the last build, a position or texture coordinate that is not finite.
    // stage_vertex_edits is the device path's companion, in the manner of stage_model_transforms: it writes the pools (they are the source data) and the flags,
    // marks the instances over the meshes whose geometry changed as staged and appends the edits in POOL coordinates -- what hipr_update_scene_vertices takes -- to
    // `pool_edits`; apply_staged_transforms() then brings triangles and trees along before desc() is next handed out. False, nothing touched: refused as above.
    struct VertexEdit {
        uint32_t mesh, first_vertex, vertex_count;
        const HiprVertexGeometry* geometry;      // or null: positions and normals stay
        const float* texcoords;                  // float2 each, or null
        const uint32_t* tints;                   // or null
        const float* emissions;                  // float3 each, or null
    };
    bool update_vertices(const std::vector<VertexEdit>& edits, double rebuild_threshold = 1.5, bool* refused = nullptr);
    bool stage_vertex_edits(const std::vector<VertexEdit>& edits, std::vector<HiprVertexEdit>& pool_edits);
    static HiprVertexGeometry vertex_geometry(Vector3f position, const Vector3f* normal);      // null: no normal, as a mesh without normals holds it
    // Rigs over meshes of a BUILT scene (what hipr_set_scene_rigs binds on the device) and their poses (csrc/vertex_pose.h: morph targets, linear-blend skinning,
    // normals through the upper 3x3, normalised and encoded as add_mesh encodes them). set_rigs REPLACES the set; a rig's `first_vertex` is MESH-relative here. The
    // builder keeps its own copies in the resident layout. False, nothing touched: before the scene is built, a mesh the scene does not hold or the device does not
    // hold yet, a range past the mesh, rest normals for a mesh without HIPR_MESH_NORMALS or none for a mesh with them, and everything hipr_set_scene_rigs refuses
    // (hipr::check_rig_descs). The rigs stay until the next set_rigs: the pools only grow. Rig k of the list is rig k of the device when both were given the same
    // list -- after hipr_upload_scene the device's set is bound again.
    // pose_rigs is the whole host path: the rows of every pose computed with the header's text, then update_vertices on them -- true = topology kept (desc() is then
    // what hipr_pose_scene_rigs leaves on the device), false = the scene was rebuilt, or, with *refused set, nothing was touched: what update_vertices refuses about
    // the builder's state and everything hipr_pose_scene_rigs refuses about the poses (hipr::check_rig_poses).
    // stage_rig_poses is the device path's companion: it does NOT skin. It records the LATEST pose of each rig (copies of the matrices and weights), marks the
    // instances over those meshes as staged and appends the poses as the device takes them to `pool_poses`; apply_staged_transforms(), rebuild() or an adoption
    // skins from the recorded poses before the pools are next read -- correct because a posed vertex depends on the rest data and the pose alone. Every other
    // writer of the geometry pool (update_vertices, stage_vertex_edits, pose_rigs, set_rigs) skins the recorded poses FIRST and writes then: the later write wins, as
    // on the device, where the pose has long been applied.
    struct RigDesc { uint32_t mesh; HiprRigDesc rig; };
    bool set_rigs(const std::vector<RigDesc>& rigs);
    bool pose_rigs(const std::vector<HiprRigPose>& poses, double rebuild_threshold = 1.5, bool* refused = nullptr);
    bool stage_rig_poses(const std::vector<HiprRigPose>& poses, std::vector<HiprRigPose>& pool_poses);
    size_t rig_count() const { return m_rig_books.size(); }
    // The HiprVertexGeometry rows of one rig under one pose (rig.vertex_count of them; rig.first_vertex is not read): false when the rig or the pose is one the
    // device refuses.
    static bool posed_geometry(const HiprRigDesc& rig, const HiprRigPose& pose, HiprVertexGeometry* out);
    // vertex_offset, vertex_count, index_offset (in triples), primitive_count and flags of a mesh; false for a mesh the scene does not hold
    bool mesh_range(uint32_t mesh, uint32_t (&out)[5]) const;
    const std::vector<HiprMaterial>& materials() const { return m_materials; }
    const std::vector<HiprLight>& lights() const { return m_lights; }
    const std::vector<HiprTexture>& textures() const { return m_textures; }      // slot 0, "no texture", included
    const std::vector<HiprInstance>& instances() const { return m_instances; }
    // The lights of a finalized scene replaced one for one (moved or re-coloured lights; the count must match).
    bool replace_lights(const std::vector<HiprLight>& lights);
    // Lighting edits of a BUILT scene without a rebuild (what hipr_update_scene_lighting does to the resident scene; the reference rewrites its light buffer in
    // place and presamples its environment without touching geometry, OR/Renderer.cpp:852-1008, :1136-1196). No triangle, tree or pool follows a light or the
    // environment's data, so desc() is brought along in place and is then, in every array and scalar, what add_light / set_environment and rebuild() leave.
    // set_lights: the light list replaced by `lights`, any count and any types, with the presampled environment's light -- which `lights` must not carry -- kept
    // last. False, with nothing touched, before the scene is built or for a list that carries that light.
    bool set_lights(const std::vector<HiprLight>& lights);
    // What hipr_update_scene_lighting takes to build the environment of texture `texture_index` on the device: the three tables the host path evaluates through
    // libm -- the sine of every PDF row (compute_distribution), the linear value of every sRGB byte (get_pixel), the progressive multi-jittered draw points in the
    // order presample_environment visits them -- owned by `staged`, whose `build` points into it: they hold as long as `staged` lives. `sample_count` is rounded
    // up to a power of two, at least 2, as presample_environment does. The points depend on the count alone and are the expensive table (61 ms at 8192): the builder
    // keeps those of the last count asked for. False for a texture the builder does not hold.
    struct StagedEnvironmentBuild {
        HiprEnvironmentBuild build = {};
        std::vector<float> row_sines, srgb_decode, draw_points;
    };
    bool staged_environment_build(uint32_t texture_index, uint32_t sample_count, StagedEnvironmentBuild& staged) const;
    // The outcome of a hipr_update_scene_lighting taken over: `lights` as set_lights takes them; `environment_action` HIPR_ENVIRONMENT_KEEP, _REMOVE (the builder
    // drops its environment), or _BUILD with the texture, the extents `result` reports and the PDF texels and samples the call handed out, which become the
    // builder's as set_environment would take them. False, with nothing touched, where set_lights refuses, for an unknown action, or for arrays whose sizes are
    // not the ones `result` reports.
    bool adopt_lighting(const std::vector<HiprLight>& lights, int environment_action, uint32_t texture_index, const HiprLightingResult& result, std::vector<float> per_pixel_PDF,
                        std::vector<HiprLightSample> samples);

    const HiprSceneDesc& desc() const { assert(!m_staged && "apply_staged_transforms() first: the instances lead the triangles and the trees"); return m_desc; }
    const HiprSceneState& state() const { return m_state; }
    HiprSceneState& state() { return m_state; }
    CameraDescription camera;
    AABB bounds() const { assert(!m_staged && "apply_staged_transforms() first"); return m_bounds; }
    size_t mesh_count() const { return m_meshes.size(); }
    size_t texture_count() const { return m_textures.size(); }      // slot 0, "no texture", included
    size_t model_count() const { return m_instances.size(); }

private:
    struct MeshRecord { uint32_t index_offset, vertex_offset, primitive_count, vertex_count, flags; uint32_t mirrored_index_offset = 0xFFFFFFFFu; };
    // The index triples an instance of `mesh` under `object_to_world` uses: the mesh's own, or -- a transform that mirrors (negative determinant) -- a copy of
    // them with the second and third corner exchanged, so that the world-space corners wind the way the reference's transformed geometric normal points
    // (rtTransformNormal through the inverse transpose, ORS/MonteCarlo.cu:147) and every consumer of the triple order sees the same triangle.
    uint32_t index_offset_for(uint32_t mesh, const float* object_to_world);
    void build_trees_over(const std::vector<HiprTriangle>& world, const Bvh2Source& bvh2_source, Bvh2SourceReport& report, const Wide8Source& wide8_source, Wide8SourceReport& wide8_report);      // the 4-wide collapse from m_wide4_source, counted
    void move_triangles(const std::vector<bool>& moved);
    void flatten_instance(uint32_t instance, std::vector<HiprTriangle>& world);
    bool trees_fit(uint32_t triangle_count, const HiprBvhNode* nodes, uint32_t node_count, const uint32_t* order, const HiprSlot8* slots, const HiprWide8BuildResult& wide8) const;
    void note_instance_edit();
    bool write_vertex_edits(const std::vector<VertexEdit>& edits, std::vector<HiprVertexEdit>* pool_edits);      // what update_vertices and stage_vertex_edits share
    void refresh_leaf_material_bits();      // bits 0..3 of every leaf record of the 8-wide tree from m_triangles' flags
    bool list_instance_edits(std::vector<HiprInstanceEdit>& edits) const;      // staged_instance_edits without its question about the pools
    // The pool sizes at the last build or adoption (build_trees_over): what the device holds when it follows the builder, and where the tails begin.
    struct PoolSizes { size_t index_words = 0, vertices = 0, materials = 0, textures = 0, texel_bytes = 0, lights = 0; bool texcoords = false, tints = false, emission = false; };
    PoolSizes m_built_pools;
    // The ranges m_indices has grown by since then, in order: a mesh's triples (mirrored_from == HIPR_SEGMENT_FROM_HOST) or the mirrored copy of the triples from
    // `mirrored_from` on. Cleared with every build.
    std::vector<HiprIndexSegment> m_index_log;
    bool m_environment_set_since = false;      // set_environment after the last build: the environment's data is an upload's business
    bool m_environment_texels_edited = false;  // update_texels wrote into the environment's map: its PDF image and samples describe the image before
    static constexpr uint32_t NOT_BUILT = 0xFFFFFFFFu;
    std::vector<uint32_t> m_built_index;      // per instance: its index in the list the triangles and the trees were built over, NOT_BUILT for one created since
    uint32_t m_built_instance_count = 0;      // the length of that list
    bool m_built = false, m_pools_grew = false;      // trees exist; a pool has grown since they were built
    RebuildCounts m_rebuild_counts;
    bool record_model_transforms(const std::vector<std::pair<uint32_t, Transform>>& model_transforms, std::vector<HiprInstanceTransform>* moved_instances);
    bool m_staged = false, m_staged_flips = false;      // transforms recorded in m_instances that m_triangles / m_bvh do not carry yet
    std::vector<bool> m_staged_moved;
    // The bound rigs in the resident layout (csrc/vertex_pose.h pack_rig), pool coordinates; the mesh of each; the latest staged pose of each (empty: none).
    std::vector<uint32_t> m_rig_words;
    std::vector<hipr::PoseRig> m_rig_records;
    std::vector<hipr::RigBook> m_rig_books;
    std::vector<uint32_t> m_rig_mesh;
    struct StagedPose { bool staged = false; std::vector<float> matrices, weights; };
    std::vector<StagedPose> m_staged_poses;
    void pose_rig_rows(uint32_t rig, const float* matrices, const float* weights, HiprVertexGeometry* out) const;
    void apply_staged_poses();      // the recorded poses skinned into m_geometry
    std::vector<MeshRecord> m_meshes;
    std::vector<uint32_t> m_indices;
    std::vector<HiprVertexGeometry> m_geometry;
    std::vector<float> m_texcoords, m_emissions;
    std::vector<uint32_t> m_tints;
    bool m_any_texcoords = false, m_any_tints = false, m_any_emission = false;
    std::vector<HiprMaterial> m_materials;
    std::vector<HiprLight> m_lights;
    std::vector<HiprTexture> m_textures;
    std::vector<uint8_t> m_texels;
    std::vector<HiprInstance> m_instances;
    std::vector<uint32_t> m_instance_mesh;
    std::vector<HiprTriangle> m_triangles;
    BvhBuildResult m_bvh;
    Bvh2Source m_bvh2_source;
    Wide8Source m_wide8_source;
    Wide4Source m_wide4_source;
    CollapseCounts m_wide4_collapse_counts;
    BuildCounts m_build_counts;
    CollapseCounts m_collapse_counts;
    double m_built_bvh_area = 0.0;
    uint32_t m_bvh_max_depth_limit = 62;
    mutable std::vector<float> m_draw_points;      // staged_environment_build: the draw points of the last sample count asked for
    std::vector<float> m_environment_PDF;
    std::vector<HiprLightSample> m_environment_samples;
    HiprEnvironment m_environment = {};
    bool m_has_environment = false;
    HiprSceneDesc m_desc = {};
    HiprSceneState m_state = {};
    AABB m_bounds = AABB::invalid();
};

// Fills the matrices of HiprCameraState the way prepare_camera_state does (OptiXRenderer/Renderer.cpp:1207-1248)
// from a perspective camera (Bifrost/Scene/Camera.cpp:237-266 compute_perspective_projection).
HiprCameraState make_camera_state(const CameraDescription& camera, float aspect_ratio, uint32_t accumulations, float path_regularization_PDF_scale);

} // namespace HIPRenderer
