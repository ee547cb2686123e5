// HIPRenderer/Renderer.cpp -- host side of the MI355X path tracer: scene mirroring + launch.
//
// Follows the behaviour of extensions/OptiXRenderer/OptiXRenderer/Renderer.cpp ("OR/Renderer.cpp"):
//   handle_updates           OR/Renderer.cpp:578-1205  (pull-based scene sync, accumulation reset rules)
//   prepare_camera_state     OR/Renderer.cpp:1207-1248
//   render                   OR/Renderer.cpp:1250-1265
//   request_auxiliary_buffers OR/Renderer.cpp:1267-1358
//   settings accessors       OR/Renderer.cpp:1389-1461
// Where the reference edits an OptiX scene graph incrementally, this host rebuilds the flat HiprSceneDesc
// (world-space triangles + BVH2) whenever geometry, materials or lights changed -- scenes are static between
// edits, and the rebuild is off the render path.
#include "Renderer.h"

#include "PresampledEnvironment.h"
#include "../SceneBuilder.h"
#include "../../../include/hiprenderer_c.h"
#include "../../../include/hipr_denoiser_c.h"

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>

using namespace Bifrost;
using namespace Bifrost::Assets;
using namespace Bifrost::Math;
using namespace Bifrost::Scene;

namespace HIPRenderer {

static const int MAX_RNG_SAMPLE_OFFSETS = 256;   // OR/Renderer.cpp:46

static int entry_of(Backend backend) {
    switch (backend) {
    case Backend::PathTracing: return HIPR_ENTRY_PATH_TRACING;
    case Backend::DepthVisualization: return HIPR_ENTRY_DEPTH;
    case Backend::AlbedoVisualization: return HIPR_ENTRY_ALBEDO;
    case Backend::TintVisualization: return HIPR_ENTRY_TINT;
    case Backend::RoughnessVisualization: return HIPR_ENTRY_ROUGHNESS;
    case Backend::ShadingNormalVisualization: return HIPR_ENTRY_SHADING_NORMAL;
    case Backend::PrimitiveIdVisualization: return HIPR_ENTRY_PRIMITIVE_ID;
    default: return -1;
    }
}

// ---- scene flattening: Bifrost managers -> SceneBuilder -> HiprSceneDesc --------------------------------------------
static HiprMaterial upload_material(MaterialID material_ID) {   // OR/Renderer.cpp:754-812
    HiprMaterial m = {};
    if (material_ID == MaterialID::invalid_UID()) return m;
    Assets::Material host = material_ID;
    m.flags = uint16_t(host.get_flags().raw());
    m.shading_model = uint16_t(host.get_shading_model());
    RGB tint = host.get_tint();
    m.tint[0] = tint.r; m.tint[1] = tint.g; m.tint[2] = tint.b;
    m.tint_roughness_texture_ID = host.has_tint_texture() ? int(host.get_tint_roughness_texture_ID().get_index()) : 0;
    m.roughness = host.get_roughness();
    m.roughness_texture_ID = (m.tint_roughness_texture_ID == 0 && host.has_roughness_texture()) ? int(host.get_tint_roughness_texture_ID().get_index()) : 0;
    m.specularity = host.get_specularity();
    m.metallic = host.get_metallic();
    m.metallic_texture_ID = int(host.get_metallic_texture_ID().get_index());
    m.coat = SceneBuilder::unorm16(host.get_coat());
    m.coat_roughness = SceneBuilder::unorm16(host.get_coat_roughness());
    m.coverage = host.is_cutout() ? host.get_cutout_threshold() : host.get_coverage();
    m.coverage_texture_ID = int(host.get_coverage_texture_ID().get_index());
    RGB e = host.get_emission();
    m.emission[0] = e.r; m.emission[1] = e.g; m.emission[2] = e.b;
    return m;
}

static ImageData convert_image(ImageID image_ID) {   // OR/Renderer.cpp:650-701: RGB24 is expanded to RGBA, alpha 255
    ImageData out;
    out.width = Images::get_width(image_ID);
    out.height = Images::get_height(image_ID);
    out.is_sRGB = Images::is_sRGB(image_ID);
    const size_t n = size_t(out.width) * out.height;
    const uint8_t* src = static_cast<const uint8_t*>(Images::get_pixels(image_ID));
    switch (Images::get_pixel_format(image_ID)) {
    case PixelFormat::Alpha8: case PixelFormat::Intensity8: out.format = HIPR_TEXEL_R8; out.pixels.assign(src, src + n); break;
    case PixelFormat::RGB24:
        out.format = HIPR_TEXEL_RGBA8;
        out.pixels.resize(4 * n);
        for (size_t i = 0; i < n; ++i) { out.pixels[4 * i] = src[3 * i]; out.pixels[4 * i + 1] = src[3 * i + 1]; out.pixels[4 * i + 2] = src[3 * i + 2]; out.pixels[4 * i + 3] = 255; }
        break;
    case PixelFormat::RGBA32: out.format = HIPR_TEXEL_RGBA8; out.pixels.assign(src, src + 4 * n); break;
    case PixelFormat::Intensity_Float: out.format = HIPR_TEXEL_R32F; out.pixels.assign(src, src + 4 * n); break;
    case PixelFormat::RGB_Float: {
        out.format = HIPR_TEXEL_RGBA32F;
        out.pixels.resize(16 * n);
        const float* s = reinterpret_cast<const float*>(src);
        float* d = reinterpret_cast<float*>(out.pixels.data());
        for (size_t i = 0; i < n; ++i) { d[4 * i] = s[3 * i]; d[4 * i + 1] = s[3 * i + 1]; d[4 * i + 2] = s[3 * i + 2]; d[4 * i + 3] = 1.0f; }
        break;
    }
    case PixelFormat::RGBA_Float: out.format = HIPR_TEXEL_RGBA32F; out.pixels.assign(src, src + 16 * n); break;
    default: out.format = HIPR_TEXEL_R8; out.width = out.height = 1; out.pixels.assign(1, 255); break;
    }
    return out;
}

// Dense light array in ID order (light_creation, OR/Renderer.cpp:855-902).
static std::vector<HiprLight> collect_lights() {
    std::vector<HiprLight> lights;
    for (LightSourceID light_ID : LightSources::get_iterable()) {
        Transform t = SceneNodes::get_global_transform(LightSources::get_node_ID(light_ID));
        RGB power = LightSources::get_power(light_ID);
        switch (LightSources::get_type(light_ID)) {
        case LightSources::Type::Sphere: lights.push_back(SceneBuilder::sphere_light(t.translation, power, LightSources::get_radius(light_ID))); break;
        case LightSources::Type::Spot:
            lights.push_back(SceneBuilder::spot_light(t.translation, t.rotation.forward(), power, LightSources::get_radius(light_ID), LightSources::get_cos_angle(light_ID)));
            break;
        case LightSources::Type::Directional: lights.push_back(SceneBuilder::directional_light(t.rotation.forward(), power)); break;
        }
    }
    return lights;
}

// The mesh as SceneBuilder::add_mesh takes it (load_mesh, OR/Renderer.cpp:92-136).
static MeshData mesh_data(Mesh mesh) {
    MeshData data;
    const unsigned int vertex_count = mesh.get_vertex_count(), primitive_count = mesh.get_primitive_count();
    data.positions.assign(mesh.get_positions(), mesh.get_positions() + vertex_count);
    if (mesh.get_normals()) data.normals.assign(mesh.get_normals(), mesh.get_normals() + vertex_count);
    if (mesh.get_texcoords()) data.texcoords.assign(mesh.get_texcoords(), mesh.get_texcoords() + vertex_count);
    if (mesh.get_tint_and_roughness()) {
        data.tints.resize(vertex_count);
        std::memcpy(data.tints.data(), mesh.get_tint_and_roughness(), vertex_count * 4);
    }
    if (mesh.get_emission()) data.emission.assign(mesh.get_emission(), mesh.get_emission() + vertex_count);
    data.primitives.assign(mesh.get_primitives(), mesh.get_primitives() + primitive_count);
    return data;
}

// Textures and materials keep their Bifrost indices (slot 0 = invalid), like the reference's per-ID arrays: the slots from the builder's pool sizes up to the
// managers' capacities are added, dead ones as fillers. A flatten starts from the empty pools; a growth of the resident scene from the pools as they stand.
static void add_textures_and_materials_up_to_capacity(SceneBuilder& sb) {
    for (unsigned int t = unsigned(sb.texture_count()); t < Textures::capacity(); ++t) {
        TextureID id(t);
        ImageData image;
        bool alive = Textures::get_image_ID(id) != ImageID::invalid_UID();
        if (alive) image = convert_image(Textures::get_image_ID(id));
        else { image.width = image.height = 1; image.format = HIPR_TEXEL_R8; image.pixels.assign(1, 255); }
        sb.add_texture(image, Textures::get_wrapmode_U(id) == WrapMode::Repeat, Textures::get_wrapmode_V(id) == WrapMode::Repeat,
                       Textures::get_magnification_filter(id) == MagnificationFilter::Linear, Textures::get_minification_filter(id) != MinificationFilter::None);
    }
    std::vector<bool> material_alive(Materials::capacity(), false);
    for (MaterialID id : Materials::get_iterable()) material_alive[id] = true;
    for (unsigned int m = unsigned(sb.materials().size()); m < Materials::capacity(); ++m) sb.add_material(material_alive[m] ? upload_material(MaterialID(m)) : HiprMaterial{});
}

void flatten_bifrost_scene(SceneBuilder& sb, std::map<unsigned int, uint32_t>& mesh_index) {
    add_textures_and_materials_up_to_capacity(sb);

    // Meshes are added once and shared by the models that reference them (load_mesh, OR/Renderer.cpp:92-136).
    mesh_index.clear();      // kept by the caller: a model created later over one of these meshes is an edit of the resident scene
    for (MeshModelID model_ID : MeshModels::get_iterable()) {
        MeshModel model = model_ID;
        Mesh mesh = model.get_mesh();
        auto it = mesh_index.find(mesh.get_ID());
        if (it == mesh_index.end()) it = mesh_index.emplace(mesh.get_ID(), sb.add_mesh(mesh_data(mesh))).first;
        // create_model: InstanceID = (MeshModel << 30) | model index, material_index = MaterialID index (OR/Renderer.cpp:138-159)
        sb.add_model(it->second, model.get_material().get_ID().get_index(), model.get_scene_node().get_global_transform(), model_ID.get_index());
    }

    for (const HiprLight& light : collect_lights()) sb.add_light(light);
    // Environment map of the scene (OR/Renderer.cpp:1136-1160): only four channel images, importance sampled through presampled lights.
    for (SceneRootID scene_ID : SceneRoots::get_iterable()) {
        const TextureID environment_map = SceneRoots::get_environment_map(scene_ID);
        if (environment_map == TextureID::invalid_UID()) continue;
        const ImageID image = Textures::get_image_ID(environment_map);
        if (channel_count(Images::get_pixel_format(image)) != 4) {
            printf("HIPRenderer only supports environments with 4 channels. '%s' has %u.\n", Images::get_name(image).c_str(), unsigned(channel_count(Images::get_pixel_format(image))));
            continue;
        }
        const InfiniteAreaLight light(environment_map);
        PresampledEnvironment presampled = presample_environment(light);
        sb.set_environment(environment_map.get_index(), presampled.pdf_width, presampled.pdf_height, std::move(presampled.per_pixel_PDF), std::move(presampled.samples));
        break;   // one scene root is rendered
    }
    sb.finalize();
}
void flatten_bifrost_scene(SceneBuilder& sb) {
    std::map<unsigned int, uint32_t> mesh_index;
    flatten_bifrost_scene(sb, mesh_index);
}


struct Renderer::Implementation {
    int device_ID = -1;                 // the device frames are delivered on (= device_IDs[0])
    std::vector<int> device_IDs;        // every device the renderer traces on; tiles are dealt round-robin over them (hipr_group_*)
    Core::RendererID owning_renderer_ID;
    std::vector<float> tables[5];

    struct CameraState {
        HiprGroup* context = nullptr;     // per camera: one C-ABI context (accumulation buffer + queues) on every device of the renderer, as a group
        Vector2i frame_size = {0, 0};
        bool initialized = false;
        unsigned int accumulations = 0, max_accumulation_count = UINT_MAX, max_bounce_count = 4;   // OR/Renderer.cpp:211-221
        Matrix4x4f inverse_view_projection_matrix = Matrix4x4f::identity();
        Backend backend = Backend::None;
        bool scene_uploaded = false;
        bool geometry_update_pending = false;   // the uploaded scene's instances / lights moved: hipr_update_scene_geometry, not a new upload
        // Progressive batching (render()): samples [batch_used, batch_size) of the pass traced from accumulation batch_first are waiting
        // in the context's per-sample radiance buffer; they stay valid while nothing that shaped them changes.
        unsigned int batch_first = 0, batch_size = 0, batch_used = 0;
        HiprCameraState batch_camera = {};
        HiprSceneState batch_scene_state = {};
        int batch_entry = -1;
        void drop_batch() { batch_size = batch_used = 0; }
        // Backend::AIDenoisedPathTracing (OR/IBackend.cpp:19-80): the filter object and the two half4 frames it reads, on the device frames are delivered on
        HiprDenoiser* denoiser = nullptr;
        void *noisy_frame = nullptr, *albedo_frame = nullptr;
        size_t feature_frame_pixels = 0;
    };
    unsigned int max_batch_size = 64;   // accumulations traced together at most (64: 2 % more rays per second than 32 on the 1080p atrium, 128 gains nothing more: profiles/r04_ab_spp_per_pass.txt) (set_max_batch_size; 1 = the reference's one launch per accumulation)
    std::vector<CameraState> per_camera_state = std::vector<CameraState>(1);
    AIDenoiserFlags AI_denoiser_flags = AIDenoiserFlag::Default;
    PathRegularizationSettings path_regularization = {0.5f, 0.0f};   // OR/Renderer.cpp:482-483
    int arithmetic = HIPR_ARITHMETIC_FAST;      // set_arithmetic: applied to every member context of every camera's group
    HiprSceneState scene_state = {{0, 0, 0}, 3};                     // next_event_sample_count = 3, OR/Renderer.cpp:479
    std::unique_ptr<SceneBuilder> scene;
    std::map<unsigned int, uint32_t> scene_mesh_index;      // Bifrost mesh ID -> the scene builder's mesh
    Renderer::SceneUpdateCounts scene_updates = {0, 0, 0, 0, 0, 0, 0, 0};
    Renderer::SceneBuildCounts retired_builds = {0, 0};      // of the scene builders that are gone
    Renderer::SceneCollapseCounts retired_collapses = {0, 0};
    Renderer::SceneRebuildCounts scene_rebuilds = {0, 0};

    bool is_valid() const { return device_ID >= 0; }

    ~Implementation() {
        for (CameraState& c : per_camera_state) {
            if (c.denoiser) hipr_denoiser_destroy(c.denoiser);
            if (c.context) {
                HiprContext* root = hipr_group_context(c.context, 0);
                if (c.noisy_frame) hipr_device_free(root, c.noisy_frame);
                if (c.albedo_frame) hipr_device_free(root, c.albedo_frame);
                hipr_group_destroy(c.context);
            }
        }
    }

    bool conditional_per_camera_state_resize(unsigned int camera_ID) {
        if (per_camera_state.size() <= camera_ID) { per_camera_state.resize(std::max<size_t>(Cameras::capacity(), camera_ID + 1)); return true; }
        return false;
    }

    bool load_tables(const std::filesystem::path& data_directory) {
        std::ifstream f(data_directory / "HIPRenderer" / "shading_tables.bin", std::ios::binary);
        if (!f) return false;
        char magic[8];
        uint32_t counts[5];
        f.read(magic, 8);
        f.read(reinterpret_cast<char*>(counts), sizeof(counts));
        if (!f || std::memcmp(magic, "HIPRTBL1", 8) != 0) return false;
        const uint32_t expected[5] = {1024, 1024, 8192, 8192, 1024};
        for (int i = 0; i < 5; ++i) {
            if (counts[i] != expected[i]) return false;
            tables[i].resize(counts[i]);
            f.read(reinterpret_cast<char*>(tables[i].data()), counts[i] * sizeof(float));
        }
        return bool(f);
    }

    HiprGroup* create_context() {
        HiprGroup* group = nullptr;
        if (hipr_group_create(device_IDs.data(), uint32_t(device_IDs.size()), &group) != HIPR_OK) return nullptr;
        HiprTables t = {tables[0].data(), tables[1].data(), tables[2].data(), tables[3].data(), tables[4].data()};
        if (hipr_group_upload_tables(group, &t) != HIPR_OK) { hipr_group_destroy(group); return nullptr; }
        apply_arithmetic(group);
        return group;
    }

    void apply_arithmetic(HiprGroup* group) {
        for (uint32_t m = 0; m < hipr_group_size(group); ++m) hipr_set_arithmetic(hipr_group_context(group, m), arithmetic);
    }

    // The scene builder goes; what it counted stays (scene_build_counts).
    void retire_scene() {
        if (scene) {
            retired_builds.device_builds += scene->build_counts().device_builds; retired_builds.declined_builds += scene->build_counts().declined_builds;
            retired_collapses.device_collapses += scene->collapse_counts().device_collapses; retired_collapses.declined_collapses += scene->collapse_counts().declined_collapses;
        }
        scene.reset();
    }

    // hipr_group_build_bvh2 as the scene builders' BVH2 stage (SceneBuilder::set_bvh2_source). The source's context is this Implementation, never a camera's group:
    // the group is picked when a build runs -- the first camera that has one NOW -- so a builder that outlives the camera it was first built on (a camera destroyed
    // in handle_updates, a later transform tick that rebuilds) never calls into a destroyed group. With no camera context at that moment the host builds, and the
    // build is counted as declined.
    static int build_bvh2_on_a_live_group(void* implementation, const HiprTriangle* triangles, uint32_t count, uint32_t max_depth, HiprBvhNode* out_nodes, uint32_t node_capacity,
                                          uint32_t* out_node_count, uint32_t* out_order, uint32_t* out_deepest) {
        for (CameraState& c : static_cast<Implementation*>(implementation)->per_camera_state)
            if (c.context) return hipr_group_build_bvh2(c.context, triangles, count, max_depth, out_nodes, node_capacity, out_node_count, out_order, out_deepest);
        return HIPR_ERROR_NOT_READY;
    }

    // hipr_group_build_wide8 as their 8-wide collapse (SceneBuilder::set_wide8_source), by the same rule.
    static int build_wide8_on_a_live_group(void* implementation, const HiprBvhNode* nodes, uint32_t node_count, const HiprTriangle* triangles, const uint32_t* order, uint32_t triangle_count,
                                           HiprSlot8* out_slots, uint32_t slot_capacity, HiprWide8BuildResult* out) {
        for (CameraState& c : static_cast<Implementation*>(implementation)->per_camera_state)
            if (c.context) return hipr_group_build_wide8(c.context, nodes, node_count, triangles, order, triangle_count, out_slots, slot_capacity, out);
        return HIPR_ERROR_NOT_READY;
    }

    // hipr_group_build_wide4 as their 4-wide collapse (SceneBuilder::set_wide4_source), by the same rule.
    static int build_wide4_on_a_live_group(void* implementation, const HiprBvhNode* nodes, uint32_t node_count, uint32_t triangle_count, HiprWideNode* out_nodes, uint32_t node_capacity,
                                           HiprWide4BuildResult* out) {
        for (CameraState& c : static_cast<Implementation*>(implementation)->per_camera_state)
            if (c.context) return hipr_group_build_wide4(c.context, nodes, node_count, triangle_count, out_nodes, node_capacity, out);
        return HIPR_ERROR_NOT_READY;
    }

    void rebuild_scene() {
        retire_scene();
        scene.reset(new SceneBuilder());
        // HIPR_DEVICE_BUILD=1: the BVH2 of every build of this scene builder comes from a camera's contexts (csrc/bvh2_build.h: the host builder's tree, byte for
        // byte; where the device declines the host builds it). Off by default until profiles/device_build_vs_host.txt says otherwise.
        const char* device_build = std::getenv("HIPR_DEVICE_BUILD");
        if (device_build && std::atoi(device_build) != 0) {
            scene->set_bvh2_source(Bvh2Source{build_bvh2_on_a_live_group, this});
            // ... and the 8-wide collapse with it (csrc/wide8_build.h, likewise byte for byte) unless HIPR_DEVICE_COLLAPSE=0 keeps it on the host.
            if (device_collapse_wanted()) scene->set_wide8_source(Wide8Source{build_wide8_on_a_live_group, this});
            // ... and the 4-wide collapse (csrc/wide4_build.h, byte for byte as well) where HIPR_DEVICE_COLLAPSE4 or its default asks for it.
            if (device_collapse4_wanted()) scene->set_wide4_source(Wide4Source{build_wide4_on_a_live_group, this});
        }
        flatten_bifrost_scene(*scene, scene_mesh_index);
        for (CameraState& c : per_camera_state) c.scene_uploaded = false;
    }

    // Transforms that only the devices have seen so far (refit_on_the_device) are applied to the scene builder's arrays before its description is used. The
    // builder judges its BVH2 by its own ratio rule and may rebuild where the 8-wide tree on the devices was still good: every camera then holds a topology
    // the description no longer has and takes the upload again. Returns true when the topology was kept.
    bool apply_staged_transforms() {
        if (!scene || !scene->has_staged_transforms()) return true;
        if (scene->apply_staged_transforms()) return true;
        for (CameraState& c : per_camera_state) { c.scene_uploaded = false; c.geometry_update_pending = false; c.drop_batch(); }
        return false;
    }

    bool upload_scene_to(CameraState& c) {
        if (!scene) rebuild_scene();
        apply_staged_transforms();
        if (hipr_group_upload_scene(c.context, &scene->desc()) != HIPR_OK) return false;
        ++scene_updates.uploads;
        c.scene_uploaded = true;
        c.geometry_update_pending = false;
        c.drop_batch();
        return true;
    }

    // The transform-only tick on the device (hipr_refit_scene_transforms; OR/Renderer.cpp:472,1010-1041: OptiX refits the root acceleration where it lives):
    // the scene builder only records the new matrices -- its triangles and trees are brought up to date when a description is next asked for -- and every
    // camera's contexts recompute the moved triangles and refit the 8-wide tree in place; the lights go along. false: nothing was done, the caller takes the
    // host path (HIPR_DEVICE_REFIT=0, a camera whose scene is not traced through the 8-wide tree or waits for an upload, an instance turned inside out).
    // A refit that stretched the tree past 1.5 times the uploaded tree's child box area -- update_model_transforms' ratio rule, applied to the 8-wide
    // tree -- or that met a leaf record whose triangles parted ends in a rebuild and a full upload.
    bool refit_on_the_device(const std::vector<std::pair<uint32_t, Transform>>& moved_models) {
        // HIPR_DEVICE_REFIT=0 forces the host path. The device path is the default on the strength of profiles/refit_device_vs_host.txt: one moved model of the
        // 251 k atrium 0.41 ms against 32.1 ms, of the 10 M atrium 2.8 ms against 1 589 ms.
        if (const char* v = std::getenv("HIPR_DEVICE_REFIT")) if (std::atoi(v) == 0) return false;
        bool any = false;
        for (CameraState& c : per_camera_state) {
            if (!c.context || !c.scene_uploaded) continue;      // uploads the description later, with everything in it
            int variant = -1;
            if (c.geometry_update_pending || hipr_get_trace_variant(hipr_group_context(c.context, 0), &variant) != HIPR_OK || variant != HIPR_TRACE_WIDE8_PERSISTENT) return false;
            any = true;
        }
        if (!any) return false;
        std::vector<HiprInstanceTransform> moved;
        if (!scene->stage_model_transforms(moved_models, moved)) return false;      // a flip: the host path applies what was staged and rebuilds
        const std::vector<HiprLight>& lights = scene->lights();
        bool rebuild = false;
        for (CameraState& c : per_camera_state) {
            c.drop_batch();
            if (!c.context || !c.scene_uploaded) continue;
            HiprRefitResult result = {};
            const int status = hipr_group_refit_scene_transforms(c.context, moved.data(), uint32_t(moved.size()), lights.data(), uint32_t(lights.size()), &result);
            if (status != HIPR_OK) c.scene_uploaded = false;      // this camera takes the whole description again
            else if (result.needs_rebuild || result.child_half_area > 1.5 * result.uploaded_half_area) rebuild = true;
            else ++scene_updates.device_refits;
        }
        if (rebuild && !rebuild_on_the_device()) {
            scene->rebuild();
            for (CameraState& c : per_camera_state) c.scene_uploaded = false;
        }
        return true;
    }

    // HIPR_DEVICE_REBUILD=1: a move that asks for a rebuild is answered where the triangles already are (hipr_rebuild_scene_trees; csrc/scene_rebuild.h) instead of a
    // flatten, a build and an upload of every pool. The first camera with an uploaded scene rebuilds with outputs and the scene builder adopts them
    // (SceneBuilder::adopt_rebuilt_trees: its description is then what rebuild() leaves); every other uploaded camera rebuilds without outputs -- the same kernels
    // over the same arrays give the same bytes -- and one whose call fails takes the upload. false: a decline before the adoption, or the variable unset; the caller
    // takes the host path whole. Off by default until profiles/device_rebuild_vs_host.txt says otherwise.
    bool rebuild_on_the_device() {
        const char* wanted = std::getenv("HIPR_DEVICE_REBUILD");
        if (!wanted || std::atoi(wanted) == 0) return false;
        CameraState* first = nullptr;
        for (CameraState& c : per_camera_state)
            if (c.context && c.scene_uploaded) { first = &c; break; }
        if (!first) return false;
        const uint32_t n = scene->desc_triangle_count();
        const uint32_t node_capacity = std::max(std::max(n, 1u) - 1u, 1u), slot_capacity = uint32_t(std::min<uint64_t>(2ull * n, 0xFFFFFFull));
        // the pages of this room are touched only where the device's arrays are copied to
        struct Room { void* p; ~Room() { std::free(p); } };
        Room nodes = {std::malloc(size_t(node_capacity) * sizeof(HiprBvhNode))}, order = {std::malloc(size_t(std::max(n, 1u)) * 4)}, slots = {std::malloc(size_t(std::max(slot_capacity, 1u)) * sizeof(HiprSlot8))};
        HiprSceneRebuildResult built = {};
        const bool rebuilt = nodes.p && order.p && slots.p &&
                             hipr_group_rebuild_scene_trees(first->context, scene->bvh_max_depth_limit(), static_cast<HiprBvhNode*>(nodes.p), node_capacity, static_cast<uint32_t*>(order.p),
                                                            static_cast<HiprSlot8*>(slots.p), slot_capacity, &built) == HIPR_OK;
        if (!rebuilt || !scene->adopt_rebuilt_trees(static_cast<const HiprBvhNode*>(nodes.p), built.node_count, static_cast<const uint32_t*>(order.p), built.deepest,
                                                    static_cast<const HiprSlot8*>(slots.p), built.wide8)) {
            ++scene_rebuilds.declined_rebuilds;
            return false;
        }
        for (CameraState& c : per_camera_state) {
            if (&c == first || !c.context || !c.scene_uploaded) continue;
            HiprSceneRebuildResult same = {};
            if (hipr_group_rebuild_scene_trees(c.context, scene->bvh_max_depth_limit(), nullptr, 0, nullptr, nullptr, 0, &same) != HIPR_OK) c.scene_uploaded = false;
        }
        ++scene_rebuilds.device_rebuilds;
        return true;
    }

    // HIPR_DEVICE_INSTANCE_EDIT=1: a tick whose only scene dirt is models created over meshes the builder holds and models destroyed edits the resident scenes
    // (hipr_edit_scene_instances; csrc/instance_edit.h; OR/Renderer.cpp:138-182, :1043-1110 adds or removes a child of the root group) instead of retiring the scene. The
    // instance list is brought into MeshModels iteration order -- the order flatten_bifrost_scene uses -- the first uploaded camera edits with outputs and the scene
    // builder adopts them (SceneBuilder::adopt_edited_trees), every other uploaded camera edits without outputs. false: the caller takes the full path, silently --
    // the variable unset, a camera that is not traced through the 8-wide tree or waits for something, a mesh the builder does not hold, any refusal. The builder may
    // then hold staged edits: the caller retires it. Off by default, as the rebuild path is (profiles/instance_edit_device_vs_host.txt has the figures).
    //
    // `grow` (HIPR_DEVICE_POOL_GROWTH=1, asked for by grow_pools_wanted()): the tick also brings meshes, materials or textures the builder does not hold. They go
    // through the builder's add_* calls -- textures and materials up to the managers' capacities as a flatten adds them, a created model's mesh when the builder has
    // none for it -- and every camera first has the tails appended to its resident pools (hipr_append_scene_pools; csrc/pool_growth.h; OR/Renderer.cpp:92-136
    // load_mesh, :703-812), then edits as above with what SceneBuilder::staged_scene_growth lists. Counted in pool_growths instead.
    static bool grow_pools_wanted() {
        const char* wanted = std::getenv("HIPR_DEVICE_POOL_GROWTH");
        return wanted && std::atoi(wanted) != 0;
    }
    bool edit_instances_on_the_device(bool grow = false) {
        const char* wanted = std::getenv("HIPR_DEVICE_INSTANCE_EDIT");
        if (!(grow ? grow_pools_wanted() : wanted && std::atoi(wanted) != 0) || !scene || scene->has_staged_transforms()) return false;
        CameraState* first = nullptr;
        for (CameraState& c : per_camera_state) {
            if (!c.context || !c.scene_uploaded) continue;      // uploads the description later, with everything in it
            int variant = -1;
            if (c.geometry_update_pending || hipr_get_trace_variant(hipr_group_context(c.context, 0), &variant) != HIPR_OK || variant != HIPR_TRACE_WIDE8_PERSISTENT) return false;
            if (!first) first = &c;
        }
        if (!first) return false;
        const uint32_t triangles_before = scene->desc_triangle_count();
        if (grow) add_textures_and_materials_up_to_capacity(*scene);
        for (MeshModelID model_ID : MeshModels::get_changed_models())
            if (MeshModels::get_changes(model_ID).contains(MeshModels::Change::Destroyed)) scene->remove_model(model_ID.get_index());      // false: created and destroyed since the last tick
        uint32_t rank = 0;
        for (MeshModelID model_ID : MeshModels::get_iterable()) {
            if (MeshModels::get_changes(model_ID).contains(MeshModels::Change::Created)) {
                MeshModel model = model_ID;
                auto mesh = scene_mesh_index.find(model.get_mesh().get_ID());
                const uint32_t material = model.get_material().get_ID().get_index();
                if (mesh == scene_mesh_index.end() && grow) mesh = scene_mesh_index.emplace(model.get_mesh().get_ID(), scene->add_mesh(mesh_data(model.get_mesh()))).first;
                if (mesh == scene_mesh_index.end() || material >= scene->materials().size()) return false;      // a pool would grow
                scene->insert_model(rank, mesh->second, material, model.get_scene_node().get_global_transform(), model_ID.get_index());
            }
            ++rank;
        }
        const std::vector<HiprInstance>& instances = scene->instances();
        if (instances.size() != rank) return false;
        rank = 0;
        for (MeshModelID model_ID : MeshModels::get_iterable())
            if (uint32_t(instances[rank++].instance_id) != ((1u << 30) | model_ID.get_index())) return false;      // not the order a flatten would give
        std::vector<HiprInstanceEdit> edits;
        SceneBuilder::StagedGrowth growth;
        if (!(grow ? scene->staged_scene_growth(growth, edits) : scene->staged_instance_edits(edits)) || edits.empty()) return false;
        uint64_t bound = triangles_before;
        for (const HiprInstanceEdit& e : edits) bound += e.source == HIPR_EDIT_NEW_INSTANCE ? e.primitive_count : 0u;
        const uint32_t n = uint32_t(std::min<uint64_t>(bound, 0xFFFFFFFFull));
        const uint32_t node_capacity = std::max(std::max(n, 1u) - 1u, 1u), slot_capacity = uint32_t(std::min<uint64_t>(2ull * n, 0xFFFFFFull));
        struct Room { void* p; ~Room() { std::free(p); } };
        Room nodes = {std::malloc(size_t(node_capacity) * sizeof(HiprBvhNode))}, order = {std::malloc(size_t(std::max(n, 1u)) * 4)}, slots = {std::malloc(size_t(std::max(slot_capacity, 1u)) * sizeof(HiprSlot8))};
        HiprSceneEditResult edited = {};
        for (CameraState& c : per_camera_state) c.drop_batch();
        const bool done = nodes.p && order.p && slots.p && (!grow || hipr_group_append_scene_pools(first->context, &growth.growth) == HIPR_OK) &&
                          hipr_group_edit_scene_instances(first->context, edits.data(), uint32_t(edits.size()), scene->bvh_max_depth_limit(), static_cast<HiprBvhNode*>(nodes.p), node_capacity,
                                                          static_cast<uint32_t*>(order.p), n, static_cast<HiprSlot8*>(slots.p), slot_capacity, &edited) == HIPR_OK;
        if (!done || !scene->adopt_edited_trees(static_cast<const HiprBvhNode*>(nodes.p), edited.node_count, static_cast<const uint32_t*>(order.p), edited.triangle_count, edited.deepest,
                                                static_cast<const HiprSlot8*>(slots.p), edited.wide8))
            return false;
        for (CameraState& c : per_camera_state) {
            if (&c == first || !c.context || !c.scene_uploaded) continue;
            HiprSceneEditResult same = {};
            if ((grow && hipr_group_append_scene_pools(c.context, &growth.growth) != HIPR_OK) ||
                hipr_group_edit_scene_instances(c.context, edits.data(), uint32_t(edits.size()), scene->bvh_max_depth_limit(), nullptr, 0, nullptr, 0, nullptr, 0, &same) != HIPR_OK)
                c.scene_uploaded = false;
        }
        ++(grow ? scene_updates.pool_growths : scene_updates.instance_edits);
        return true;
    }

    // The material-only tick on the device (hipr_update_scene_materials; OR/Renderer.cpp:753-850: the reference rewrites one slot of its material buffer): the
    // scene builder brings its own description along without a rebuild, and every camera with an uploaded scene has the changed slots copied into its resident
    // pools and the arrays derived from materials rewritten by kernels. A camera that waits for its upload takes the whole description later. false: the caller
    // takes the full path -- a new scene -- which is also what any refusal or error ends in (an index outside the uploaded pools, a scene searched
    // exhaustively, HIPR_DEVICE_MATERIAL_UPDATE=0).
    bool update_materials_on_the_device(const std::vector<HiprMaterialUpdate>& changed, const std::vector<HiprInstanceMaterial>& assignments) {
        // HIPR_DEVICE_MATERIAL_UPDATE=0 forces the full path. The device path is the default on the strength of profiles/material_update_device_vs_host.txt: one
        // material's roughness of the 251 k atrium 0.05 ms against 149 ms for a new scene, of the 10 M atrium 0.39 ms against 2 844 ms.
        if (const char* v = std::getenv("HIPR_DEVICE_MATERIAL_UPDATE")) if (std::atoi(v) == 0) return false;
        if (!scene->update_materials(changed, assignments)) return false;
        for (CameraState& c : per_camera_state) {
            c.drop_batch();
            if (!c.context || !c.scene_uploaded) continue;
            if (hipr_group_update_scene_materials(c.context, changed.data(), uint32_t(changed.size()), assignments.data(), uint32_t(assignments.size())) != HIPR_OK) return false;
            ++scene_updates.material_updates;
        }
        return true;
    }

    // The lighting tick on the device (HIPR_DEVICE_LIGHTING=1, opt-in; hipr_update_scene_lighting; OR/Renderer.cpp:852-1008: the reference rewrites its light buffer
    // in place, :1136-1196: it presamples its environment without touching geometry): light sources created or destroyed, and a scene's environment map set to a
    // texture the resident pools hold. Every camera with an uploaded scene takes the new light list and, for a new map, builds the PDF image and the samples from its
    // resident texels (csrc/environment_build.h) -- the first with outputs, which the scene builder adopts without a rebuild. A camera that waits for its upload takes
    // the whole description later. false: the caller takes the full path -- a new scene -- which is also what any refusal or error ends in. A map whose texture is
    // new in the tick is not taken here: the tick takes the full path.
    static bool device_lighting_wanted() {
        const char* wanted = std::getenv("HIPR_DEVICE_LIGHTING");
        return wanted && std::atoi(wanted) != 0;
    }
    bool update_lighting_on_the_device(TextureID environment_map) {
        if (!scene || scene->has_staged_transforms() || scene->has_staged_edits()) return false;
        CameraState* first = nullptr;
        for (CameraState& c : per_camera_state) {
            if (!c.context || !c.scene_uploaded) continue;      // uploads the description later, with everything in it
            if (c.geometry_update_pending) return false;
            if (!first) first = &c;
        }
        if (!first) return false;
        const std::vector<HiprLight> lights = collect_lights();
        int action = HIPR_ENVIRONMENT_KEEP;
        uint32_t texture_index = 0;
        SceneBuilder::StagedEnvironmentBuild staged;
        std::vector<float> per_pixel_PDF;
        std::vector<HiprLightSample> samples;
        if (environment_map != TextureID::invalid_UID()) {
            const ImageID image = Textures::get_image_ID(environment_map);
            if (channel_count(Images::get_pixel_format(image)) != 4) return false;      // the full path says so and goes without the map
            texture_index = environment_map.get_index();
            if (!scene->staged_environment_build(texture_index, 8192, staged)) return false;      // presample_environment's default count
            action = HIPR_ENVIRONMENT_BUILD;
            per_pixel_PDF.resize(size_t(Images::get_width(image)) * staged.build.pdf_height);
            samples.resize(staged.build.sample_count);
        }
        const HiprEnvironmentBuild* build = action == HIPR_ENVIRONMENT_BUILD ? &staged.build : nullptr;
        for (CameraState& c : per_camera_state) c.drop_batch();
        HiprLightingResult result = {};
        if (hipr_group_update_scene_lighting(first->context, lights.data(), uint32_t(lights.size()), action, build, build ? per_pixel_PDF.data() : nullptr, per_pixel_PDF.size(),
                                             build ? samples.data() : nullptr, uint32_t(samples.size()), &result) != HIPR_OK)
            return false;
        per_pixel_PDF.resize(size_t(result.pdf_width) * result.pdf_height);
        samples.resize(result.sample_count);
        if (!scene->adopt_lighting(lights, action, texture_index, result, action == HIPR_ENVIRONMENT_BUILD ? std::move(per_pixel_PDF) : std::vector<float>(),
                                   action == HIPR_ENVIRONMENT_BUILD ? std::move(samples) : std::vector<HiprLightSample>()))
            return false;
        for (CameraState& c : per_camera_state) {
            if (&c == first || !c.context || !c.scene_uploaded) continue;
            HiprLightingResult same = {};
            if (hipr_group_update_scene_lighting(c.context, lights.data(), uint32_t(lights.size()), action, build, nullptr, 0, nullptr, 0, &same) != HIPR_OK) c.scene_uploaded = false;
        }
        ++scene_updates.lighting_updates;
        return true;
    }

    // The pixel-edit tick on the device (HIPR_DEVICE_TEXEL_UPDATE=1, opt-in: the calls are measured, profiles/texel_update_device_vs_host.txt, the tick through this class is not; hipr_update_scene_texels; the reference asserts
    // "Pixel update not implemented yet", OR/Renderer.cpp:697-698): images whose pixels were rewritten in place (Images::get_mutable_pixels) and that textures inside
    // the uploaded pool show. Every such texture takes ONE rectangle, the whole image, converted as a flatten converts it (convert_image: RGB24 expanded); the scene
    // builder follows without a rebuild (SceneBuilder::update_texels) and every camera with an uploaded scene has the rectangles written into its resident texel pool
    // and the flags that follow texels decided again by kernels. When an edited image is the scene's environment map, the environment is rebuilt on the device in the
    // same tick (update_lighting_on_the_device) -- with HIPR_DEVICE_LIGHTING=1 only; without it the tick takes the full path, so the sky's radiance and its sampling
    // PDF never disagree. false: the caller takes the full path -- a new scene -- which is also what any refusal or error ends in.
    static bool device_texel_update_wanted() {
        const char* wanted = std::getenv("HIPR_DEVICE_TEXEL_UPDATE");
        return wanted && std::atoi(wanted) != 0;
    }
    bool update_texels_on_the_device() {
        if (!scene || scene->has_staged_transforms() || scene->has_staged_edits()) return false;
        for (const CameraState& c : per_camera_state)
            if (c.context && c.scene_uploaded && c.geometry_update_pending) return false;
        TextureID environment_map = TextureID::invalid_UID(), edited_environment_map = TextureID::invalid_UID();
        for (SceneRootID scene_ID : SceneRoots::get_iterable())
            if (SceneRoots::get_environment_map(scene_ID) != TextureID::invalid_UID()) { environment_map = SceneRoots::get_environment_map(scene_ID); break; }      // one scene root is rendered
        struct Whole { uint32_t texture; ImageData image; };
        std::vector<Whole> images;
        for (ImageID image_ID : Images::get_changed_images())
            for (unsigned int t = 1; t < Textures::capacity(); ++t) {
                if (Textures::get_image_ID(TextureID(t)) != image_ID) continue;
                if (t >= scene->texture_count()) return false;
                images.push_back({t, convert_image(image_ID)});
                const HiprTexture& pooled = scene->textures()[t];
                if (pooled.width != images.back().image.width || pooled.height != images.back().image.height || pooled.format != images.back().image.format) return false;
                if (TextureID(t) == environment_map) edited_environment_map = environment_map;
            }
        if (edited_environment_map != TextureID::invalid_UID() && !device_lighting_wanted()) return false;
        std::vector<HiprTexelEdit> edits;
        for (const Whole& w : images) {
            const uint64_t pitch = w.image.pixels.size() / w.image.height;
            if (!scene->update_texels(w.texture, 0, 0, w.image.width, w.image.height, w.image.pixels.data(), pitch)) return false;
            edits.push_back({w.texture, 0u, 0u, w.image.width, w.image.height, w.image.pixels.data(), pitch});
        }
        for (CameraState& c : per_camera_state) {
            c.drop_batch();
            if (!c.context || !c.scene_uploaded || edits.empty()) continue;
            HiprTexelUpdateResult result = {};
            if (hipr_group_update_scene_texels(c.context, edits.data(), uint32_t(edits.size()), &result) != HIPR_OK) return false;
            ++scene_updates.texel_updates;
        }
        return edited_environment_map == TextureID::invalid_UID() || update_lighting_on_the_device(edited_environment_map);
    }

    // ---- handle_updates -----------------------------------------------------------------------------------------------
    void handle_updates() {
        bool should_reset_accumulations = false, scene_dirty = false, models_edited = false;
        // HIPR_DEVICE_POOL_GROWTH=1: meshes created or destroyed, materials created past the builder's pool and images and textures created past it are dirt the
        // resident scene can take at the tails of its pools, where models created or destroyed are the only other dirt of the tick (edit_instances_on_the_device).
        const bool pools_may_grow = scene && grow_pools_wanted();
        bool pools_grow = false;

        for (CameraID cam_ID : Cameras::get_changed_cameras()) {   // OR/Renderer.cpp:581-619
            auto changes = Cameras::get_changes(cam_ID);
            if (changes.contains(Cameras::Change::Destroyed)) {
                if (cam_ID < per_camera_state.size()) {
                    if (per_camera_state[cam_ID].context) hipr_group_destroy(per_camera_state[cam_ID].context);
                    per_camera_state[cam_ID] = CameraState();
                }
                continue;
            }
            bool camera_initialized = per_camera_state.size() > cam_ID && per_camera_state[cam_ID].initialized;
            bool uses_this_renderer = owning_renderer_ID == Cameras::get_renderer_ID(cam_ID);
            bool create = uses_this_renderer && changes.is_set(Cameras::Change::Created);
            bool switch_to = uses_this_renderer && changes.is_set(Cameras::Change::Renderer);
            if (!camera_initialized && (create || switch_to)) {
                conditional_per_camera_state_resize(cam_ID);
                CameraState& state = per_camera_state[cam_ID];
                state.initialized = true;
                state.accumulations = 0;
                state.frame_size = {0, 0};
                if (state.backend == Backend::None) state.backend = Backend::PathTracing;   // preserve a backend set before handle_updates
            }
        }

        for (MeshID mesh_ID : Meshes::get_changed_meshes())
            if (Meshes::get_changes(mesh_ID).any_set(Meshes::Change::Created, Meshes::Change::Destroyed)) {
                (pools_may_grow ? pools_grow : scene_dirty) = true;      // a destroyed mesh's data stays pooled ...
                scene_mesh_index.erase(mesh_ID.get_index());      // ... but its ID is recycled after the tick: whatever mesh carries it from here on is not the one the builder holds
            }
        // HIPR_DEVICE_TEXEL_UPDATE=1: images whose pixels were rewritten, and nothing else of images and textures, are dirt the resident scene can take
        // (update_texels_on_the_device), where they are the tick's only dirt; unset, they make a new scene as they always did.
        bool texels_edited = scene && device_texel_update_wanted() && !Images::get_changed_images().is_empty() && Textures::get_changed_textures().is_empty();
        for (ImageID image_ID : Images::get_changed_images()) texels_edited = texels_edited && Images::get_changes(image_ID) == Images::Change::PixelsUpdated;
        if (!texels_edited && (!Images::get_changed_images().is_empty() || !Textures::get_changed_textures().is_empty())) {
            bool created_past_the_pool = pools_may_grow;
            for (ImageID image_ID : Images::get_changed_images()) created_past_the_pool = created_past_the_pool && Images::get_changes(image_ID) == Images::Change::Created;
            for (TextureID texture_ID : Textures::get_changed_textures())
                created_past_the_pool = created_past_the_pool && Textures::get_changes(texture_ID) == Textures::Change::Created && texture_ID.get_index() >= scene->texture_count();
            (created_past_the_pool ? pools_grow : scene_dirty) = true;
        }

        // Materials (:753-850). A changed material inside the uploaded pool is an edit of the resident scene (update_materials_on_the_device); a pool that grew is a new scene.
        std::vector<HiprMaterialUpdate> changed_materials;
        std::vector<HiprInstanceMaterial> material_assignments;
        bool materials_dirty = false, only_created_materials = true;      // the latter: every entry of changed_materials is a material created in a free slot of the pool
        for (MaterialID material_ID : Materials::get_changed_materials()) {
            auto changes = Materials::get_changes(material_ID);
            if (!changes.any_set(Materials::Change::Created, Materials::Change::Updated, Materials::Change::ShadingModel)) continue;
            should_reset_accumulations = true;
            if (scene && !changes.contains(Materials::Change::Destroyed) && material_ID.get_index() < scene->materials().size())
                { changed_materials.push_back({uint32_t(material_ID.get_index()), upload_material(material_ID)}); only_created_materials = only_created_materials && changes.contains(Materials::Change::Created); }
            else if (pools_may_grow && !changes.contains(Materials::Change::Destroyed)) pools_grow = true;      // created past the pool
            else materials_dirty = true;
        }
        // Lights (:852-1008): created or destroyed lights change the light count (a new scene description); updated ones are replaced in place.
        // HIPR_DEVICE_LIGHTING=1: a changed light count and an environment map set are dirt the resident scene can take (update_lighting_on_the_device), where
        // lighting is the tick's only dirt; unset, they make a new scene as they always did.
        const bool lighting_may_stay = scene && device_lighting_wanted();
        bool lights_recounted = false, lights_moved = false;
        TextureID environment_map_set = TextureID::invalid_UID();
        for (LightSourceID light_ID : LightSources::get_changed_lights()) {
            if (LightSources::get_changes(light_ID).any_set(LightSources::Change::Created, LightSources::Change::Destroyed)) (lighting_may_stay ? lights_recounted : scene_dirty) = true;
            else lights_moved = true;
            should_reset_accumulations = true;
        }

        // Moved nodes (:1010-1041; only nodes that carry renderables or lights matter). The reference updates the node's transform and
        // marks the root acceleration structure dirty, which OptiX REFITS (:472); here the scene's world-space triangles of the moved
        // models are recomputed and the BVH is refitted (SceneBuilder::update_model_transforms), the rest of the scene stays as uploaded.
        std::vector<std::pair<uint32_t, Transform>> moved_models;
        for (SceneNodeID node_ID : SceneNodes::get_changed_nodes()) {
            if (!SceneNodes::get_changes(node_ID).contains(SceneNodes::Change::Transform)) continue;
            for (MeshModelID m : MeshModels::get_iterable())
                if (MeshModels::get_scene_node_ID(m) == node_ID && !MeshModels::get_changes(m).contains(MeshModels::Change::Created)) {      // a created model brings its transform along
                    moved_models.emplace_back(m.get_index(), SceneNodes::get_global_transform(node_ID));
                    should_reset_accumulations = true;
                }
            for (LightSourceID l : LightSources::get_iterable())
                if (LightSources::get_node_ID(l) == node_ID) { lights_moved = true; should_reset_accumulations = true; }
        }
        for (MeshModelID model_ID : MeshModels::get_changed_models()) {   // :1043-1110
            auto changes = MeshModels::get_changes(model_ID);
            if (!changes.any_set(MeshModels::Change::Created, MeshModels::Change::Destroyed, MeshModels::Change::Material)) continue;
            should_reset_accumulations = true;
            if (scene && !changes.any_set(MeshModels::Change::Created, MeshModels::Change::Destroyed)) {      // a model given another material
                const std::vector<HiprInstance>& instances = scene->instances();
                for (size_t i = 0; i < instances.size(); ++i)
                    if (uint32_t(instances[i].instance_id) == ((1u << 30) | model_ID.get_index()))
                        material_assignments.push_back({uint32_t(i), int32_t(MeshModel(model_ID).get_material().get_ID().get_index())});
            } else if (scene) models_edited = true;      // created or destroyed: an edit of the resident scene where that is the tick's only dirt, else a new scene
            else scene_dirty = true;
        }

        for (SceneRootID scene_ID : SceneRoots::get_changed_scenes()) {   // :1112-1200
            auto changes = SceneRoots::get_changes(scene_ID);
            if (changes.contains(SceneRoots::Change::Destroyed)) {
                scene_state.environment_tint[0] = scene_state.environment_tint[1] = scene_state.environment_tint[2] = 0.0f;
                should_reset_accumulations = true;
                continue;
            }
            if (changes.any_set(SceneRoots::Change::EnvironmentMap, SceneRoots::Change::Created) && SceneRoots::get_environment_map(scene_ID) != TextureID::invalid_UID()) {
                if (lighting_may_stay && environment_map_set == TextureID::invalid_UID()) environment_map_set = SceneRoots::get_environment_map(scene_ID);
                else scene_dirty = true;
                should_reset_accumulations = true;
            }
            if (changes.any_set(SceneRoots::Change::EnvironmentTint, SceneRoots::Change::Created)) {
                RGB tint = SceneRoots::get_environment_tint(scene_ID);
                scene_state.environment_tint[0] = tint.r; scene_state.environment_tint[1] = tint.g; scene_state.environment_tint[2] = tint.b;
                should_reset_accumulations = true;
            }
        }

        // Material edits are applied to the resident scene when they are the tick's only dirt; with anything else in the tick, or when the device path declines,
        // they make a new scene as they always did.
        if (materials_dirty) scene_dirty = true;
        // Pixel edits likewise: with any other dirt in the tick, or when the device path declines, they make a new scene.
        if (texels_edited) {
            const bool only_dirt = !scene_dirty && !models_edited && !pools_grow && moved_models.empty() && changed_materials.empty() && material_assignments.empty() && !lights_recounted &&
                                   !lights_moved && environment_map_set == TextureID::invalid_UID();
            if (only_dirt && update_texels_on_the_device()) should_reset_accumulations = true;
            else scene_dirty = true;
        }
        // Lighting edits likewise: with any other dirt in the tick -- a moved model, a material, a model, a pool that grows (the map's own texture included) -- or when
        // the device path declines, they make a new scene.
        if (lights_recounted || environment_map_set != TextureID::invalid_UID()) {
            const bool only_dirt = !scene_dirty && !models_edited && !pools_grow && moved_models.empty() && changed_materials.empty() && material_assignments.empty();
            if (only_dirt && update_lighting_on_the_device(environment_map_set)) lights_moved = false;      // the new list carries the moved lights as well
            else scene_dirty = true;
        }
        // Created and destroyed models likewise: with any other dirt in the tick they make a new scene.
        // (With pools that may grow, a material created in a free slot of the pool is the material edit below, and the models follow it.)
        if (models_edited && (!moved_models.empty() || lights_moved || (!changed_materials.empty() && !(pools_may_grow && pools_grow && only_created_materials)) || !material_assignments.empty())) scene_dirty = true;
        if (!changed_materials.empty() || !material_assignments.empty())
            if (scene_dirty || !scene || !moved_models.empty() || lights_moved || !update_materials_on_the_device(changed_materials, material_assignments)) scene_dirty = true;

        if (pools_grow && !models_edited) scene_dirty = true;      // nothing draws the new data yet: the next scene brings it
        if (models_edited && (scene_dirty || !edit_instances_on_the_device(pools_grow))) scene_dirty = true;

        if (!scene_dirty && scene && (!moved_models.empty() || lights_moved)) {
            // transform-only tick: refit in place; a tree the motion has stretched too far is rebuilt by the scene builder itself
            if (lights_moved && !scene->replace_lights(collect_lights())) scene_dirty = true;      // the light count changed after all
            else if (!refit_on_the_device(moved_models)) {
                const bool topology_kept = moved_models.empty() ? apply_staged_transforms() : scene->update_model_transforms(moved_models);
                for (CameraState& c : per_camera_state) {
                    if (topology_kept) c.geometry_update_pending = c.scene_uploaded;
                    else c.scene_uploaded = false;
                    c.drop_batch();
                }
            }
        }
        if (scene_dirty) retire_scene();   // rebuilt lazily by the next render
        if (scene_dirty)
            for (CameraState& c : per_camera_state) c.scene_uploaded = false;
        if (should_reset_accumulations)
            for (CameraState& c : per_camera_state) c.accumulations = 0;
    }

    // ---- render -------------------------------------------------------------------------------------------------------
    bool prepare_camera_state(CameraID camera_ID, Vector2i frame_size, HiprCameraState& out) {   // OR/Renderer.cpp:1207-1248
        CameraState& state = per_camera_state[camera_ID];
        if (!state.context) {
            state.context = create_context();
            if (!state.context) return false;
        }
        if (!state.scene_uploaded && !upload_scene_to(state)) return false;
        if (state.geometry_update_pending) {
            // nothing is staged here: a pending update is only ever set after update_model_transforms / apply_staged_transforms, and refit_on_the_device stages nothing while one is pending
            if (scene && hipr_group_update_scene_geometry(state.context, &scene->desc()) == HIPR_OK) ++scene_updates.geometry_updates;
            else if (!upload_scene_to(state)) return false;
            state.geometry_update_pending = false;
            state.drop_batch();
        }
        if (frame_size.x != state.frame_size.x || frame_size.y != state.frame_size.y) {
            if (hipr_group_set_frame(state.context, uint32_t(frame_size.x), uint32_t(frame_size.y), 1) != HIPR_OK) return false;
            state.frame_size = frame_size;
            state.accumulations = 0;
            state.drop_batch();
        }
        Matrix4x4f inverse_projection = Cameras::get_inverse_projection_matrix(camera_ID);
        Matrix4x4f inverse_view_projection = Cameras::get_inverse_view_projection_matrix(camera_ID);
        if (state.inverse_view_projection_matrix != inverse_view_projection) state.accumulations = 0;
        state.inverse_view_projection_matrix = inverse_view_projection;

        out = {};
        std::memcpy(out.inverse_projection_matrix, inverse_projection.begin(), sizeof(out.inverse_projection_matrix));
        std::memcpy(out.inverse_view_projection_matrix, inverse_view_projection.begin(), sizeof(out.inverse_view_projection_matrix));
        Matrix3x3f rotation = to_matrix3x3(Cameras::get_inverse_view_transform(camera_ID).rotation);   // holds view -> world (OR/Renderer.cpp:1238-1239)
        std::memcpy(out.view_to_world_rotation, rotation.begin(), sizeof(out.view_to_world_rotation));
        out.accumulations = state.accumulations;
        out.max_bounce_count = state.max_bounce_count;
        out.path_regularization_PDF_scale = path_regularization.PDF_scale;       // PDF_scale_at_accumulation (OR/Renderer.cpp:1244) is evaluated per path on the device
        out.path_regularization_scale_decay = path_regularization.scale_decay;
        return true;
    }

    // The reference traces ONE accumulation per render() (a blocking context->launch, OR/Renderer.cpp:1250-1265). Here the tracing is
    // batched without changing what a call returns: when the samples traced earlier are used up, the next `batch` accumulations are
    // traced in one wavefront pass (hipr_trace_pass) and every render() folds exactly one of them into the running mean and
    // writes the frame (hipr_accumulate_samples) -- bit for bit the image one launch per accumulation gives, since the per-sample
    // radiance and the f64 fold are the same. The batch grows with the accumulation count (1, 1, 1, 1, 2, 3, 4, 6, ... up to
    // max_batch_size), so a camera that keeps moving still gets one accumulation per call, and at most a third of the work done since
    // the last reset is ever thrown away by the next one.
    unsigned int next_batch_size(const CameraState& state) const {
        unsigned int batch = std::max(1u, std::min(max_batch_size, state.accumulations / 2));
        const unsigned int remaining = state.max_accumulation_count - state.accumulations;
        return std::min(batch, std::max(1u, remaining));
    }

    // AIDenoisedBackend::render (OR/IBackend.cpp:62-80) with the reference's command list spelled out: the path tracing launch, whose ray
    // generation program also accumulates the albedo feature image (ORS/SimpleRGPs.cu:149-201) -- here a second, one-segment pass of the
    // HIPR_ENTRY_DENOISER_ALBEDO entry into the context's second running mean --, the filter (the presenting list only: every frame, or the
    // power-of-two and every 32nd frame under LogarithmicFeedback), and copy_to_output with its two debug views. One accumulation per
    // call, not batched: the albedo pass between two folds would overwrite the samples a batch keeps in the path slots.
    unsigned int render_denoised(CameraState& state, const HiprCameraState& camera, void* buffer, unsigned int pitch, Vector2i frame_size) {
        HiprContext* root = hipr_group_context(state.context, 0);
        const size_t pixels = size_t(frame_size.x) * size_t(frame_size.y);
        if (!state.denoiser && hipr_denoiser_create(device_ID, &state.denoiser) != HIPR_OK) { printf("HIPRenderer: cannot create the denoiser.\n"); return state.accumulations; }
        if (pixels > state.feature_frame_pixels) {
            if (state.noisy_frame) hipr_device_free(root, state.noisy_frame);
            if (state.albedo_frame) hipr_device_free(root, state.albedo_frame);
            state.noisy_frame = state.albedo_frame = nullptr; state.feature_frame_pixels = 0;
            if (hipr_device_malloc(root, pixels * 8, &state.noisy_frame) != HIPR_OK || hipr_device_malloc(root, pixels * 8, &state.albedo_frame) != HIPR_OK) return state.accumulations;
            state.feature_frame_pixels = pixels;
        }
        state.drop_batch();
        const uint32_t width = uint32_t(frame_size.x), height = uint32_t(frame_size.y);
        hipr_group_set_scene_state(state.context, &scene_state);
        hipr_group_set_entry_point(state.context, HIPR_ENTRY_PATH_TRACING);
        if (hipr_group_set_samples_per_pass(state.context, 1) != HIPR_OK || hipr_group_trace_pass(state.context, &camera) != HIPR_OK ||
            hipr_group_accumulate_samples(state.context, 0, 1, state.accumulations, state.noisy_frame, width, 1) != HIPR_OK) return state.accumulations;
        hipr_group_set_entry_point(state.context, HIPR_ENTRY_DENOISER_ALBEDO);
        bool albedo_ok = hipr_group_use_scratch_accumulation(state.context, 2) == HIPR_OK && hipr_group_trace_pass(state.context, &camera) == HIPR_OK &&
                         hipr_group_accumulate_samples(state.context, 0, 1, state.accumulations, state.albedo_frame, width, 1) == HIPR_OK;
        hipr_group_use_scratch_accumulation(state.context, 0);
        hipr_group_set_entry_point(state.context, HIPR_ENTRY_PATH_TRACING);
        if (!albedo_ok) return state.accumulations;

        const unsigned int frame_number = state.accumulations + 1;
        const bool presenting = (frame_number & (frame_number - 1)) == 0 || frame_number % 32 == 0 || !AI_denoiser_flags.is_set(AIDenoiserFlag::LogarithmicFeedback);
        const int show = AI_denoiser_flags.is_set(AIDenoiserFlag::VisualizeNoise) ? HIPR_DENOISER_SHOW_NOISE
                       : AI_denoiser_flags.is_set(AIDenoiserFlag::VisualizeAlbedo) ? HIPR_DENOISER_SHOW_ALBEDO : HIPR_DENOISER_SHOW_FILTERED;
        HiprDenoiserSettings settings;
        hipr_denoiser_default_settings(&settings);
        if (hipr_denoiser_process(state.denoiser, &settings, state.noisy_frame, width, state.albedo_frame, width, width, height, presenting ? 1 : 0, show, buffer, pitch) != HIPR_OK ||
            hipr_denoiser_synchronize(state.denoiser) != HIPR_OK) {
            printf("HIPRenderer: denoising failed: %s\n", hipr_denoiser_last_error(state.denoiser));
            return state.accumulations;
        }
        return ++state.accumulations;
    }

    unsigned int render(CameraID camera_ID, void* buffer, unsigned int pitch, Vector2i frame_size) {   // OR/Renderer.cpp:1250-1265
        conditional_per_camera_state_resize(camera_ID);
        HiprCameraState camera;
        if (!prepare_camera_state(camera_ID, frame_size, camera)) return 0;
        CameraState& state = per_camera_state[camera_ID];
        if (state.accumulations >= state.max_accumulation_count) return state.accumulations;
        if (state.backend == Backend::AIDenoisedPathTracing) return render_denoised(state, camera, buffer, pitch, frame_size);
        int entry = entry_of(state.backend);
        entry = entry < 0 ? HIPR_ENTRY_PATH_TRACING : entry;

        // Is the next accumulation already traced, with the settings in force now? (Accumulation resets change `accumulations`;
        // bounce count, regularisation, next event sample count, environment tint and backend take effect immediately as in the reference.)
        HiprCameraState comparable = camera;
        comparable.accumulations = state.batch_camera.accumulations;
        const bool batch_valid = state.batch_used < state.batch_size && state.batch_first + state.batch_used == state.accumulations && state.batch_entry == entry &&
                                 std::memcmp(&comparable, &state.batch_camera, sizeof(HiprCameraState)) == 0 &&
                                 std::memcmp(&scene_state, &state.batch_scene_state, sizeof(HiprSceneState)) == 0;
        if (!batch_valid) {
            const unsigned int batch = next_batch_size(state);
            hipr_group_set_scene_state(state.context, &scene_state);
            hipr_group_set_entry_point(state.context, entry);
            if (hipr_group_set_samples_per_pass(state.context, batch) != HIPR_OK || hipr_group_trace_pass(state.context, &camera) != HIPR_OK) { state.drop_batch(); return state.accumulations; }
            state.batch_first = state.accumulations; state.batch_size = batch; state.batch_used = 0;
            state.batch_camera = camera; state.batch_scene_state = scene_state; state.batch_entry = entry;
        }
        if (hipr_group_accumulate_samples(state.context, state.batch_used, 1, state.accumulations, buffer, pitch, 1) != HIPR_OK) return state.accumulations;   // launch is blocking in the reference
        ++state.batch_used;
        ++state.accumulations;
        return state.accumulations;
    }
};

// ------------------------------------------------------------------------------------------------------------------------
// Renderer
// ------------------------------------------------------------------------------------------------------------------------
Renderer* Renderer::initialize(int device_ID, const std::filesystem::path& data_directory) { return initialize(std::vector<int>{device_ID}, data_directory); }

Renderer* Renderer::initialize(const std::vector<int>& device_IDs, const std::filesystem::path& data_directory) {
    if (device_IDs.empty()) return nullptr;
    Renderer* r = new Renderer(device_IDs, data_directory);
    if (r->m_impl->is_valid()) return r;
    delete r;
    return nullptr;
}

Renderer::Renderer(const std::vector<int>& device_IDs, const std::filesystem::path& data_directory)
    : m_renderer_ID(Core::Renderers::create("HIPRenderer")), m_impl(new Implementation()) {
    m_impl->owning_renderer_ID = m_renderer_ID;
    if (hipr_device_count() == 0) { fprintf(stderr, "HIPRenderer: no HIP device available.\n"); return; }   // OR/Renderer.cpp:280-281
    if (!m_impl->load_tables(data_directory)) { fprintf(stderr, "HIPRenderer failed to initialize: cannot read %s/HIPRenderer/shading_tables.bin\n", data_directory.c_str()); return; }
    m_impl->device_ID = device_IDs[0];
    m_impl->device_IDs = device_IDs;
    HiprGroup* probe = m_impl->create_context();   // fail here, like the OptiX context creation would
    if (!probe) { fprintf(stderr, "HIPRenderer failed to initialize:\n%s\n", hipr_last_error()); m_impl->device_ID = -1; return; }
    const std::string gather = hipr_group_gather_description(probe);
    hipr_group_destroy(probe);
    if (device_IDs.size() == 1) printf("HIPRenderer using HIP device %d.\n", device_IDs[0]);
    else {
        printf("HIPRenderer using %d HIP devices (", int(device_IDs.size()));
        for (size_t i = 0; i < device_IDs.size(); ++i) printf(i ? ", %d" : "%d", device_IDs[i]);
        printf("): 8x8 pixel tiles dealt round-robin, frames assembled on device %d by %s.\n", device_IDs[0], gather.c_str());
    }
}

Renderer::~Renderer() {
    Core::Renderers::destroy(m_renderer_ID);
    delete m_impl;
}

int Renderer::get_next_event_sample_count(SceneRootID) const { return m_impl->scene_state.next_event_sample_count; }
void Renderer::set_next_event_sample_count(SceneRootID, int sample_count) {
    m_impl->scene_state.next_event_sample_count = std::min(sample_count, MAX_RNG_SAMPLE_OFFSETS);   // OR/Renderer.cpp:1390-1392
}

unsigned int Renderer::get_max_bounce_count(CameraID camera_ID) const { m_impl->conditional_per_camera_state_resize(camera_ID); return m_impl->per_camera_state[camera_ID].max_bounce_count; }
void Renderer::set_max_bounce_count(CameraID camera_ID, unsigned int bounce_count) { m_impl->conditional_per_camera_state_resize(camera_ID); m_impl->per_camera_state[camera_ID].max_bounce_count = bounce_count; }

unsigned int Renderer::get_max_accumulation_count(CameraID camera_ID) const { m_impl->conditional_per_camera_state_resize(camera_ID); return m_impl->per_camera_state[camera_ID].max_accumulation_count; }
void Renderer::set_max_accumulation_count(CameraID camera_ID, unsigned int count) { m_impl->conditional_per_camera_state_resize(camera_ID); m_impl->per_camera_state[camera_ID].max_accumulation_count = count; }

Backend Renderer::get_backend(CameraID camera_ID) const { m_impl->conditional_per_camera_state_resize(camera_ID); return m_impl->per_camera_state[camera_ID].backend; }

void Renderer::set_backend(CameraID camera_ID, Backend backend) {   // OR/Renderer.cpp:1417-1455
    if (backend == Backend::None) return;
    m_impl->conditional_per_camera_state_resize(camera_ID);
    auto& state = m_impl->per_camera_state[camera_ID];
    if (backend != Backend::AIDenoisedPathTracing && entry_of(backend) < 0) {
        printf("HIPRenderer: Backend %u not supported.\n", unsigned(backend));
        backend = Backend::AlbedoVisualization;
    }
    state.backend = backend;
    state.accumulations = 0u;
}

PathRegularizationSettings Renderer::get_path_regularization_settings() const { return m_impl->path_regularization; }
void Renderer::set_path_regularization_settings(PathRegularizationSettings settings) { m_impl->path_regularization = settings; }
unsigned int Renderer::get_max_batch_size() const { return m_impl->max_batch_size; }
void Renderer::set_max_batch_size(unsigned int accumulations) { m_impl->max_batch_size = std::max(1u, std::min(accumulations, 256u)); }
Renderer::Arithmetic Renderer::get_arithmetic() const { return m_impl->arithmetic == HIPR_ARITHMETIC_EXACT ? Arithmetic::Exact : Arithmetic::Fast; }
void Renderer::set_arithmetic(Arithmetic arithmetic) {
    const int mode = arithmetic == Arithmetic::Exact ? HIPR_ARITHMETIC_EXACT : HIPR_ARITHMETIC_FAST;
    if (mode == m_impl->arithmetic) return;
    m_impl->arithmetic = mode;
    for (auto& state : m_impl->per_camera_state) {      // the samples traced ahead and the running mean belong to the other estimator
        if (state.context) m_impl->apply_arithmetic(state.context);
        state.drop_batch();
        state.accumulations = 0;
    }
}
AIDenoiserFlags Renderer::get_AI_denoiser_flags() const { return m_impl->AI_denoiser_flags; }
void Renderer::set_AI_denoiser_flags(AIDenoiserFlags flags) { m_impl->AI_denoiser_flags = flags; }

void Renderer::handle_updates() { m_impl->handle_updates(); }

Renderer::SceneUpdateCounts Renderer::scene_update_counts() const { return m_impl->scene_updates; }
Renderer::SceneRebuildCounts Renderer::scene_rebuild_counts() const { return m_impl->scene_rebuilds; }
Renderer::SceneCollapseCounts Renderer::scene_collapse_counts() const {
    SceneCollapseCounts counts = m_impl->retired_collapses;
    if (m_impl->scene) { counts.device_collapses += m_impl->scene->collapse_counts().device_collapses; counts.declined_collapses += m_impl->scene->collapse_counts().declined_collapses; }
    return counts;
}
Renderer::SceneBuildCounts Renderer::scene_build_counts() const {
    SceneBuildCounts counts = m_impl->retired_builds;
    if (m_impl->scene) { counts.device_builds += m_impl->scene->build_counts().device_builds; counts.declined_builds += m_impl->scene->build_counts().declined_builds; }
    return counts;
}

unsigned int Renderer::render(CameraID camera_ID, void* half4_device_buffer, unsigned int buffer_pitch, Vector2i frame_size) {
    return m_impl->render(camera_ID, half4_device_buffer, buffer_pitch, frame_size);
}

bool Renderer::read_accumulation(std::vector<double>& out_rgba) const {
    for (auto& state : m_impl->per_camera_state)
        if (state.context && state.frame_size.x > 0) {
            out_rgba.resize(size_t(state.frame_size.x) * state.frame_size.y * 4);
            return hipr_group_read_accumulation(state.context, out_rgba.data(), out_rgba.size() / 4) == HIPR_OK;
        }
    return false;
}

static float round_through_half(float v) {
    // The reference reads AOV screenshots back from the half4 output buffer (OR/Renderer.cpp:1317-1329):
    // round to binary16 (nearest even) and back. Values here are colours in [0, 1] or small positives.
    uint32_t bits;
    std::memcpy(&bits, &v, 4);
    const uint32_t sign = bits & 0x80000000u;
    bits &= 0x7FFFFFFFu;
    if (bits >= 0x47800000u) bits = bits > 0x7F800000u ? 0x7FC00000u : 0x7F800000u;   // >= 65536 (or inf / nan) -> inf / nan
    else if (bits < 0x38800000u) {                                                       // half subnormal: quantum 2^-24
        float a; std::memcpy(&a, &bits, 4);
        a = std::nearbyintf(a * 16777216.0f) * (1.0f / 16777216.0f);
        std::memcpy(&bits, &a, 4);
    } else {
        const uint32_t lsb = (bits >> 13) & 1u;
        bits = (bits + 0x0FFFu + lsb) & ~0x1FFFu;
        if (bits >= 0x47800000u) bits = 0x7F800000u;
    }
    bits |= sign;
    float out;
    std::memcpy(&out, &bits, 4);
    return out;
}

std::vector<Screenshot> Renderer::request_auxiliary_buffers(CameraID camera_ID, Cameras::ScreenshotContent content_requested, Vector2i frame_size) {
    typedef Screenshot::Content Content;
    std::vector<Screenshot> screenshots;
    const unsigned int supported = unsigned(Content::Depth) | unsigned(Content::Albedo) | unsigned(Content::Tint) | unsigned(Content::Roughness);
    if ((content_requested.raw() & supported) == 0) return screenshots;

    m_impl->conditional_per_camera_state_resize(camera_ID);
    HiprCameraState camera;
    if (!m_impl->prepare_camera_state(camera_ID, frame_size, camera)) return screenshots;
    auto& state = m_impl->per_camera_state[camera_ID];
    const unsigned int accumulation_count = std::max(1u, state.accumulations);
    const int pixel_count = frame_size.x * frame_size.y;
    hipr_group_set_scene_state(state.context, &m_impl->scene_state);

    state.drop_batch();   // the auxiliary passes reuse the context's per-sample radiance buffer
    if (hipr_group_set_samples_per_pass(state.context, 1) != HIPR_OK) return screenshots;
    auto render_auxiliary_feature = [&](int entry, std::vector<double>& accumulation) -> bool {
        if (hipr_group_use_scratch_accumulation(state.context, 1) != HIPR_OK) return false;
        hipr_group_set_entry_point(state.context, entry);
        bool ok = true;
        for (camera.accumulations = 0; ok && camera.accumulations < accumulation_count; ++camera.accumulations)
            ok = hipr_group_trace_pass(state.context, &camera) == HIPR_OK && hipr_group_accumulate_samples(state.context, 0, 1, camera.accumulations, nullptr, 0, 1) == HIPR_OK;
        accumulation.resize(size_t(pixel_count) * 4);
        ok = ok && hipr_group_read_accumulation(state.context, accumulation.data(), pixel_count) == HIPR_OK;
        hipr_group_use_scratch_accumulation(state.context, 0);
        return ok;
    };
    auto unorm8 = [](float v) { v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); return (unsigned char)(v * 255.0f + 0.5f); };

    std::vector<double> acc;
    if (content_requested.is_set(Content::Depth) && render_auxiliary_feature(HIPR_ENTRY_DEPTH, acc)) {
        float* pixels = new float[pixel_count];
        for (int i = 0; i < pixel_count; ++i) pixels[i] = float(acc[4 * i]);
        Screenshot s; s.width = frame_size.x; s.height = frame_size.y; s.content = Content::Depth; s.format = PixelFormat::Intensity_Float; s.pixels = pixels;
        screenshots.push_back(s);
    }
    auto rgb24_screenshot = [&](Content content, int entry) {
        if (!content_requested.is_set(content) || !render_auxiliary_feature(entry, acc)) return;
        unsigned char* pixels = new unsigned char[3 * pixel_count];
        for (int i = 0; i < pixel_count; ++i)
            for (int c = 0; c < 3; ++c) pixels[3 * i + c] = unorm8(round_through_half(float(acc[4 * i + c])));
        Screenshot s; s.width = frame_size.x; s.height = frame_size.y; s.content = content; s.format = PixelFormat::RGB24; s.pixels = pixels;
        screenshots.push_back(s);
    };
    rgb24_screenshot(Content::Albedo, HIPR_ENTRY_ALBEDO);
    rgb24_screenshot(Content::Tint, HIPR_ENTRY_TINT);
    if (content_requested.is_set(Content::Roughness) && render_auxiliary_feature(HIPR_ENTRY_ROUGHNESS, acc)) {
        unsigned char* pixels = new unsigned char[pixel_count];
        for (int i = 0; i < pixel_count; ++i) pixels[i] = unorm8(round_through_half(float(acc[4 * i])));
        Screenshot s; s.width = frame_size.x; s.height = frame_size.y; s.content = Content::Roughness; s.format = PixelFormat::Intensity8; s.pixels = pixels;
        screenshots.push_back(s);
    }
    int entry = entry_of(state.backend);
    hipr_group_set_entry_point(state.context, entry < 0 ? HIPR_ENTRY_PATH_TRACING : entry);
    return screenshots;
}

} // namespace HIPRenderer
