// host/host_api.cpp -- C entry points of the headless driver library (libhiprenderer_host.so).
//
// Python (tests, bench.py) drives the C++ host code through these; they hold no rendering logic.
// The scene a handle owns is exactly what a Bifrost host would hand to hipr_upload_scene().
#include "Scenes.h"

#include <algorithm>
#include <cstdio>
#include <exception>
#include <cstring>
#include <string>

#include "HIPRenderer/PresampledEnvironment.h"
#include "HIPRenderer/Renderer.h"
#include "ImageIO/ImageLoader.h"
#include "ImageIO/PngImage.h"
#include "MaterialScene.h"
#include "ObjLoader/ObjLoader.h"
#include "RNG.h"
#include "SceneLoading.h"
#include "glTFLoader/glTFLoader.h"

#include <chrono>
#include <cmath>

using namespace HIPRenderer;

// A small procedural sky for tests and benchmarks: horizon-to-zenith gradient, dark ground, one bright sun disc. 64 x 32 RGBA float.
static void add_procedural_environment(SceneBuilder& sb) {
    using namespace Bifrost;
    const unsigned width = 64, height = 32;
    std::vector<float> pixels(size_t(width) * height * 4);
    const Math::Vector3f sun = Math::normalize(Math::Vector3f(0.4f, 0.7f, -0.3f));
    for (unsigned y = 0; y < height; ++y)
        for (unsigned x = 0; x < width; ++x) {
            const Math::Vector3f direction = Math::latlong_texcoord_to_direction({(x + 0.5f) / width, (y + 0.5f) / height});
            const float up = direction.y;
            float r = up > 0 ? 0.35f + 0.25f * (1 - up) : 0.08f, g = up > 0 ? 0.55f + 0.2f * (1 - up) : 0.07f, b = up > 0 ? 0.9f : 0.06f;
            const float alignment = Math::dot(direction, sun);
            if (alignment > 0.97f) { const float s = (alignment - 0.97f) / 0.03f; r += 60.0f * s; g += 55.0f * s; b += 45.0f * s; }
            float* p = pixels.data() + 4 * (x + size_t(y) * width);
            p[0] = r; p[1] = g; p[2] = b; p[3] = 1.0f;
        }
    const Assets::ImageID image = Assets::Images::create2D("procedural sky", Assets::PixelFormat::RGBA_Float, false, width, height, pixels.data(), pixels.size() * 4);
    const Assets::TextureID texture = Assets::Textures::create2D(image, Assets::MagnificationFilter::Linear, Assets::MinificationFilter::Linear, Assets::WrapMode::Repeat,
                                                                 Assets::WrapMode::Clamp);
    const Assets::InfiniteAreaLight light(texture);
    PresampledEnvironment presampled = presample_environment(light, 1024);
    ImageData data;
    data.width = width; data.height = height; data.format = HIPR_TEXEL_RGBA32F; data.is_sRGB = false;
    data.pixels.assign(reinterpret_cast<const uint8_t*>(pixels.data()), reinterpret_cast<const uint8_t*>(pixels.data()) + pixels.size() * 4);
    const uint32_t texture_index = sb.add_texture(data, true, false, true, true);
    sb.set_environment(texture_index, presampled.pdf_width, presampled.pdf_height, std::move(presampled.per_pixel_PDF), std::move(presampled.samples));
    Assets::Textures::destroy(texture);
    Assets::Images::destroy(image);
}

extern "C" {

// name: "cornell" | "atrium" | "quad" | "empty_ortho". variant bit 1: light the scene with a procedural environment map. variant bit 0: force every material to the Diffuse
// shading model (BASELINE.json config 2). param0/param1: atrium target triangles + seed, ortho width + height.
static void* create_material_scene(const std::string& shader_ball_path, unsigned variant);
static void* create_glass_scene(const std::string& resource_directory, unsigned variant);
static void* create_opacity_scene(unsigned quads_per_edge, unsigned variant);

// The builders hand a worker thread's exception (std::bad_alloc on a scene too large for the host) to the caller: every entry that reaches
// finalize() / refit_bvh() turns it into its error value here -- nothing may unwind through the C boundary.
static void* scene_create(const char* name, unsigned variant, unsigned param0, unsigned param1);
void* hiprh_scene_create(const char* name, unsigned variant, unsigned param0, unsigned param1) {
    try { return scene_create(name, variant, param0, param1); }
    catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_create: %s\n", e.what()); Bifrost::deallocate_all(); return nullptr; }
}
static void* scene_create(const char* name, unsigned variant, unsigned param0, unsigned param1) {
    if (!name) return nullptr;
    if (!std::strncmp(name, "material", 8) && (name[8] == 0 || name[8] == ':')) return create_material_scene(name[8] ? name + 9 : "", variant);
    if (!std::strncmp(name, "glass", 5) && (name[5] == 0 || name[5] == ':')) return create_glass_scene(name[5] ? name + 6 : "", variant);
    if (!std::strcmp(name, "opacity")) return create_opacity_scene(param0, variant);
    SceneBuilder* sb = new SceneBuilder();
    std::string n = name;
    if (n == "cornell") Scenes::create_cornell_box(*sb, param0 ? param0 : 1u);   // param0: quads per wall edge
    else if (n == "atrium") Scenes::create_atrium(*sb, param0 ? param0 : 260000u, param1 ? param1 : 1u, (variant & 16u) != 0);      // variant bit 4: textured, with cut-out banners
    else if (n == "quad") Scenes::create_quad_scene(*sb, param0, param1);
    else if (n == "empty_ortho") Scenes::create_empty_ortho_scene(*sb, param0, param1, RGB(0.1f, 0.5f, 2.0f));
    else { delete sb; return nullptr; }
    if (variant & 1u) sb->force_shading_model(HIPR_SHADING_DIFFUSE);
    if (variant & 2u) add_procedural_environment(*sb);
    if (variant & 8u)   // a spot light as well (tests): a disc of radius 0.04 below the ceiling, a 35 degree cone aimed at the short box
        sb->add_light(SceneBuilder::spot_light(Vector3f(0.2f, 0.42f, -0.1f), Bifrost::Math::normalize(Vector3f(-0.35f, -1.0f, 0.15f)), RGB(1.5f, 1.2f, 0.9f), 0.04f, std::cos(35.0f * 3.14159265f / 180.0f)));
    sb->finalize();
    return sb;
}

// "material" | "material:<path to Shaderball.gltf>": SimpleViewer's material test scene (BASELINE.json config 3) built in the
// Bifrost managers and flattened, with the viewer's clip planes and its 32 bounces (apps/SimpleViewer/main.cpp:353,428-429).
// variant bit 0: all materials Diffuse; bit 2: the coated variant. The Bifrost managers are scratch space here.
static void* create_material_scene(const std::string& shader_ball_path, unsigned variant) {
    using namespace Bifrost;
    deallocate_all();
    Scene::SceneRoot scene = Scene::SceneRoot("Model scene", RGB(0.68f, 0.92f, 1.0f));
    const Scene::CameraID camera_ID = Scene::Cameras::create("Camera", scene.get_ID(), Math::Matrix4x4f::identity(), Math::Matrix4x4f::identity());
    ViewerScenes::create_material_scene(camera_ID, scene.get_root_node(), shader_ball_path, (variant & 4u) != 0);
    if (Assets::MeshModels::get_iterable().size() < 2) { deallocate_all(); return nullptr; }     // the shader ball did not load
    const SceneLoading::ViewerDefaults defaults = SceneLoading::apply_viewer_defaults(scene.get_root_node(), camera_ID, false);
    if (variant & 1u)
        for (Assets::MaterialID material_ID : Assets::Materials::get_iterable()) Assets::Material(material_ID).set_shading_model(Assets::ShadingModel::Diffuse);

    SceneBuilder* sb = new SceneBuilder();
    sb->set_environment_tint(Scene::SceneRoots::get_environment_tint(scene.get_ID()));
    flatten_bifrost_scene(*sb);
    sb->camera.transform = Scene::Cameras::get_transform(camera_ID);
    sb->camera.near_plane = defaults.near_plane;
    sb->camera.far_plane = defaults.far_plane;
    sb->camera.max_bounce_count = 32;
    deallocate_all();
    return sb;
}

// "glass" | "glass:<directory with Shaderball.gltf and Diamond.glb>": the transmissive part of the viewer's glass scene
// (apps/SimpleViewer/Scenes/Glass.cpp), flattened like the material scene; procedural stand-ins without the directory.
static void* create_glass_scene(const std::string& resource_directory, unsigned variant) {
    using namespace Bifrost;
    deallocate_all();
    Scene::SceneRoot scene = Scene::SceneRoot("Model scene", RGB(0.68f, 0.92f, 1.0f));
    const Scene::CameraID camera_ID = Scene::Cameras::create("Camera", scene.get_ID(), Math::Matrix4x4f::identity(), Math::Matrix4x4f::identity());
    const std::string shader_ball = resource_directory.empty() ? "" : resource_directory + "/Shaderball.gltf", diamond = resource_directory.empty() ? "" : resource_directory + "/Diamond.glb";
    ViewerScenes::create_glass_scene(camera_ID, scene.get_root_node(), shader_ball, diamond);
    if (Assets::MeshModels::get_iterable().size() < 5) { deallocate_all(); return nullptr; }     // floor, ball (2), lens, handle, diamond
    const SceneLoading::ViewerDefaults defaults = SceneLoading::apply_viewer_defaults(scene.get_root_node(), camera_ID, false);
    if (variant & 1u)
        for (Assets::MaterialID material_ID : Assets::Materials::get_iterable()) Assets::Material(material_ID).set_shading_model(Assets::ShadingModel::Diffuse);

    SceneBuilder* sb = new SceneBuilder();
    sb->set_environment_tint(Scene::SceneRoots::get_environment_tint(scene.get_ID()));
    flatten_bifrost_scene(*sb);
    sb->camera.transform = Scene::Cameras::get_transform(camera_ID);
    sb->camera.near_plane = defaults.near_plane;
    sb->camera.far_plane = defaults.far_plane;
    sb->camera.max_bounce_count = 32;
    deallocate_all();
    return sb;
}

// "opacity": the viewer's opacity scene (apps/SimpleViewer/Scenes/Opacity.h), the reference's test bed for cut-outs and partial
// coverage. param0 = quads per edge of the box and the planes (1 = as the viewer builds it: 24 triangles).
static void* create_opacity_scene(unsigned quads_per_edge, unsigned variant) {
    using namespace Bifrost;
    deallocate_all();
    Scene::SceneRoot scene = Scene::SceneRoot("Model scene", RGB(0.68f, 0.92f, 1.0f));
    const Scene::CameraID camera_ID = Scene::Cameras::create("Camera", scene.get_ID(), Math::Matrix4x4f::identity(), Math::Matrix4x4f::identity());
    ViewerScenes::create_opacity_scene(camera_ID, scene.get_root_node(), quads_per_edge);
    const SceneLoading::ViewerDefaults defaults = SceneLoading::apply_viewer_defaults(scene.get_root_node(), camera_ID, false);
    if (variant & 1u)
        for (Assets::MaterialID material_ID : Assets::Materials::get_iterable()) Assets::Material(material_ID).set_shading_model(Assets::ShadingModel::Diffuse);

    SceneBuilder* sb = new SceneBuilder();
    sb->set_environment_tint(Scene::SceneRoots::get_environment_tint(scene.get_ID()));
    flatten_bifrost_scene(*sb);
    sb->camera.transform = Scene::Cameras::get_transform(camera_ID);
    sb->camera.near_plane = defaults.near_plane;
    sb->camera.far_plane = defaults.far_plane;
    sb->camera.max_bounce_count = 32;
    deallocate_all();
    return sb;
}

// A model file (.obj, .gltf, .glb) set up the way SimpleViewer sets up a scene loaded from its command line
// (apps/SimpleViewer/main.cpp:330-429): sky-blue environment tint, cut-out detection, camera placed from the scene bounds,
// the default directional light when the file brings none. Textures: PNG only (ImageIO/PngImage.h). Null when the file
// cannot be loaded. The Bifrost managers are scratch space here: whatever they held is dropped.
void* hiprh_scene_load_with_environment(const char* path, const char* environment_map_path, unsigned variant);
void* hiprh_scene_load(const char* path, unsigned variant) { return hiprh_scene_load_with_environment(path, nullptr, variant); }

// The same with SimpleViewer's --environment-map (main.cpp:331-341, 533): a latitude-longitude image (Radiance .hdr, PNG or JPEG) that lights the
// scene and is seen where paths escape; it counts as a light source, so no default directional light is added (main.cpp:419-426).
static void* scene_load_with_environment(const char* path, const char* environment_map_path, unsigned variant);
void* hiprh_scene_load_with_environment(const char* path, const char* environment_map_path, unsigned variant) {
    // No exception crosses the C boundary: a crafted or truncated asset that exhausts memory inside a decoder costs the load, not the process.
    try { return scene_load_with_environment(path, environment_map_path, variant); }
    catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_load: %s\n", e.what()); Bifrost::deallocate_all(); return nullptr; }
}
static void* scene_load_with_environment(const char* path, const char* environment_map_path, unsigned variant) {
    using namespace Bifrost;
    if (!path) return nullptr;
    deallocate_all();
    Scene::SceneRoot scene = Scene::SceneRoot("Model scene", RGB(0.68f, 0.92f, 1.0f));
    Scene::SceneNode loaded = Scene::SceneNode::invalid();
    if (ObjLoader::file_supported(path)) loaded = ObjLoader::load(path, SceneLoading::load_image);
    else if (glTFLoader::file_supported(path)) loaded = glTFLoader::load(path);
    if (loaded == Scene::SceneNode::invalid()) { deallocate_all(); return nullptr; }
    loaded.set_parent(scene.get_root_node());
    SceneLoading::detect_and_flag_cutout_materials();
    bool has_environment = false;
    if (environment_map_path && environment_map_path[0]) {
        const Assets::TextureID environment = SceneLoading::load_environment_map(environment_map_path);
        if (environment != Assets::TextureID::invalid_UID()) { scene.set_environment_map(environment); has_environment = true; }
    }
    const Scene::CameraID camera_ID = Scene::Cameras::create("Camera", scene.get_ID(), Math::Matrix4x4f::identity(), Math::Matrix4x4f::identity());
    const SceneLoading::ViewerDefaults defaults = SceneLoading::apply_viewer_defaults(scene.get_root_node(), camera_ID, true, has_environment);

    if (variant & 1u)
        for (Assets::MaterialID material_ID : Assets::Materials::get_iterable()) Assets::Material(material_ID).set_shading_model(Assets::ShadingModel::Diffuse);

    SceneBuilder* sb = new SceneBuilder();
    sb->set_environment_tint(Scene::SceneRoots::get_environment_tint(scene.get_ID()));
    flatten_bifrost_scene(*sb);
    sb->camera.transform = Scene::Cameras::get_transform(camera_ID);
    sb->camera.near_plane = defaults.near_plane;
    sb->camera.far_plane = defaults.far_plane;
    deallocate_all();
    return sb;
}

// The plugin path timed end to end (bench.py's `plugin_renderer` key): the atrium built in the Bifrost managers, pulled by
// HIPRenderer::Renderer::handle_updates and rendered by `calls` blocking Renderer::render() calls into a device render target, exactly what
// SimpleViewer's main loop does per frame (apps/SimpleViewer/main.cpp:298-308). out[0] = milliseconds of the timed calls, out[1] = accumulations
// reached, out[2] = flattened triangle count. max_batch: Renderer::set_max_batch_size (1 = one launch per accumulation, the reference's granularity).
// Returns 0, or a negative number when the renderer cannot be created or a call fails. The Bifrost managers are scratch space here.
static int renderer_bench(const char* data_directory, unsigned target_triangles, unsigned width, unsigned height, unsigned warmup_calls, unsigned calls, unsigned max_batch, double* out3);
int hiprh_renderer_bench(const char* data_directory, unsigned target_triangles, unsigned width, unsigned height, unsigned warmup_calls, unsigned calls, unsigned max_batch, double* out3) {
    try { return renderer_bench(data_directory, target_triangles, width, height, warmup_calls, calls, max_batch, out3); }
    catch (const std::exception& e) { fprintf(stderr, "hiprh_renderer_bench: %s\n", e.what()); Bifrost::deallocate_all(); return -5; }
}
static int renderer_bench(const char* data_directory, unsigned target_triangles, unsigned width, unsigned height, unsigned warmup_calls, unsigned calls, unsigned max_batch, double* out3) {
    using namespace Bifrost;
    if (!data_directory || !out3 || !width || !height) return -1;
    deallocate_all();
    Renderer* renderer = Renderer::initialize(0, data_directory);
    if (!renderer) return -2;
    int status = 0;
    {
        Scene::SceneRoot scene = Scene::SceneRoot("Atrium", RGB(0.68f, 0.92f, 1.0f));
        const Scene::CameraID camera_ID = Scene::Cameras::create("Camera", scene.get_ID(), Math::Matrix4x4f::identity(), Math::Matrix4x4f::identity());
        const ViewerScenes::AtriumCamera camera = ViewerScenes::create_atrium_scene(camera_ID, scene.get_root_node(), target_triangles, 1);
        Math::Matrix4x4f projection, inverse_projection;
        Scene::CameraUtils::compute_perspective_projection(camera.near_plane, camera.far_plane, camera.field_of_view, float(width) / float(height), projection, inverse_projection);
        Scene::Cameras::set_projection_matrices(camera_ID, projection, inverse_projection);
        Scene::Cameras::set_renderer_ID(camera_ID, renderer->get_renderer_ID());
        renderer->set_max_bounce_count(camera_ID, camera.max_bounce_count);
        renderer->set_max_batch_size(max_batch);
        renderer->handle_updates();
        reset_all_change_notifications();

        HiprContext* allocator = nullptr;     // the render target the presentation layer would own
        void* target = nullptr;
        if (hipr_create(0, &allocator) != HIPR_OK || hipr_device_malloc(allocator, uint64_t(width) * height * 8, &target) != HIPR_OK) status = -3;
        unsigned int accumulations = 0;
        for (unsigned i = 0; status == 0 && i < warmup_calls; ++i) accumulations = renderer->render(camera_ID, target, width, Math::Vector2i(int(width), int(height)));
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned i = 0; status == 0 && i < calls; ++i) {
            const unsigned int next = renderer->render(camera_ID, target, width, Math::Vector2i(int(width), int(height)));
            if (next != accumulations + 1) status = -4;
            accumulations = next;
        }
        out3[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        out3[1] = double(accumulations);
        unsigned triangles = 0;
        for (Assets::MeshModelID model : Assets::MeshModels::get_iterable()) triangles += Assets::MeshModel(model).get_mesh().get_primitive_count();
        out3[2] = double(triangles);
        if (target) hipr_device_free(allocator, target);
        if (allocator) hipr_destroy(allocator);
    }
    delete renderer;
    deallocate_all();
    return status;
}

// Decodes any image file the loaders read (PNG, JPEG, Radiance HDR) for the codec tests: returns the byte count of the pixels (8 bit or float, rows
// top-down unless `flip`), 0 when the file cannot be decoded; format: 0 = 8 bit, 1 = float.
static size_t image_load(const char* path, int flip, unsigned* width, unsigned* height, unsigned* channels, int* is_float, void* out, size_t capacity);
size_t hiprh_image_load(const char* path, int flip, unsigned* width, unsigned* height, unsigned* channels, int* is_float, void* out, size_t capacity) {
    try { return image_load(path, flip, width, height, channels, is_float, out, capacity); }
    catch (const std::exception& e) { fprintf(stderr, "hiprh_image_load: %s\n", e.what()); return 0; }
}
static size_t image_load(const char* path, int flip, unsigned* width, unsigned* height, unsigned* channels, int* is_float, void* out, size_t capacity) {
    using namespace Bifrost::Assets;
    if (!path) return 0;
    Image image = ImageLoader::load(path);
    if (!image.exists()) return 0;
    const PixelFormat format = image.get_pixel_format();
    const bool floats = format == PixelFormat::Intensity_Float || format == PixelFormat::RGB_Float || format == PixelFormat::RGBA_Float;
    const unsigned w = image.get_width(), h = image.get_height(), c = unsigned(channel_count(format));
    const size_t row = size_t(w) * c * (floats ? 4 : 1), bytes = row * h;
    if (width) *width = w;
    if (height) *height = h;
    if (channels) *channels = c;
    if (is_float) *is_float = floats;
    if (out && capacity >= bytes)
        for (unsigned y = 0; y < h; ++y) std::memcpy(static_cast<char*>(out) + size_t(y) * row, image.get_pixels<char>() + size_t(flip ? y : h - 1 - y) * row, row);
    Images::destroy(image.get_ID());
    return bytes;
}

// Decodes a PNG file into 8 bit pixels (tests: cross-check of the decoder against an independent one). Returns the byte count
// the image needs, 0 when the file cannot be decoded; copies the pixels when `capacity` is large enough. flip: bottom row first.
size_t hiprh_png_load(const char* path, int flip, unsigned* width, unsigned* height, unsigned* channels, unsigned char* out, size_t capacity) {
    using namespace Bifrost::Assets;
    if (!path) return 0;
    Image image = PngImage::load(path);
    if (!image.exists()) return 0;
    const unsigned w = image.get_width(), h = image.get_height(), c = unsigned(channel_count(image.get_pixel_format()));
    const size_t bytes = size_t(w) * h * c;
    if (width) *width = w;
    if (height) *height = h;
    if (channels) *channels = c;
    if (out && capacity >= bytes)
        for (unsigned y = 0; y < h; ++y)
            std::memcpy(out + size_t(y) * w * c, image.get_pixels<unsigned char>() + size_t(flip ? y : h - 1 - y) * w * c, size_t(w) * c);
    Images::destroy(image.get_ID());
    return bytes;
}

// Transform-only update of a built scene (SceneBuilder::update_model_transforms): model `model_index` (1-based, in creation order for the
// built-in scenes) gets the transform translation[3], rotation quaternion xyzw[4], uniform scale. Returns 1 when the BVH was refitted in
// place (topology kept: hipr_update_scene_geometry suffices), 0 when the builder rebuilt the tree (upload the scene again), -1 on error.
int hiprh_scene_move_model(void* scene, unsigned model_index, const float* translation3, const float* rotation4, float scale, double rebuild_threshold) {
    if (!scene || !translation3 || !rotation4) return -1;
    const Transform t(Vector3f(translation3[0], translation3[1], translation3[2]), Bifrost::Math::Quaternionf(rotation4[0], rotation4[1], rotation4[2], rotation4[3]), scale);
    try { return static_cast<SceneBuilder*>(scene)->update_model_transforms({{model_index, t}}, rebuild_threshold > 0.0 ? rebuild_threshold : 1.5) ? 1 : 0; }
    catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_move_model: %s\n", e.what()); return -1; }
}

// The instances model `model_index` is drawn by and the 3x4 object-to-world matrix the pose gives them -- what hipr_refit_scene_transforms takes -- WITHOUT moving
// anything in the scene. Returns the number of instances (written up to `capacity`), -1 on bad arguments.
int hiprh_scene_model_pose(void* scene, unsigned model_index, const float* translation3, const float* rotation4, float scale, unsigned* out_instance_indices, float* out_matrices_12, unsigned capacity) {
    if (!scene || !translation3 || !rotation4) return -1;
    const Transform t(Vector3f(translation3[0], translation3[1], translation3[2]), Bifrost::Math::Quaternionf(rotation4[0], rotation4[1], rotation4[2], rotation4[3]), scale);
    const Bifrost::Math::Matrix3x4f m = Bifrost::Math::to_matrix3x4(t);
    const std::vector<HiprInstance>& instances = static_cast<SceneBuilder*>(scene)->instances();
    unsigned count = 0;
    for (size_t i = 0; i < instances.size(); ++i)
        if (uint32_t(instances[i].instance_id) == ((1u << 30) | model_index)) {
            if (count < capacity && out_instance_indices && out_matrices_12) {
                out_instance_indices[count] = unsigned(i);
                std::memcpy(out_matrices_12 + 12 * size_t(count), m.begin(), 12 * sizeof(float));
            }
            ++count;
        }
    return int(count);
}

// Material-only update of a built scene (SceneBuilder::update_materials): slots of the material pool rewritten, instances given another material; the builder's
// description follows without a rebuild. Returns 1 when done, 0 when an index was out of range (nothing done), -1 on error.
int hiprh_scene_update_materials(void* scene, const HiprMaterialUpdate* materials, unsigned material_count, const HiprInstanceMaterial* assignments, unsigned assignment_count) {
    if (!scene || (material_count && !materials) || (assignment_count && !assignments)) return -1;
    try {
        return static_cast<SceneBuilder*>(scene)->update_materials(std::vector<HiprMaterialUpdate>(materials, materials + material_count),
                                                                   std::vector<HiprInstanceMaterial>(assignments, assignments + assignment_count)) ? 1 : 0;
    } catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_update_materials: %s\n", e.what()); return -1; }
}

// Pixel edit of a texture of a built scene (SceneBuilder::update_texels): the rectangle takes `pixels`, rows `row_pitch_bytes` apart, in the texture's pooled format; the
// builder's description follows without a rebuild. Returns 1 when done, 0 where the device call would refuse (nothing done), -1 on error. out_environment_stale (may be
// null): whether the environment's PDF image and samples lag behind an edit of its map.
int hiprh_scene_update_texels(void* scene, unsigned texture_index, unsigned x, unsigned y, unsigned width, unsigned height, const void* pixels, unsigned long long row_pitch_bytes,
                              int* out_environment_stale) {
    if (!scene) return -1;
    try {
        SceneBuilder* builder = static_cast<SceneBuilder*>(scene);
        const bool done = builder->update_texels(texture_index, x, y, width, height, pixels, row_pitch_bytes);
        if (out_environment_stale) *out_environment_stale = builder->environment_texels_edited() ? 1 : 0;
        return done ? 1 : 0;
    } catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_update_texels: %s\n", e.what()); return -1; }
}

namespace {
std::vector<SceneBuilder::VertexEdit> mesh_vertex_edits(const unsigned* meshes, const HiprVertexEdit* edits, unsigned count) {
    std::vector<SceneBuilder::VertexEdit> out(count);
    for (unsigned k = 0; k < count; ++k) out[k] = {meshes[k], edits[k].first_vertex, edits[k].vertex_count, edits[k].geometry, edits[k].texcoords, edits[k].tints, edits[k].emissions};
    return out;
}
}

// Vertex edits of meshes of a built scene (SceneBuilder::update_vertices), the whole host path: edit k names mesh meshes[k] and, MESH-relative, the range and the
// arrays of edits[k]. Returns 1 when the topology was kept, 0 when the scene was rebuilt, -2 when the edits were refused (nothing touched), -1 on error.
int hiprh_scene_update_vertices(void* scene, const unsigned* meshes, const HiprVertexEdit* edits, unsigned count, double rebuild_threshold) {
    if (!scene || (count && (!meshes || !edits))) return -1;
    try {
        bool refused = false;
        const bool kept = static_cast<SceneBuilder*>(scene)->update_vertices(mesh_vertex_edits(meshes, edits, count), rebuild_threshold > 0.0 ? rebuild_threshold : 1.5, &refused);
        return refused ? -2 : (kept ? 1 : 0);
    } catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_update_vertices: %s\n", e.what()); return -1; }
}

// SceneBuilder::stage_vertex_edits: the pools and the flags are written, the triangles and the trees stay behind (hiprh_scene_desc must not be asked until
// hiprh_scene_apply_staged, hiprh_scene_rebuild or an adoption has caught up); out_pool_edits[0 .. count) are the edits in POOL coordinates, what
// hipr_update_scene_vertices takes. Returns 1, 0 when refused (nothing touched), -1 on error.
int hiprh_scene_stage_vertex_edits(void* scene, const unsigned* meshes, const HiprVertexEdit* edits, unsigned count, HiprVertexEdit* out_pool_edits) {
    if (!scene || (count && (!meshes || !edits || !out_pool_edits))) return -1;
    try {
        std::vector<HiprVertexEdit> pool_edits;
        if (!static_cast<SceneBuilder*>(scene)->stage_vertex_edits(mesh_vertex_edits(meshes, edits, count), pool_edits)) return 0;
        std::copy(pool_edits.begin(), pool_edits.end(), out_pool_edits);
        return 1;
    } catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_stage_vertex_edits: %s\n", e.what()); return -1; }
}

// SceneBuilder::apply_staged_transforms: everything staged reaches the triangles and the trees. Returns 1 when the topology was kept, 0 after a rebuild, -1 on error.
int hiprh_scene_apply_staged(void* scene, double rebuild_threshold) {
    if (!scene) return -1;
    try { return static_cast<SceneBuilder*>(scene)->apply_staged_transforms(rebuild_threshold > 0.0 ? rebuild_threshold : 1.5) ? 1 : 0; }
    catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_apply_staged: %s\n", e.what()); return -1; }
}

// SceneBuilder::vertex_geometry for `count` vertices: positions and (may be null) normals, float3 each, packed as the geometry pool holds them.
int hiprh_vertex_geometry(const float* positions, const float* normals, unsigned count, HiprVertexGeometry* out) {
    if (!positions || !out) return -1;
    for (unsigned v = 0; v < count; ++v) {
        const Vector3f normal = normals ? Vector3f(normals[3 * v], normals[3 * v + 1], normals[3 * v + 2]) : Vector3f(0, 0, 0);
        out[v] = SceneBuilder::vertex_geometry(Vector3f(positions[3 * v], positions[3 * v + 1], positions[3 * v + 2]), normals ? &normal : nullptr);
    }
    return 0;
}

// SceneBuilder::mesh_range: out5 = vertex_offset, vertex_count, index_offset (in triples), primitive_count, flags. Returns 1, 0 for a mesh the scene does not hold.
int hiprh_scene_mesh_range(void* scene, unsigned mesh, unsigned* out5) {
    if (!scene || !out5) return -1;
    uint32_t range[5];
    if (!static_cast<SceneBuilder*>(scene)->mesh_range(mesh, range)) return 0;
    std::copy(range, range + 5, out5);
    return 1;
}

// SceneBuilder::set_rigs: rig k lies over mesh meshes[k], its first_vertex MESH-relative. Returns 1, 0 when refused (nothing touched), -1 on error.
int hiprh_scene_set_rigs(void* scene, const unsigned* meshes, const HiprRigDesc* rigs, unsigned count) {
    if (!scene || (count && (!meshes || !rigs))) return -1;
    try {
        std::vector<SceneBuilder::RigDesc> list(count);
        for (unsigned k = 0; k < count; ++k) list[k] = {meshes[k], rigs[k]};
        return static_cast<SceneBuilder*>(scene)->set_rigs(list) ? 1 : 0;
    } catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_set_rigs: %s\n", e.what()); return -1; }
}

// SceneBuilder::pose_rigs, the whole host path. Returns 1 when the topology was kept, 0 when the scene was rebuilt, -2 when the poses were refused (nothing
// touched), -1 on error.
int hiprh_scene_pose_rigs(void* scene, const HiprRigPose* poses, unsigned count, double rebuild_threshold) {
    if (!scene) return -1;
    try {
        bool refused = false;
        const bool kept = static_cast<SceneBuilder*>(scene)->pose_rigs(std::vector<HiprRigPose>(poses, poses + (poses ? count : 0u)), rebuild_threshold > 0.0 ? rebuild_threshold : 1.5, &refused);
        return refused || (count && !poses) ? -2 : (kept ? 1 : 0);
    } catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_pose_rigs: %s\n", e.what()); return -1; }
}

// SceneBuilder::stage_rig_poses: the latest pose of each rig recorded, nothing skinned (hiprh_scene_desc must not be asked until hiprh_scene_apply_staged,
// hiprh_scene_rebuild or an adoption has caught up); out_pool_poses[0 .. count) are the poses as hipr_pose_scene_rigs takes them. Returns 1, 0 when refused.
int hiprh_scene_stage_rig_poses(void* scene, const HiprRigPose* poses, unsigned count, HiprRigPose* out_pool_poses) {
    if (!scene || (count && (!poses || !out_pool_poses))) return -1;
    try {
        std::vector<HiprRigPose> pool_poses;
        if (!static_cast<SceneBuilder*>(scene)->stage_rig_poses(std::vector<HiprRigPose>(poses, poses + count), pool_poses)) return 0;
        std::copy(pool_poses.begin(), pool_poses.end(), out_pool_poses);
        return 1;
    } catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_stage_rig_poses: %s\n", e.what()); return -1; }
}

// SceneBuilder::posed_geometry: the rows of one rig under one pose, rig->vertex_count of them. Returns 1, 0 when the rig or the pose is refused, -1 on error.
int hiprh_posed_geometry(const HiprRigDesc* rig, const HiprRigPose* pose, HiprVertexGeometry* out) {
    if (!rig || !pose || !out) return -1;
    try { return SceneBuilder::posed_geometry(*rig, *pose, out) ? 1 : 0; }
    catch (const std::exception& e) { fprintf(stderr, "hiprh_posed_geometry: %s\n", e.what()); return -1; }
}

// SceneBuilder::rebuild: a fresh tree over the instances and materials as they stand. Returns 0, -1 on error.
int hiprh_scene_rebuild(void* scene) {
    if (!scene) return -1;
    try { static_cast<SceneBuilder*>(scene)->rebuild(); return 0; }
    catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_rebuild: %s\n", e.what()); return -1; }
}

// SceneBuilder::stage_model_transforms for one model: the pose is recorded in the instances, the triangles and the trees stay (hiprh_scene_desc must not be asked
// until hiprh_scene_adopt_trees, hiprh_scene_move_model or hiprh_scene_rebuild has caught up). Returns 1, 0 when the pose turns an instance inside out, -1 on error.
int hiprh_scene_stage_model(void* scene, unsigned model_index, const float* translation3, const float* rotation4, float scale) {
    if (!scene || !translation3 || !rotation4) return -1;
    const Transform t(Vector3f(translation3[0], translation3[1], translation3[2]), Bifrost::Math::Quaternionf(rotation4[0], rotation4[1], rotation4[2], rotation4[3]), scale);
    try {
        std::vector<HiprInstanceTransform> moved;
        return static_cast<SceneBuilder*>(scene)->stage_model_transforms({{model_index, t}}, moved) ? 1 : 0;
    } catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_stage_model: %s\n", e.what()); return -1; }
}

// SceneBuilder::adopt_rebuilt_trees: the trees hipr_rebuild_scene_trees made of the resident scene taken over in place of a rebuild. Returns 1 when adopted, 0 when
// refused (nothing touched), -1 on error.
int hiprh_scene_adopt_trees(void* scene, const HiprBvhNode* nodes, unsigned node_count, const unsigned* order, unsigned deepest, const HiprSlot8* slots, const HiprWide8BuildResult* wide8) {
    if (!scene || !wide8) return -1;
    try { return static_cast<SceneBuilder*>(scene)->adopt_rebuilt_trees(nodes, node_count, order, deepest, slots, *wide8) ? 1 : 0; }
    catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_adopt_trees: %s\n", e.what()); return -1; }
}
// The builder's current order (BvhBuildResult::order): triangle_count words, valid until the scene changes or is destroyed.
const unsigned* hiprh_scene_order(void* scene, unsigned* out_count) {
    if (!scene || !out_count) return nullptr;
    const std::vector<uint32_t>& order = static_cast<SceneBuilder*>(scene)->order();
    *out_count = unsigned(order.size());
    return order.data();
}
// SceneBuilder::remove_model: every instance of the model leaves the instance list; the triangles and the trees stay behind (hiprh_scene_desc must not be asked until
// hiprh_scene_rebuild or hiprh_scene_adopt_edited_trees has caught up). Returns 1, 0 when the scene has no such model, -1 on error.
int hiprh_scene_remove_model(void* scene, unsigned model_index) {
    if (!scene) return -1;
    try { return static_cast<SceneBuilder*>(scene)->remove_model(model_index) ? 1 : 0; }
    catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_remove_model: %s\n", e.what()); return -1; }
}
// SceneBuilder::insert_model: a model of mesh `mesh` and material `material` at `position` of the instance list (past the end: appended), posed as
// hiprh_scene_move_model poses. Returns the model index used, 0 on bad arguments.
unsigned hiprh_scene_insert_model(void* scene, unsigned position, unsigned mesh, unsigned material, const float* translation3, const float* rotation4, float scale, unsigned model_index) {
    if (!scene || !translation3 || !rotation4) return 0;
    SceneBuilder* sb = static_cast<SceneBuilder*>(scene);
    if (mesh >= sb->mesh_count() || material >= sb->materials().size()) return 0;
    const Transform t(Vector3f(translation3[0], translation3[1], translation3[2]), Bifrost::Math::Quaternionf(rotation4[0], rotation4[1], rotation4[2], rotation4[3]), scale);
    try { return sb->insert_model(position, mesh, material, t, model_index); }
    catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_insert_model: %s\n", e.what()); return 0; }
}
// out[0] = mesh, out[1] = material, out[2] = place in the instance list of the model's first instance. Returns 1, 0 when the scene has no such model.
int hiprh_scene_model_info(void* scene, unsigned model_index, unsigned* out3) {
    if (!scene || !out3) return -1;
    return static_cast<const SceneBuilder*>(scene)->model_info(model_index, out3[0], out3[1], out3[2]) ? 1 : 0;
}
// SceneBuilder::staged_instance_edits: the list hipr_edit_scene_instances takes for the edits since the last build, up to `capacity` entries written. Returns the
// length of the list, -2 when the edits are not the device's to apply (a pool has grown, a transform is staged, nothing is built), -1 on error.
int hiprh_scene_staged_edits(void* scene, HiprInstanceEdit* out, unsigned capacity) {
    if (!scene) return -1;
    try {
        std::vector<HiprInstanceEdit> edits;
        if (!static_cast<const SceneBuilder*>(scene)->staged_instance_edits(edits)) return -2;
        if (out) std::copy(edits.begin(), edits.begin() + std::min<size_t>(capacity, edits.size()), out);
        return int(edits.size());
    } catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_staged_edits: %s\n", e.what()); return -1; }
}
// SceneBuilder::adopt_edited_trees: the trees hipr_edit_scene_instances made taken over in place of a rebuild. Returns 1 when adopted, 0 when refused (nothing
// touched), -1 on error.
int hiprh_scene_adopt_edited_trees(void* scene, const HiprBvhNode* nodes, unsigned node_count, const unsigned* order, unsigned order_count, unsigned deepest, const HiprSlot8* slots,
                                   const HiprWide8BuildResult* wide8) {
    if (!scene || !wide8) return -1;
    try { return static_cast<SceneBuilder*>(scene)->adopt_edited_trees(nodes, node_count, order, order_count, deepest, slots, *wide8) ? 1 : 0; }
    catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_adopt_edited_trees: %s\n", e.what()); return -1; }
}
// SceneBuilder::add_mesh from plain arrays: `vertex_count` positions (3 floats each) and, each NULL or one per vertex, normals (3 floats), texcoords (2 floats),
// tints (1 word) and emission (3 floats); `primitive_count` index triples. Returns the mesh index, -1 on error (a null array, an index past the vertices).
int hiprh_scene_add_mesh(void* scene, const float* positions, const float* normals, const float* texcoords, const unsigned* tints, const float* emission, unsigned vertex_count, const unsigned* primitives,
                         unsigned primitive_count) {
    if (!scene || !positions || !primitives || !vertex_count || !primitive_count) return -1;
    for (size_t k = 0; k < 3 * size_t(primitive_count); ++k)
        if (primitives[k] >= vertex_count) return -1;
    try {
        MeshData mesh;
        for (unsigned v = 0; v < vertex_count; ++v) {
            mesh.positions.push_back(Vector3f(positions[3 * v], positions[3 * v + 1], positions[3 * v + 2]));
            if (normals) mesh.normals.push_back(Vector3f(normals[3 * v], normals[3 * v + 1], normals[3 * v + 2]));
            if (texcoords) mesh.texcoords.push_back(Vector2f{texcoords[2 * v], texcoords[2 * v + 1]});
            if (tints) mesh.tints.push_back(tints[v]);
            if (emission) mesh.emission.push_back(Vector3f(emission[3 * v], emission[3 * v + 1], emission[3 * v + 2]));
        }
        for (unsigned p = 0; p < primitive_count; ++p) mesh.primitives.push_back(Vector3ui{primitives[3 * p], primitives[3 * p + 1], primitives[3 * p + 2]});
        return int(static_cast<SceneBuilder*>(scene)->add_mesh(std::move(mesh)));
    } catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_add_mesh: %s\n", e.what()); return -1; }
}
// SceneBuilder::add_material. Returns the material index, -1 on error.
int hiprh_scene_add_material(void* scene, const HiprMaterial* material) {
    if (!scene || !material) return -1;
    try { return int(static_cast<SceneBuilder*>(scene)->add_material(*material)); }
    catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_add_material: %s\n", e.what()); return -1; }
}
// SceneBuilder::add_texture: `pixels` are width x height texels of `format` (HIPR_TEXEL_*), `byte_count` of them. Returns the texture index, -1 on error.
int hiprh_scene_add_texture(void* scene, unsigned width, unsigned height, unsigned format, int is_sRGB, const unsigned char* pixels, unsigned long long byte_count, int repeat_u, int repeat_v,
                            int linear_magnification, int linear_minification) {
    if (!scene || !pixels || !width || !height) return -1;
    const unsigned long long texel = format == HIPR_TEXEL_R8 ? 1u : (format == HIPR_TEXEL_RGBA8 || format == HIPR_TEXEL_R32F ? 4u : (format == HIPR_TEXEL_RGBA32F ? 16u : 0u));
    if (!texel || byte_count != texel * width * height) return -1;
    try {
        ImageData image;
        image.width = width; image.height = height; image.format = uint8_t(format); image.is_sRGB = is_sRGB != 0;
        image.pixels.assign(pixels, pixels + byte_count);
        return int(static_cast<SceneBuilder*>(scene)->add_texture(image, repeat_u != 0, repeat_v != 0, linear_magnification != 0, linear_minification != 0));
    } catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_add_texture: %s\n", e.what()); return -1; }
}
// SceneBuilder::staged_scene_growth: what hipr_append_scene_pools (`out_growth`) and hipr_edit_scene_instances (`out_edits`, up to `capacity` entries written) take
// for everything since the last build or adoption. The pointers of `out_growth` hold until the next call of this function on the calling thread and the next
// hiprh_scene_add_* call on the scene. Returns the length of the edit list, -2 when it is not the device's to apply, -1 on error.
int hiprh_scene_staged_growth(void* scene, HiprPoolGrowth* out_growth, HiprInstanceEdit* out_edits, unsigned capacity) {
    if (!scene || !out_growth) return -1;
    try {
        static thread_local SceneBuilder::StagedGrowth staged;
        std::vector<HiprInstanceEdit> edits;
        if (!static_cast<const SceneBuilder*>(scene)->staged_scene_growth(staged, edits)) return -2;
        *out_growth = staged.growth;
        if (out_edits) std::copy(edits.begin(), edits.begin() + std::min<size_t>(capacity, edits.size()), out_edits);
        return int(edits.size());
    } catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_staged_growth: %s\n", e.what()); return -1; }
}
// A scene given an environment from raw pixels through the HOST path, the way add_procedural_environment does: the image and the texture in the Bifrost managers,
// InfiniteAreaLight + presample_environment over them, SceneBuilder::add_texture + set_environment. `format` HIPR_TEXEL_RGBA8 or HIPR_TEXEL_RGBA32F. The caller
// rebuilds (hiprh_scene_rebuild) before it reads the description. Returns the texture index, -1 on error.
int hiprh_scene_add_environment(void* scene, unsigned width, unsigned height, unsigned format, int is_sRGB, const unsigned char* pixels, unsigned long long byte_count, int repeat_u, int repeat_v,
                                int linear_magnification, int linear_minification, unsigned sample_count) {
    if (!scene || !pixels || !width || !height || (format != HIPR_TEXEL_RGBA8 && format != HIPR_TEXEL_RGBA32F)) return -1;
    if (byte_count != (format == HIPR_TEXEL_RGBA8 ? 4ull : 16ull) * width * height) return -1;
    try {
        using namespace Bifrost;
        const Assets::ImageID image = Assets::Images::create2D("environment", format == HIPR_TEXEL_RGBA8 ? Assets::PixelFormat::RGBA32 : Assets::PixelFormat::RGBA_Float, is_sRGB != 0, width, height,
                                                               pixels, size_t(byte_count));
        const Assets::TextureID texture = Assets::Textures::create2D(image, linear_magnification ? Assets::MagnificationFilter::Linear : Assets::MagnificationFilter::None,
                                                                     linear_minification ? Assets::MinificationFilter::Linear : Assets::MinificationFilter::None,
                                                                     repeat_u ? Assets::WrapMode::Repeat : Assets::WrapMode::Clamp, repeat_v ? Assets::WrapMode::Repeat : Assets::WrapMode::Clamp);
        const Assets::InfiniteAreaLight light(texture);
        PresampledEnvironment presampled = presample_environment(light, sample_count);
        ImageData data;
        data.width = width; data.height = height; data.format = uint8_t(format); data.is_sRGB = is_sRGB != 0;
        data.pixels.assign(pixels, pixels + byte_count);
        SceneBuilder* sb = static_cast<SceneBuilder*>(scene);
        const uint32_t texture_index = sb->add_texture(data, repeat_u != 0, repeat_v != 0, linear_magnification != 0, linear_minification != 0);
        sb->set_environment(texture_index, presampled.pdf_width, presampled.pdf_height, std::move(presampled.per_pixel_PDF), std::move(presampled.samples));
        Assets::Textures::destroy(texture);
        Assets::Images::destroy(image);
        return int(texture_index);
    } catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_add_environment: %s\n", e.what()); return -1; }
}
// SceneBuilder::add_light (the host path: the caller rebuilds) and SceneBuilder::set_lights (a built scene's list replaced in place). 1 / 0 = done / refused, -1 on error.
int hiprh_scene_add_light(void* scene, const HiprLight* light) {
    if (!scene || !light) return -1;
    try { static_cast<SceneBuilder*>(scene)->add_light(*light); return 1; }
    catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_add_light: %s\n", e.what()); return -1; }
}
int hiprh_scene_set_lights(void* scene, const HiprLight* lights, unsigned count) {
    if (!scene || (count && !lights)) return -1;
    try { return static_cast<SceneBuilder*>(scene)->set_lights(std::vector<HiprLight>(lights, lights + count)) ? 1 : 0; }
    catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_set_lights: %s\n", e.what()); return -1; }
}
const HiprLight* hiprh_scene_lights(void* scene, unsigned* out_count) {
    if (!scene || !out_count) return nullptr;
    const std::vector<HiprLight>& lights = static_cast<SceneBuilder*>(scene)->lights();
    *out_count = unsigned(lights.size());
    return lights.data();
}
// SceneBuilder::staged_environment_build: what hipr_update_scene_lighting takes to build the environment of `texture_index`. The pointers of `out_build` hold until the
// next call of this function on the calling thread. 1 / 0 = staged / not a texture of the scene, -1 on error.
int hiprh_scene_staged_environment_build(void* scene, unsigned texture_index, unsigned sample_count, HiprEnvironmentBuild* out_build) {
    if (!scene || !out_build) return -1;
    try {
        static thread_local SceneBuilder::StagedEnvironmentBuild staged;
        if (!static_cast<const SceneBuilder*>(scene)->staged_environment_build(texture_index, sample_count, staged)) return 0;
        *out_build = staged.build;
        return 1;
    } catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_staged_environment_build: %s\n", e.what()); return -1; }
}
// SceneBuilder::adopt_lighting: the outcome of a hipr_update_scene_lighting taken over. `per_pixel_PDF` and `samples` are read for HIPR_ENVIRONMENT_BUILD only, with the
// extents `result` reports. 1 / 0 = adopted / refused, -1 on error.
int hiprh_scene_adopt_lighting(void* scene, const HiprLight* lights, unsigned count, int environment_action, unsigned texture_index, const HiprLightingResult* result, const float* per_pixel_PDF,
                               const HiprLightSample* samples) {
    if (!scene || !result || (count && !lights)) return -1;
    try {
        std::vector<float> pdf;
        std::vector<HiprLightSample> drawn;
        if (environment_action == HIPR_ENVIRONMENT_BUILD) {
            if (!per_pixel_PDF || !samples) return -1;
            pdf.assign(per_pixel_PDF, per_pixel_PDF + size_t(result->pdf_width) * result->pdf_height);
            drawn.assign(samples, samples + result->sample_count);
        }
        return static_cast<SceneBuilder*>(scene)->adopt_lighting(std::vector<HiprLight>(lights, lights + count), environment_action, texture_index, *result, std::move(pdf), std::move(drawn)) ? 1 : 0;
    } catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_adopt_lighting: %s\n", e.what()); return -1; }
}
// out[0] = calls of hiprh_scene_adopt_trees that adopted, out[1] = calls that refused.
int hiprh_scene_rebuild_counts(void* scene, unsigned* out2) {
    if (!scene || !out2) return -1;
    const SceneBuilder* sb = static_cast<SceneBuilder*>(scene);
    out2[0] = sb->rebuild_counts().adopted; out2[1] = sb->rebuild_counts().refused;
    return 0;
}

static int build_bvh2_on_context(void* context, const HiprTriangle* triangles, uint32_t count, uint32_t max_depth, HiprBvhNode* out_nodes, uint32_t node_capacity, uint32_t* out_node_count,
                                 uint32_t* out_order, uint32_t* out_deepest);
static int build_wide8_on_context(void* context, const HiprBvhNode* nodes, uint32_t node_count, const HiprTriangle* triangles, const uint32_t* order, uint32_t triangle_count, HiprSlot8* out_slots,
                                  uint32_t slot_capacity, HiprWide8BuildResult* out);
static int build_wide4_on_context(void* context, const HiprBvhNode* nodes, uint32_t node_count, uint32_t triangle_count, HiprWideNode* out_nodes, uint32_t node_capacity, HiprWide4BuildResult* out);
// Installs hipr_build_bvh2 of `context` (NULL: removes it) as the BVH2 stage of the scene's builds, hipr_build_wide8 as their 8-wide collapse (unless
// device_collapse_wanted() says the host collapses) and hipr_build_wide4 as their 4-wide collapse (where device_collapse4_wanted() says so; the adoptions ask
// it too), and, with a context, rebuilds the scene through them. A decline
// or a device error is silent here: the host's stage builds the same tree. Returns 1 when the device built the BVH2, 0 when the host did, -1 on error.
int hiprh_scene_use_device_builder(void* scene, void* context) {
    if (!scene) return -1;
    SceneBuilder* sb = static_cast<SceneBuilder*>(scene);
    try {
        sb->set_bvh2_source(context ? Bvh2Source{build_bvh2_on_context, context} : Bvh2Source());
        sb->set_wide8_source(context && device_collapse_wanted() ? Wide8Source{build_wide8_on_context, context} : Wide8Source());
        sb->set_wide4_source(context && device_collapse4_wanted() ? Wide4Source{build_wide4_on_context, context} : Wide4Source());
        if (!context) return 0;
        const unsigned before = sb->build_counts().device_builds;
        sb->rebuild();
        return sb->build_counts().device_builds > before ? 1 : 0;
    } catch (const std::exception& e) { fprintf(stderr, "hiprh_scene_use_device_builder: %s\n", e.what()); return -1; }
}
// out[0] = builds whose BVH2 the device made, out[1] = builds where it was asked and the host built instead, out[2] = the longest range the host's last BVH2 stage split at the median.
int hiprh_scene_build_counts(void* scene, unsigned* out3) {
    if (!scene || !out3) return -1;
    const SceneBuilder* sb = static_cast<SceneBuilder*>(scene);
    out3[0] = sb->build_counts().device_builds; out3[1] = sb->build_counts().declined_builds; out3[2] = sb->longest_median_range();
    return 0;
}

// out[0] = builds whose 8-wide tree the device collapsed, out[1] = builds where it was asked and the host collapsed instead.
int hiprh_scene_collapse_counts(void* scene, unsigned* out2) {
    if (!scene || !out2) return -1;
    const SceneBuilder* sb = static_cast<SceneBuilder*>(scene);
    out2[0] = sb->collapse_counts().device_collapses; out2[1] = sb->collapse_counts().declined_collapses;
    return 0;
}

// The same for the 4-wide tree, adoptions included (SceneBuilder::wide4_collapse_counts).
int hiprh_scene_wide4_collapse_counts(void* scene, unsigned* out2) {
    if (!scene || !out2) return -1;
    const SceneBuilder* sb = static_cast<SceneBuilder*>(scene);
    out2[0] = sb->wide4_collapse_counts().device_collapses; out2[1] = sb->wide4_collapse_counts().declined_collapses;
    return 0;
}
// Tests of the source wiring without a device: a Wide4Source that hands back the host's own collapse (mode 1), one that declines with its outputs untouched (mode 2);
// mode 0 removes the source. Nothing is rebuilt here.
static int host_collapse_as_wide4_source(void*, const HiprBvhNode* nodes, uint32_t node_count, uint32_t, HiprWideNode* out_nodes, uint32_t node_capacity, HiprWide4BuildResult* out) {
    uint32_t stack_entries = 0;
    const std::vector<HiprWideNode> wide = collapse_wide4_on_host(nodes, node_count, 1u, stack_entries, nullptr, nullptr);
    if (wide.size() > node_capacity) return HIPR_ERROR_INVALID_ARGUMENT;
    std::copy(wide.begin(), wide.end(), out_nodes);
    out->node_count = uint32_t(wide.size()); out->stack_entries = stack_entries;
    return HIPR_OK;
}
static int declining_wide4_source(void*, const HiprBvhNode*, uint32_t, uint32_t, HiprWideNode*, uint32_t, HiprWide4BuildResult*) { return HIPR_ERROR_UNSUPPORTED; }
int hiprh_scene_set_test_wide4_source(void* scene, int mode) {
    if (!scene || mode < 0 || mode > 2) return -1;
    static_cast<SceneBuilder*>(scene)->set_wide4_source(mode == 1 ? Wide4Source{host_collapse_as_wide4_source, nullptr} : (mode == 2 ? Wide4Source{declining_wide4_source, nullptr} : Wide4Source()));
    return 0;
}
// hipr_build_wide4 of `context` (NULL: removes it) as the 4-wide collapse of the scene's later builds and adoptions, whatever device_collapse4_wanted() says
// (tools/wide4_collapse_probe.py measures both ways; tests install it). Nothing is rebuilt here.
int hiprh_scene_use_device_wide4(void* scene, void* context) {
    if (!scene) return -1;
    static_cast<SceneBuilder*>(scene)->set_wide4_source(context ? Wide4Source{build_wide4_on_context, context} : Wide4Source());
    return 0;
}

// The builder's material and instance arrays (valid until the scene changes or is destroyed).
const HiprMaterial* hiprh_scene_materials(void* scene, unsigned* out_count) {
    if (!scene || !out_count) return nullptr;
    const std::vector<HiprMaterial>& m = static_cast<SceneBuilder*>(scene)->materials();
    *out_count = unsigned(m.size());
    return m.data();
}
const HiprInstance* hiprh_scene_instances(void* scene, unsigned* out_count) {
    if (!scene || !out_count) return nullptr;
    const std::vector<HiprInstance>& i = static_cast<SceneBuilder*>(scene)->instances();
    *out_count = unsigned(i.size());
    return i.data();
}

// Wide8Builder.cpp's quantise_node on one synthetic node (tests of csrc/wide8_refit.h's restatement).
void hiprh_wide8_quantise_node(const float* boxes_8x6, unsigned valid, const float* grid_min3, const float* grid_cell3, HiprNode8* out) {
    HIPRenderer::quantise_wide8_node(boxes_8x6, valid, grid_min3, grid_cell3, *out);
}

// `count` nodes at once: 48 floats of boxes, a valid mask, 6 floats of grid (min xyz, cell xyz) and a 64-byte node each.
void hiprh_wide8_quantise_nodes(const float* boxes, const unsigned* valid, const float* grids, HiprNode8* out, unsigned count) {
    for (unsigned i = 0; i < count; ++i) HIPRenderer::quantise_wide8_node(boxes + 48 * size_t(i), valid[i], grids + 6 * size_t(i), grids + 6 * size_t(i) + 3, out[i]);
}

void hiprh_scene_destroy(void* scene) { delete static_cast<SceneBuilder*>(scene); }

const HiprSceneDesc* hiprh_scene_desc(void* scene) { return scene ? &static_cast<SceneBuilder*>(scene)->desc() : nullptr; }

int hiprh_scene_state(void* scene, HiprSceneState* out) {
    if (!scene || !out) return -1;
    *out = static_cast<SceneBuilder*>(scene)->state();
    return 0;
}

// max_bounce_count < 0 keeps the scene's own default.
int hiprh_scene_camera(void* scene, unsigned width, unsigned height, unsigned accumulations, int max_bounce_count, float pdf_scale, HiprCameraState* out) {
    if (!scene || !out || !width || !height) return -1;
    SceneBuilder* sb = static_cast<SceneBuilder*>(scene);
    CameraDescription cam = sb->camera;
    if (max_bounce_count >= 0) cam.max_bounce_count = unsigned(max_bounce_count);
    *out = make_camera_state(cam, float(width) / float(height), accumulations, pdf_scale);
    return 0;
}

// A camera state for a caller's camera (tests of the camera-ray stage against the reference's ground-truth rays, BifrostTests/Scene/
// CameraTest.h). params14: position[3], rotation quaternion x y z w, field of view, near, far, orthographic flag, ortho width, height, depth.
int hiprh_make_camera(const float* params14, unsigned width, unsigned height, unsigned accumulations, unsigned max_bounce_count, HiprCameraState* out) {
    if (!params14 || !out || !width || !height) return -1;
    CameraDescription cam;
    cam.transform = Transform(Vector3f(params14[0], params14[1], params14[2]), Bifrost::Math::Quaternionf(params14[3], params14[4], params14[5], params14[6]), 1.0f);
    cam.field_of_view = params14[7]; cam.near_plane = params14[8]; cam.far_plane = params14[9];
    cam.orthographic = params14[10] != 0.0f; cam.ortho_width = params14[11]; cam.ortho_height = params14[12]; cam.ortho_depth = params14[13];
    cam.max_bounce_count = max_bounce_count;
    *out = make_camera_state(cam, float(width) / float(height), accumulations, 0.5f);
    return 0;
}

// Stand-alone BVH build over caller triangles (tests): returns a handle owning nodes + order.
struct BvhHandle { BvhBuildResult result; };
void* hiprh_bvh_build(const HiprTriangle* triangles, unsigned count, unsigned max_depth) {
    BvhHandle* h = nullptr;
    try {
        std::vector<HiprTriangle> t(triangles, triangles + count);
        h = new BvhHandle();
        h->result = build_bvh(t, max_depth);
        return h;
    } catch (const std::exception& e) { fprintf(stderr, "hiprh_bvh_build: %s\n", e.what()); delete h; return nullptr; }
}
// hipr_build_bvh2 as a Bvh2Source.
static int build_bvh2_on_context(void* context, const HiprTriangle* triangles, uint32_t count, uint32_t max_depth, HiprBvhNode* out_nodes, uint32_t node_capacity, uint32_t* out_node_count,
                                 uint32_t* out_order, uint32_t* out_deepest) {
    return hipr_build_bvh2(static_cast<HiprContext*>(context), triangles, count, max_depth, out_nodes, node_capacity, out_node_count, out_order, out_deepest);
}
// The same handle with the BVH2 stage built on the device by `context` (hipr_build_bvh2), the collapses on the host. NULL when the device declines or fails -- this entry
// does not fall back: the status is in *out_status (HIPR_ERROR_UNSUPPORTED for a decline) and the message in hipr_last_error().
void* hiprh_bvh_build_on_device(void* context, const HiprTriangle* triangles, unsigned count, unsigned max_depth, int* out_status) {
    BvhHandle* h = nullptr;
    if (out_status) *out_status = HIPR_ERROR_INVALID_ARGUMENT;
    if (!context || !triangles || !count) return nullptr;
    try {
        std::vector<HiprTriangle> t(triangles, triangles + count);
        h = new BvhHandle();
        Bvh2SourceReport report;
        report.fall_back = false;
        h->result = build_bvh(t, max_depth, Bvh2Source{build_bvh2_on_context, context}, &report);
        if (out_status) *out_status = report.asked ? report.status : HIPR_ERROR_UNSUPPORTED;      // not asked: the host builder is configured away from the device's tree
        if (!report.used) { delete h; return nullptr; }
        return h;
    } catch (const std::exception& e) { fprintf(stderr, "hiprh_bvh_build_on_device: %s\n", e.what()); delete h; return nullptr; }
}
// hipr_build_wide8 as a Wide8Source.
static int build_wide8_on_context(void* context, const HiprBvhNode* nodes, uint32_t node_count, const HiprTriangle* triangles, const uint32_t* order, uint32_t triangle_count, HiprSlot8* out_slots,
                                  uint32_t slot_capacity, HiprWide8BuildResult* out) {
    return hipr_build_wide8(static_cast<HiprContext*>(context), nodes, node_count, triangles, order, triangle_count, out_slots, slot_capacity, out);
}
// A handle whose 8-wide tree `context` collapsed on the device (hipr_build_wide8) from the caller's BVH2 and triangles (`order` may be NULL); the handle's other trees
// are empty. NULL when the device declines or fails -- this entry does not fall back: the status is in *out_status and the message in hipr_last_error().
void* hiprh_wide8_build_on_device(void* context, const HiprBvhNode* nodes, unsigned node_count, const HiprTriangle* triangles, const unsigned* order, unsigned triangle_count, int* out_status) {
    BvhHandle* h = nullptr;
    if (out_status) *out_status = HIPR_ERROR_INVALID_ARGUMENT;
    if (!context) return nullptr;
    try {
        const size_t capacity = size_t(std::min<uint64_t>(2ull * std::max(triangle_count, 1u), 0xFFFFFFull));
        std::vector<HiprSlot8> slots(capacity);
        HiprWide8BuildResult built = {};
        const int status = hipr_build_wide8(static_cast<HiprContext*>(context), nodes, node_count, triangles, order, triangle_count, slots.data(), uint32_t(capacity), &built);
        if (out_status) *out_status = status;
        if (status != HIPR_OK) return nullptr;
        h = new BvhHandle();
        slots.resize(built.slot_count);
        Wide8Result& w = h->result.wide8;
        w.slots = std::move(slots);
        w.height = built.height;
        for (int a = 0; a < 3; ++a) { w.grid_min[a] = built.grid_min[a]; w.grid_cell[a] = built.grid_cell[a]; }
        w.node_count = built.node_count; w.leaf_count = built.leaf_count; w.paired_leaves = built.paired_leaves;
        return h;
    } catch (const std::exception& e) { fprintf(stderr, "hiprh_wide8_build_on_device: %s\n", e.what()); delete h; return nullptr; }
}
// hipr_build_wide4 as a Wide4Source.
static int build_wide4_on_context(void* context, const HiprBvhNode* nodes, uint32_t node_count, uint32_t triangle_count, HiprWideNode* out_nodes, uint32_t node_capacity, HiprWide4BuildResult* out) {
    return hipr_build_wide4(static_cast<HiprContext*>(context), nodes, node_count, triangle_count, out_nodes, node_capacity, out);
}
// A handle whose 4-wide tree `context` collapsed on the device (hipr_build_wide4) from the caller's BVH2; the handle's other trees are empty. NULL when the device
// refuses or fails -- this entry does not fall back: the status is in *out_status and the message in hipr_last_error().
void* hiprh_wide4_build_on_device(void* context, const HiprBvhNode* nodes, unsigned node_count, unsigned triangle_count, int* out_status) {
    BvhHandle* h = nullptr;
    if (out_status) *out_status = HIPR_ERROR_INVALID_ARGUMENT;
    if (!context) return nullptr;
    try {
        std::vector<HiprWideNode> wide(std::max(node_count, 1u));
        HiprWide4BuildResult built = {};
        const int status = hipr_build_wide4(static_cast<HiprContext*>(context), nodes, node_count, triangle_count, wide.data(), uint32_t(wide.size()), &built);
        if (out_status) *out_status = status;
        if (status != HIPR_OK) return nullptr;
        h = new BvhHandle();
        wide.resize(built.node_count);
        h->result.wide_nodes = std::move(wide);
        h->result.wide_stack_entries = built.stack_entries;
        return h;
    } catch (const std::exception& e) { fprintf(stderr, "hiprh_wide4_build_on_device: %s\n", e.what()); delete h; return nullptr; }
}
// A handle whose 4-wide tree the HOST's WideCollapse made from the caller's BVH2 (node 0 the root, parents before children) on `threads` threads, the root's budget
// chosen as build_bvh chooses it; the handle's other trees are empty. out2 (may be NULL): nodes that stopped adopting because one more child did not fit, the budget.
void* hiprh_wide4_collapse(const HiprBvhNode* nodes, unsigned node_count, unsigned threads, unsigned* out2) {
    BvhHandle* h = nullptr;
    if (!nodes || !node_count) return nullptr;
    try {
        h = new BvhHandle();
        uint32_t did_not_fit = 0, budget = 0;
        h->result.wide_nodes = collapse_wide4_on_host(nodes, node_count, threads, h->result.wide_stack_entries, &did_not_fit, &budget);
        if (out2) { out2[0] = did_not_fit; out2[1] = budget; }
        return h;
    } catch (const std::exception& e) { fprintf(stderr, "hiprh_wide4_collapse: %s\n", e.what()); delete h; return nullptr; }
}
// quantise_children of host/BvhBuilder.cpp over `groups` child-box groups (tests of csrc/wide4_build.h's exponent search): boxes = 4 x (lo xyz, hi xyz) floats per
// group, counts = children per group (1 .. 4).
void hiprh_wide4_quantise_children(const float* boxes, const unsigned* counts, unsigned groups, HiprWideNode* out) {
    for (unsigned g = 0; g < groups; ++g) HIPRenderer::quantise_wide4_children(boxes + 24 * size_t(g), counts[g], out[g]);
}
// The handle's 8-wide tree: slots, height, grid (min xyz, cell xyz) and counters (nodes, leaf records, records of two triangles).
const HiprSlot8* hiprh_bvh_wide8_slots(void* h) { return static_cast<BvhHandle*>(h)->result.wide8.slots.data(); }
unsigned hiprh_bvh_wide8_slot_count(void* h) { return unsigned(static_cast<BvhHandle*>(h)->result.wide8.slots.size()); }
unsigned hiprh_bvh_wide8_height(void* h) { return static_cast<BvhHandle*>(h)->result.wide8.height; }
void hiprh_bvh_wide8_grid(void* h, float* out6) {
    const Wide8Result& w = static_cast<BvhHandle*>(h)->result.wide8;
    for (int a = 0; a < 3; ++a) { out6[a] = w.grid_min[a]; out6[3 + a] = w.grid_cell[a]; }
}
void hiprh_bvh_wide8_counts(void* h, unsigned* out3) {
    const Wide8Result& w = static_cast<BvhHandle*>(h)->result.wide8;
    out3[0] = w.node_count; out3[1] = w.leaf_count; out3[2] = w.paired_leaves;
}
// Test-only counters of the host's BVH2 stage: the ranges it split at the median and the longest of them.
unsigned hiprh_bvh_median_splits(void* h) { return static_cast<BvhHandle*>(h)->result.median_splits; }
unsigned hiprh_bvh_longest_median_range(void* h) { return static_cast<BvhHandle*>(h)->result.longest_median_range; }
unsigned hiprh_bvh_node_count(void* h) { return unsigned(static_cast<BvhHandle*>(h)->result.nodes.size()); }
unsigned hiprh_bvh_max_depth(void* h) { return static_cast<BvhHandle*>(h)->result.max_depth; }
const HiprBvhNode* hiprh_bvh_nodes(void* h) { return static_cast<BvhHandle*>(h)->result.nodes.data(); }
const unsigned* hiprh_bvh_order(void* h) { return static_cast<BvhHandle*>(h)->result.order.data(); }
unsigned hiprh_bvh_wide_node_count(void* h) { return unsigned(static_cast<BvhHandle*>(h)->result.wide_nodes.size()); }
unsigned hiprh_bvh_wide_stack_entries(void* h) { return static_cast<BvhHandle*>(h)->result.wide_stack_entries; }
const HiprWideNode* hiprh_bvh_wide_nodes(void* h) { return static_cast<BvhHandle*>(h)->result.wide_nodes.data(); }
// The host's progressive multi-jittered blue-noise points (host/RNG.cpp), for the cross-check against the oracle's generator.
void hiprh_pmjbn_samples(float* out_xy, unsigned count, unsigned candidates) {
    Bifrost::Math::RNG::fill_progressive_multijittered_bluenoise_samples(reinterpret_cast<Bifrost::Math::Vector2f*>(out_xy), reinterpret_cast<Bifrost::Math::Vector2f*>(out_xy) + count, candidates);
}
void hiprh_bvh_destroy(void* h) { delete static_cast<BvhHandle*>(h); }

void hiprh_encode_octahedral(const float* normals_n3, int n, short* out_n2) {
    for (int i = 0; i < n; ++i) {
        Bifrost::Math::OctahedralNormal e = Bifrost::Math::OctahedralNormal::encode_precise({normals_n3[3 * i], normals_n3[3 * i + 1], normals_n3[3 * i + 2]});
        out_n2[2 * i] = e.encoding.x;
        out_n2[2 * i + 1] = e.encoding.y;
    }
}

// The host's environment light over an RGBA float latitude-longitude image: samples (radiance[3], PDF, direction[3], distance)
// for n random pairs, PDF(direction) of those directions, the PDF image's size and, capacity allowing, the per pixel PDF.
// Same argument list as oracle/ref/reference_api.cpp's ref_infinite_area_light, which runs the reference's own class.
int hiprh_infinite_area_light(int width, int height, const float* rgba, const float* u_n2, int n, float* out_samples_n8, float* out_pdf_n, int* out_pdf_size2,
                              float* out_per_pixel_PDF, int per_pixel_capacity) {
    using namespace Bifrost;
    const Assets::ImageID image = Assets::Images::create2D("environment", Assets::PixelFormat::RGBA_Float, false, unsigned(width), unsigned(height), rgba, size_t(width) * height * 16);
    const Assets::TextureID texture = Assets::Textures::create2D(image, Assets::MagnificationFilter::Linear, Assets::MinificationFilter::Linear, Assets::WrapMode::Repeat,
                                                                 Assets::WrapMode::Clamp);
    int status = 0;
    {
        const Assets::InfiniteAreaLight light(texture);
        for (int i = 0; i < n; ++i) {
            const Assets::LightSample s = light.sample({u_n2[2 * i], u_n2[2 * i + 1]});
            float* o = out_samples_n8 + 8 * i;
            o[0] = s.radiance.r; o[1] = s.radiance.g; o[2] = s.radiance.b; o[3] = s.PDF;
            o[4] = s.direction_to_light.x; o[5] = s.direction_to_light.y; o[6] = s.direction_to_light.z; o[7] = s.distance;
            out_pdf_n[i] = light.PDF(s.direction_to_light);
        }
        out_pdf_size2[0] = int(light.get_PDF_width()); out_pdf_size2[1] = int(light.get_PDF_height());
        if (out_per_pixel_PDF && per_pixel_capacity >= out_pdf_size2[0] * out_pdf_size2[1])
            Assets::InfiniteAreaLightUtils::reconstruct_solid_angle_PDF_sans_sin_theta(light, out_per_pixel_PDF);
        else if (out_per_pixel_PDF)
            status = 1;
    }
    Assets::Textures::destroy(texture);
    Assets::Images::destroy(image);
    return status;
}

// The host's software texture lookup (Assets::sample2D); same argument list as oracle/ref/reference_api.cpp's ref_sample2D.
void hiprh_sample2D(int format, int is_sRGB, int width, int height, const void* pixels, int byte_count, int magnification, int minification, int wrap_U, int wrap_V,
                    const float* uv_n2, int n, float* out_n4) {
    using namespace Bifrost::Assets;
    const ImageID image = Images::create2D("texture", PixelFormat(format), is_sRGB != 0, unsigned(width), unsigned(height), pixels, size_t(byte_count));
    const TextureID texture = Textures::create2D(image, MagnificationFilter(magnification), MinificationFilter(minification), WrapMode(wrap_U), WrapMode(wrap_V));
    for (int i = 0; i < n; ++i) {
        const Bifrost::Math::RGBA c = sample2D(texture, {uv_n2[2 * i], uv_n2[2 * i + 1]});
        out_n4[4 * i] = c.r; out_n4[4 * i + 1] = c.g; out_n4[4 * i + 2] = c.b; out_n4[4 * i + 3] = c.a;
    }
    Textures::destroy(texture);
    Images::destroy(image);
}

} // extern "C"
