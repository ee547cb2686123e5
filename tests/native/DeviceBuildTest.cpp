// DeviceBuildTest.cpp -- scene builds through HIPRenderer::Renderer with the BVH2 stage on the device (HIPR_DEVICE_BUILD=1, hipr_group_build_bvh2;
// OR/Renderer.cpp:161-182,471-476 asks OptiX for a "Trbvh" build, which runs on the GPU): a scene that gains a model and loses it again is rebuilt twice, and
// every frame must equal, bit for bit in exact arithmetic, the frame of a renderer whose host builds the trees.
#include "MiniTest.h"

#include "../../bifrost3d_amd/host/HIPRenderer/Renderer.h"
#include "../../bifrost3d_amd/host/MaterialScene.h"
#include "../../include/hiprenderer_c.h"

#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>
#include <filesystem>

using namespace Bifrost;

namespace HIPRenderer {

class DeviceBuildFixture {
public:
    bool usable() const { return hipr_device_count() > 0; }
    void SetUp() { deallocate_all(); }
    void TearDown() { deallocate_all(); unsetenv("HIPR_DEVICE_BUILD"); unsetenv("HIPR_DEVICE_REFIT"); }

    static std::filesystem::path data_directory() {   // <repo>/bifrost3d_amd/data, found from the location of this executable
        if (const char* dir = std::getenv("HIPR_DATA_DIRECTORY")) return dir;
        std::error_code error;
        std::filesystem::path executable = std::filesystem::read_symlink("/proc/self/exe", error);
        return executable.parent_path() / ".." / ".." / "bifrost3d_amd" / "data";
    }

    // The small atrium rendered for two accumulations; a copy of one of its models is created, two accumulations; the copy is destroyed, two accumulations.
    // Returns the three accumulations one after the other.
    std::vector<double> render_with_a_model_that_comes_and_goes(bool on_the_device, Renderer::SceneBuildCounts& builds) {
        if (on_the_device) setenv("HIPR_DEVICE_BUILD", "1", 1); else unsetenv("HIPR_DEVICE_BUILD");
        deallocate_all();
        std::vector<double> frames;
        Renderer* renderer = Renderer::initialize(0, data_directory());
        EXPECT_TRUE(renderer != nullptr);
        if (!renderer) return frames;
        renderer->set_arithmetic(Renderer::Arithmetic::Exact);
        {
            const Math::Vector2i frame_size(64, 36);
            Scene::SceneRoot scene = Scene::SceneRoot("Atrium", Math::RGB(0.68f, 0.92f, 1.0f));
            const Scene::CameraID camera_ID = Scene::Cameras::create("Camera", scene.get_ID(), Math::Matrix4x4f::identity(), Math::Matrix4x4f::identity());
            const ViewerScenes::AtriumCamera camera = ViewerScenes::create_atrium_scene(camera_ID, scene.get_root_node(), 6000, 5);
            Math::Matrix4x4f projection, inverse_projection;
            Scene::CameraUtils::compute_perspective_projection(camera.near_plane, camera.far_plane, camera.field_of_view, float(frame_size.x) / float(frame_size.y), projection, inverse_projection);
            Scene::Cameras::set_projection_matrices(camera_ID, projection, inverse_projection);
            Scene::Cameras::set_renderer_ID(camera_ID, renderer->get_renderer_ID());
            renderer->set_max_bounce_count(camera_ID, camera.max_bounce_count);
            void* target = nullptr;
            EXPECT_TRUE(hipMalloc(&target, size_t(frame_size.x) * frame_size.y * 8) == hipSuccess);
            auto tick = [&] {
                renderer->handle_updates();
                const unsigned int iteration = renderer->render(camera_ID, target, frame_size.x, frame_size);
                reset_all_change_notifications();
                return iteration;
            };
            auto keep = [&] {
                std::vector<double> accumulation;
                EXPECT_TRUE(renderer->read_accumulation(accumulation));
                frames.insert(frames.end(), accumulation.begin(), accumulation.end());
            };
            EXPECT_EQ(1u, tick());
            EXPECT_EQ(2u, tick());
            keep();

            // the scene gains a model: a second instance of the first model's mesh, set where the camera sees it
            const Assets::MeshModel first = *Assets::MeshModels::get_iterable().begin();
            Scene::SceneNode node = Scene::SceneNodes::create("Newcomer", Math::Transform(Math::Vector3f(0.3f, 0.4f, 0.2f)));
            node.set_parent(scene.get_root_node());
            const Assets::MeshModelID newcomer = Assets::MeshModels::create(node.get_ID(), first.get_mesh().get_ID(), first.get_material().get_ID());
            EXPECT_EQ(1u, tick());      // restarted
            EXPECT_EQ(2u, tick());
            keep();

            // ... and loses it
            Assets::MeshModels::destroy(newcomer);
            EXPECT_EQ(1u, tick());
            EXPECT_EQ(2u, tick());
            keep();
            builds = renderer->scene_build_counts();
            if (target) (void)hipFree(target);
        }
        delete renderer;
        deallocate_all();
        return frames;
    }
};

GPU_TEST_F(DeviceBuildFixture, a_model_that_comes_and_goes_gives_the_same_frames_with_the_bvh2_built_on_the_device) {
    Renderer::SceneBuildCounts device_builds = {0, 0}, host_builds = {0, 0};
    const std::vector<double> device = render_with_a_model_that_comes_and_goes(true, device_builds);
    const std::vector<double> host = render_with_a_model_that_comes_and_goes(false, host_builds);
    EXPECT_EQ(3u, device_builds.device_builds);      // the first build and the two rebuilds: a camera's contexts exist before its scene is first built
    EXPECT_EQ(0u, device_builds.declined_builds);
    EXPECT_EQ(0u, host_builds.device_builds);      // with the variable unset nothing asks the device
    EXPECT_EQ(0u, host_builds.declined_builds);
    EXPECT_TRUE(!device.empty());
    EXPECT_EQ(device.size(), host.size());
    const size_t frame = device.size() / 3;
    EXPECT_TRUE(frame > 0 && std::memcmp(device.data(), device.data() + frame, frame * sizeof(double)) != 0);      // the newcomer did show in the picture
    size_t different = 0;
    for (size_t i = 0; i < device.size() && i < host.size(); ++i) different += std::memcmp(&device[i], &host[i], sizeof(double)) != 0;
    if (different) fprintf(stderr, "device build vs host build: %zu of %zu accumulated values differ\n", different, device.size());
    EXPECT_EQ(size_t(0), different);
}

// Two cameras; the first one, on whose contexts the scene was first built, is destroyed; then a model is flung far away, which stretches the refitted BVH2 past the
// scene builder's ratio rule, so the SAME scene builder rebuilds. The build must run on the contexts of the camera that is left.
static std::vector<double> render_after_the_first_camera_went(bool on_the_device, Renderer::SceneBuildCounts& builds) {
    if (on_the_device) setenv("HIPR_DEVICE_BUILD", "1", 1); else unsetenv("HIPR_DEVICE_BUILD");
    setenv("HIPR_DEVICE_REFIT", "0", 1);      // the moved model goes through SceneBuilder::update_model_transforms, which rebuilds a stretched tree
    deallocate_all();
    std::vector<double> frame;
    Renderer* renderer = Renderer::initialize(0, DeviceBuildFixture::data_directory());
    EXPECT_TRUE(renderer != nullptr);
    if (!renderer) return frame;
    renderer->set_arithmetic(Renderer::Arithmetic::Exact);
    {
        const Math::Vector2i frame_size(64, 36);
        Scene::SceneRoot scene = Scene::SceneRoot("Atrium", Math::RGB(0.68f, 0.92f, 1.0f));
        const Scene::CameraID first_ID = Scene::Cameras::create("First", scene.get_ID(), Math::Matrix4x4f::identity(), Math::Matrix4x4f::identity());
        const ViewerScenes::AtriumCamera camera = ViewerScenes::create_atrium_scene(first_ID, scene.get_root_node(), 6000, 5);
        const Scene::CameraID second_ID = Scene::Cameras::create("Second", scene.get_ID(), Math::Matrix4x4f::identity(), Math::Matrix4x4f::identity());
        Scene::Cameras::set_transform(second_ID, Scene::Cameras::get_transform(first_ID));
        Math::Matrix4x4f projection, inverse_projection;
        Scene::CameraUtils::compute_perspective_projection(camera.near_plane, camera.far_plane, camera.field_of_view, float(frame_size.x) / float(frame_size.y), projection, inverse_projection);
        for (Scene::CameraID camera_ID : {first_ID, second_ID}) {
            Scene::Cameras::set_projection_matrices(camera_ID, projection, inverse_projection);
            Scene::Cameras::set_renderer_ID(camera_ID, renderer->get_renderer_ID());
            renderer->set_max_bounce_count(camera_ID, camera.max_bounce_count);
        }
        void* target = nullptr;
        EXPECT_TRUE(hipMalloc(&target, size_t(frame_size.x) * frame_size.y * 8) == hipSuccess);
        auto tick = [&](Scene::CameraID camera_ID) {
            renderer->handle_updates();
            const unsigned int iteration = renderer->render(camera_ID, target, frame_size.x, frame_size);
            reset_all_change_notifications();
            return iteration;
        };
        EXPECT_EQ(1u, tick(first_ID));       // the scene is built here, with the first camera's contexts the only ones
        EXPECT_EQ(1u, tick(second_ID));
        Scene::Cameras::destroy(first_ID);
        EXPECT_EQ(2u, tick(second_ID));      // handle_updates destroys the first camera's contexts
        Scene::SceneNode node = Assets::MeshModel(*Assets::MeshModels::get_iterable().begin()).get_scene_node();
        Math::Transform pose = node.get_global_transform();
        pose.translation = pose.translation + Math::Vector3f(400.0f, 0.0f, 0.0f);
        node.set_global_transform(pose);
        EXPECT_EQ(1u, tick(second_ID));      // restarted, over the rebuilt scene
        EXPECT_EQ(2u, tick(second_ID));
        EXPECT_TRUE(renderer->read_accumulation(frame));
        builds = renderer->scene_build_counts();
        EXPECT_TRUE(renderer->scene_update_counts().uploads >= 3u);      // both cameras' first uploads and the upload of the rebuilt scene: the tree was rebuilt, not refitted
        if (target) (void)hipFree(target);
    }
    delete renderer;
    deallocate_all();
    return frame;
}

GPU_TEST_F(DeviceBuildFixture, a_rebuild_after_the_first_camera_is_destroyed_builds_on_the_camera_that_is_left) {
    Renderer::SceneBuildCounts device_builds = {0, 0}, host_builds = {0, 0};
    const std::vector<double> device = render_after_the_first_camera_went(true, device_builds);
    const std::vector<double> host = render_after_the_first_camera_went(false, host_builds);
    EXPECT_EQ(2u, device_builds.device_builds);      // the first build on the first camera's contexts, the rebuild on the second camera's
    EXPECT_EQ(0u, device_builds.declined_builds);
    EXPECT_EQ(0u, host_builds.device_builds);
    EXPECT_TRUE(!device.empty());
    EXPECT_EQ(device.size(), host.size());
    size_t different = 0;
    for (size_t i = 0; i < device.size() && i < host.size(); ++i) different += std::memcmp(&device[i], &host[i], sizeof(double)) != 0;
    EXPECT_EQ(size_t(0), different);
}

} // namespace HIPRenderer
