// DeviceRefitTest.cpp -- a moved node through HIPRenderer::Renderer: the transform-only tick refits the 8-wide tree on the device
// (hipr_refit_scene_transforms; OR/Renderer.cpp:472,1010-1041 refits the root acceleration) and must deliver, bit for bit, the
// accumulation of the host path it replaces (SceneBuilder::update_model_transforms + hipr_update_scene_geometry, HIPR_DEVICE_REFIT=0).
#include "MiniTest.h"

#include "../../bifrost3d_amd/host/HIPRenderer/Renderer.h"
#include "../../bifrost3d_amd/host/MaterialScene.h"
#include "../../include/hiprenderer_c.h"

#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <filesystem>

using namespace Bifrost;

namespace HIPRenderer {

class DeviceRefitFixture {
public:
    bool usable() const { return hipr_device_count() > 0; }
    void SetUp() { deallocate_all(); }
    void TearDown() { deallocate_all(); unsetenv("HIPR_DEVICE_REFIT"); }

    static std::filesystem::path data_directory() {   // <repo>/bifrost3d_amd/data, found from the location of this executable
        if (const char* dir = std::getenv("HIPR_DATA_DIRECTORY")) return dir;
        std::error_code error;
        std::filesystem::path executable = std::filesystem::read_symlink("/proc/self/exe", error);
        return executable.parent_path() / ".." / ".." / "bifrost3d_amd" / "data";
    }

    // The small atrium (6 000 triangles: traced through the 8-wide tree) rendered for two accumulations, one of its models moved, three more accumulations.
    // Returns the accumulation after the move; `still` receives the one before it, `updates` how the scene reached the device over the whole run.
    std::vector<double> render_with_a_moved_model(bool on_the_device, std::vector<double>& still, Renderer::SceneUpdateCounts& updates) {
        setenv("HIPR_DEVICE_REFIT", on_the_device ? "1" : "0", 1);
        deallocate_all();
        std::vector<double> moved;
        Renderer* renderer = Renderer::initialize(0, data_directory());
        EXPECT_TRUE(renderer != nullptr);
        if (!renderer) return moved;
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
            EXPECT_EQ(1u, tick());
            EXPECT_EQ(2u, tick());
            EXPECT_TRUE(renderer->read_accumulation(still));

            // every model in turn is given a new pose: the floor, walls, columns ... whatever the camera sees moves
            unsigned int index = 0;
            for (Assets::MeshModelID model_ID : Assets::MeshModels::get_iterable()) {
                if (++index > 3) break;
                Scene::SceneNode node = Assets::MeshModel(model_ID).get_scene_node();
                Math::Transform pose = node.get_global_transform();
                pose.translation = pose.translation + Math::Vector3f(0.35f, 0.2f * float(index), -0.15f);
                pose.rotation = Math::Quaternionf::from_angle_axis(0.1f * float(index), Math::Vector3f::up()) * pose.rotation;
                node.set_global_transform(pose);
            }
            EXPECT_EQ(1u, tick());      // restarted
            EXPECT_EQ(2u, tick());
            EXPECT_EQ(3u, tick());
            EXPECT_TRUE(renderer->read_accumulation(moved));
            updates = renderer->scene_update_counts();
            if (target) (void)hipFree(target);
        }
        delete renderer;
        deallocate_all();
        return moved;
    }
};

GPU_TEST_F(DeviceRefitFixture, a_moved_node_gives_the_same_accumulation_on_the_device_and_on_the_host_path) {
    std::vector<double> still_device, still_host;
    Renderer::SceneUpdateCounts device_updates = {}, host_updates = {};
    const std::vector<double> device = render_with_a_moved_model(true, still_device, device_updates);
    const std::vector<double> host = render_with_a_moved_model(false, still_host, host_updates);
    // the device leg did refit on the device, once, with no rebuild and no second upload behind it; the other leg went through the host and never near the kernels
    EXPECT_EQ(1u, device_updates.device_refits);
    EXPECT_EQ(0u, device_updates.geometry_updates);
    EXPECT_EQ(1u, device_updates.uploads);
    EXPECT_EQ(0u, host_updates.device_refits);
    EXPECT_EQ(1u, host_updates.geometry_updates);
    EXPECT_EQ(1u, host_updates.uploads);
    EXPECT_TRUE(!device.empty());
    EXPECT_EQ(device.size(), host.size());
    EXPECT_TRUE(still_device == still_host);
    EXPECT_TRUE(still_device != device);      // the models did move in the picture
    size_t different = 0;
    for (size_t i = 0; i < device.size() && i < host.size(); ++i) different += std::memcmp(&device[i], &host[i], sizeof(double)) != 0;
    if (different) fprintf(stderr, "device refit vs host refit: %zu of %zu accumulated values differ\n", different, device.size());
    EXPECT_EQ(size_t(0), different);
}

} // namespace HIPRenderer
