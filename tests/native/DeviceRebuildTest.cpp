// DeviceRebuildTest.cpp -- a node dragged far through HIPRenderer::Renderer: the device refit reports a tree stretched past the 1.5 rule, and with
// HIPR_DEVICE_REBUILD=1 the trees are rebuilt where the triangles already are (hipr_rebuild_scene_trees; OR/Renderer.cpp:472,1010-1041 marks the acceleration
// dirty and OptiX rebuilds it on the device, :161-182,471-476) and the scene builder adopts them: no further upload, and the frame of a renderer that was given
// the pose from the start, bit for bit. With the variable unset the host rebuilds and the camera takes the upload, as before.
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

class DeviceRebuildFixture {
public:
    bool usable() const { return hipr_device_count() > 0; }
    void SetUp() { deallocate_all(); }
    void TearDown() { deallocate_all(); unsetenv("HIPR_DEVICE_REBUILD"); }

    static std::filesystem::path data_directory() {   // <repo>/bifrost3d_amd/data, found from the location of this executable
        if (const char* dir = std::getenv("HIPR_DATA_DIRECTORY")) return dir;
        std::error_code error;
        std::filesystem::path executable = std::filesystem::read_symlink("/proc/self/exe", error);
        return executable.parent_path() / ".." / ".." / "bifrost3d_amd" / "data";
    }

    static void drag_the_first_model_far() {
        for (Assets::MeshModelID model_ID : Assets::MeshModels::get_iterable()) {
            Scene::SceneNode node = Assets::MeshModel(model_ID).get_scene_node();
            node.set_global_transform(Math::Transform(Math::Vector3f(40.0f, 10.0f, -25.0f), Math::Quaternionf::identity(), 1.0f));
            break;
        }
    }

    // The small atrium (traced through the 8-wide tree). `from_the_start`: the model stands at the far pose before the first upload, three accumulations; otherwise
    // two accumulations, the model is dragged there, three more. Returns the last accumulation.
    std::vector<double> render(const char* device_rebuild, bool from_the_start, Renderer::SceneUpdateCounts& updates, Renderer::SceneRebuildCounts& rebuilds) {
        if (device_rebuild) setenv("HIPR_DEVICE_REBUILD", device_rebuild, 1); else unsetenv("HIPR_DEVICE_REBUILD");
        deallocate_all();
        std::vector<double> frame;
        Renderer* renderer = Renderer::initialize(0, data_directory());
        EXPECT_TRUE(renderer != nullptr);
        if (!renderer) return frame;
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
            if (from_the_start) drag_the_first_model_far();
            else {
                EXPECT_EQ(1u, tick());
                EXPECT_EQ(2u, tick());
                drag_the_first_model_far();
            }
            EXPECT_EQ(1u, tick());
            EXPECT_EQ(2u, tick());
            EXPECT_EQ(3u, tick());
            EXPECT_TRUE(renderer->read_accumulation(frame));
            updates = renderer->scene_update_counts();
            rebuilds = renderer->scene_rebuild_counts();
            if (target) (void)hipFree(target);
        }
        delete renderer;
        deallocate_all();
        return frame;
    }

    static size_t differing(const std::vector<double>& a, const std::vector<double>& b) {
        size_t different = a.size() == b.size() ? 0 : 1;
        for (size_t i = 0; i < a.size() && i < b.size(); ++i) different += std::memcmp(&a[i], &b[i], sizeof(double)) != 0;
        return different;
    }
};

GPU_TEST_F(DeviceRebuildFixture, a_node_dragged_far_is_rebuilt_on_the_device_without_an_upload) {
    Renderer::SceneUpdateCounts device_updates = {}, host_updates = {}, start_updates = {};
    Renderer::SceneRebuildCounts device_rebuilds = {}, host_rebuilds = {}, start_rebuilds = {};
    const std::vector<double> device = render("1", false, device_updates, device_rebuilds);
    const std::vector<double> host = render(nullptr, false, host_updates, host_rebuilds);
    const std::vector<double> start = render(nullptr, true, start_updates, start_rebuilds);
    EXPECT_EQ(1u, device_rebuilds.device_rebuilds);
    EXPECT_EQ(0u, device_rebuilds.declined_rebuilds);
    EXPECT_EQ(1u, device_updates.uploads);      // the first one: no further upload
    EXPECT_EQ(0u, device_updates.geometry_updates);
    // with the variable unset: the host rebuilds and the camera takes the whole description again
    EXPECT_EQ(0u, host_rebuilds.device_rebuilds);
    EXPECT_EQ(0u, host_rebuilds.declined_rebuilds);
    EXPECT_EQ(2u, host_updates.uploads);
    EXPECT_EQ(1u, start_updates.uploads);
    EXPECT_TRUE(!device.empty());
    EXPECT_EQ(size_t(0), differing(device, start));
    EXPECT_EQ(size_t(0), differing(host, start));
}

} // namespace HIPRenderer
