// InstanceEditTest.cpp -- a model destroyed and a copy of another created through HIPRenderer::Renderer: with HIPR_DEVICE_INSTANCE_EDIT=1 the tick edits the resident
// scene (hipr_edit_scene_instances; OR/Renderer.cpp:138-182, :1043-1110 removes and adds a child of the root group) and the scene builder adopts the trees: the counter
// moves, no further upload, and the frame of the host path bit for bit. With the variable unset the scene is retired and the camera takes the upload, as before.
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

class InstanceEditFixture {
public:
    bool usable() const { return hipr_device_count() > 0; }
    void SetUp() { deallocate_all(); }
    void TearDown() { deallocate_all(); unsetenv("HIPR_DEVICE_INSTANCE_EDIT"); }

    static std::filesystem::path data_directory() {   // <repo>/bifrost3d_amd/data, found from the location of this executable
        if (const char* dir = std::getenv("HIPR_DATA_DIRECTORY")) return dir;
        std::error_code error;
        std::filesystem::path executable = std::filesystem::read_symlink("/proc/self/exe", error);
        return executable.parent_path() / ".." / ".." / "bifrost3d_amd" / "data";
    }

    // The first model goes; the third one is drawn once more, aside, under the second one's material.
    static void destroy_one_model_and_copy_another(Scene::SceneNode root) {
        Assets::MeshModelID models[3];
        int found = 0;
        for (Assets::MeshModelID model_ID : Assets::MeshModels::get_iterable()) {
            if (found < 3) models[found] = model_ID;
            ++found;
        }
        EXPECT_TRUE(found >= 3);
        if (found < 3) return;
        const Assets::MeshModel source = models[2], other = models[1];
        Scene::SceneNode node = Scene::SceneNodes::create("Copy", Math::Transform(Math::Vector3f(0.6f, 0.4f, -0.8f), Math::Quaternionf::identity(), 0.7f));
        node.set_parent(root);
        Assets::MeshModels::create(node.get_ID(), source.get_mesh().get_ID(), other.get_material().get_ID());
        Assets::MeshModels::destroy(models[0]);
    }

    // The small atrium (traced through the 8-wide tree): two accumulations, the edit, three more. Returns the last accumulation.
    std::vector<double> render(const char* device_edit, Renderer::SceneUpdateCounts& updates) {
        if (device_edit) setenv("HIPR_DEVICE_INSTANCE_EDIT", device_edit, 1); else unsetenv("HIPR_DEVICE_INSTANCE_EDIT");
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
            EXPECT_EQ(1u, tick());
            EXPECT_EQ(2u, tick());
            destroy_one_model_and_copy_another(scene.get_root_node());
            EXPECT_EQ(1u, tick());
            EXPECT_EQ(2u, tick());
            EXPECT_EQ(3u, tick());
            EXPECT_TRUE(renderer->read_accumulation(frame));
            updates = renderer->scene_update_counts();
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

GPU_TEST_F(InstanceEditFixture, a_destroyed_model_and_a_created_copy_edit_the_resident_scene) {
    Renderer::SceneUpdateCounts device_updates = {}, host_updates = {};
    const std::vector<double> device = render("1", device_updates);
    const std::vector<double> host = render(nullptr, host_updates);
    EXPECT_EQ(1u, device_updates.instance_edits);
    EXPECT_EQ(1u, device_updates.uploads);      // the first one: no further upload
    // with the variable unset: the scene is retired and the camera takes the whole description again
    EXPECT_EQ(0u, host_updates.instance_edits);
    EXPECT_EQ(2u, host_updates.uploads);
    EXPECT_TRUE(!device.empty());
    EXPECT_EQ(size_t(0), differing(device, host));
}

} // namespace HIPRenderer
