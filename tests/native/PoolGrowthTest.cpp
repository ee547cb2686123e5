// PoolGrowthTest.cpp -- a model created over a NEW mesh under a NEW material, and another model destroyed, through HIPRenderer::Renderer: with
// HIPR_DEVICE_POOL_GROWTH=1 the tick appends the mesh to the resident pools (hipr_append_scene_pools; OR/Renderer.cpp:92-136 load_mesh, :754-812 upload_material),
// edits the resident scene (hipr_edit_scene_instances) and the scene builder adopts the trees: the counter moves, no further upload, and the frame of the host path
// bit for bit. With the variable unset the scene is retired and the camera takes the upload, as before.
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

class PoolGrowthFixture {
public:
    bool usable() const { return hipr_device_count() > 0; }
    void SetUp() { deallocate_all(); }
    void TearDown() { deallocate_all(); unsetenv("HIPR_DEVICE_POOL_GROWTH"); }

    static std::filesystem::path data_directory() {   // <repo>/bifrost3d_amd/data, found from the location of this executable
        if (const char* dir = std::getenv("HIPR_DATA_DIRECTORY")) return dir;
        std::error_code error;
        std::filesystem::path executable = std::filesystem::read_symlink("/proc/self/exe", error);
        return executable.parent_path() / ".." / ".." / "bifrost3d_amd" / "data";
    }

    // A box the scene has no mesh for, under a metal the scene has no material for, in front of the camera; the first model goes.
    static void create_a_model_over_a_new_mesh_and_destroy_another(Scene::SceneNode root) {
        Assets::MeshModelID first = Assets::MeshModelID::invalid_UID();
        for (Assets::MeshModelID model_ID : Assets::MeshModels::get_iterable()) { first = model_ID; break; }
        EXPECT_TRUE(first != Assets::MeshModelID::invalid_UID());
        Assets::Mesh box = Assets::MeshCreation::box(2, Math::Vector3f(1.0f, 0.5f, 0.8f));
        Assets::Material metal = Assets::Material::create_metal("New metal", Math::RGB(0.9f, 0.5f, 0.2f), 0.3f);
        Scene::SceneNode node = Scene::SceneNodes::create("New box", Math::Transform(Math::Vector3f(0.6f, 0.4f, -0.8f), Math::Quaternionf::identity(), 0.7f));
        node.set_parent(root);
        Assets::MeshModels::create(node.get_ID(), box.get_ID(), metal.get_ID());
        Assets::MeshModels::destroy(first);
    }

    // Three ticks that each grow or leave a pool. A: a box with a model over it. B: that model AND its mesh destroyed -- the mesh's data stays pooled, its ID is free
    // after the tick. C: a plane, which takes the recycled ID, with a model over it: it must be drawn as the plane, not as the box whose ID it carries.
    Assets::MeshModelID created_model = Assets::MeshModelID::invalid_UID();
    Assets::MeshID created_mesh = Assets::MeshID::invalid_UID();
    void recycled_mesh_tick(int which, Scene::SceneNode root) {
        const Math::Transform pose(Math::Vector3f(0.6f, 0.4f, -0.8f), Math::Quaternionf::identity(), 0.7f);
        if (which == 0 || which == 2) {
            Assets::Mesh mesh = which == 0 ? Assets::MeshCreation::box(2, Math::Vector3f(1.0f, 0.5f, 0.8f)) : Assets::MeshCreation::plane(3, Assets::MeshFlag::GeometryBuffers);
            if (which == 2) EXPECT_EQ(created_mesh.get_index(), mesh.get_ID().get_index());      // the recycled ID: what the case is about
            Assets::MeshModelID first = Assets::MeshModelID::invalid_UID();
            for (Assets::MeshModelID model_ID : Assets::MeshModels::get_iterable()) { first = model_ID; break; }
            Scene::SceneNode node = Scene::SceneNodes::create(which == 0 ? "New box" : "New plane", pose);
            node.set_parent(root);
            created_mesh = mesh.get_ID();
            created_model = Assets::MeshModels::create(node.get_ID(), mesh.get_ID(), Assets::MeshModel(first).get_material().get_ID());
        } else {
            Assets::MeshModels::destroy(created_model);
            Assets::Meshes::destroy(created_mesh);
        }
    }

    // The small atrium (traced through the 8-wide tree): two accumulations, the growth, three more. Returns the last accumulation. `recycled`: the three ticks of
    // recycled_mesh_tick, two accumulations after each of the first two, instead of the one growth.
    std::vector<double> render(const char* device_growth, Renderer::SceneUpdateCounts& updates, bool recycled = false) {
        if (device_growth) setenv("HIPR_DEVICE_POOL_GROWTH", device_growth, 1); else unsetenv("HIPR_DEVICE_POOL_GROWTH");
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
            if (recycled) {
                for (int which = 0; which < 2; ++which) {
                    recycled_mesh_tick(which, scene.get_root_node());
                    EXPECT_EQ(1u, tick());
                    EXPECT_EQ(2u, tick());
                }
                recycled_mesh_tick(2, scene.get_root_node());
            } else create_a_model_over_a_new_mesh_and_destroy_another(scene.get_root_node());
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

GPU_TEST_F(PoolGrowthFixture, a_model_over_a_new_mesh_grows_the_resident_pools) {
    Renderer::SceneUpdateCounts device_updates = {}, host_updates = {};
    const std::vector<double> device = render("1", device_updates);
    const std::vector<double> host = render(nullptr, host_updates);
    EXPECT_EQ(1u, device_updates.pool_growths);
    EXPECT_EQ(0u, device_updates.instance_edits);      // counted as a growth, not as an edit
    EXPECT_EQ(1u, device_updates.uploads);             // the first one: one upload instead of two
    // with the variable unset: the counter stays 0, the scene is retired and the camera takes the whole description again
    EXPECT_EQ(0u, host_updates.pool_growths);
    EXPECT_EQ(2u, host_updates.uploads);
    EXPECT_TRUE(!device.empty());
    EXPECT_EQ(size_t(0), differing(device, host));
}

GPU_TEST_F(PoolGrowthFixture, a_new_mesh_under_a_recycled_mesh_id_is_drawn_as_itself) {
    Renderer::SceneUpdateCounts device_updates = {}, host_updates = {};
    const std::vector<double> device = render("1", device_updates, true);
    const std::vector<double> host = render(nullptr, host_updates, true);
    EXPECT_EQ(3u, device_updates.pool_growths);        // the box, the destroyed mesh, the plane
    EXPECT_EQ(1u, device_updates.uploads);
    EXPECT_EQ(0u, host_updates.pool_growths);
    EXPECT_EQ(4u, host_updates.uploads);
    EXPECT_TRUE(!device.empty());
    EXPECT_EQ(size_t(0), differing(device, host));
}

} // namespace HIPRenderer
