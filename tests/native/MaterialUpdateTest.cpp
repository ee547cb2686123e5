// MaterialUpdateTest.cpp -- material edits through HIPRenderer::Renderer: a tick whose only changes are a material's data and a model's material is applied to
// the resident scene by kernels (hipr_update_scene_materials; OR/Renderer.cpp:753-850 rewrites one slot of the material buffer) and must deliver, bit for bit,
// the accumulation of the path it replaces (a new scene: flatten, build, upload; HIPR_DEVICE_MATERIAL_UPDATE=0).
#include "MiniTest.h"

#include "../../bifrost3d_amd/host/HIPRenderer/Renderer.h"
#include "../../include/hiprenderer_c.h"

#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>
#include <filesystem>

using namespace Bifrost;

namespace HIPRenderer {

class MaterialUpdateFixture {
public:
    bool usable() const { return hipr_device_count() > 0; }
    void SetUp() { deallocate_all(); }
    void TearDown() { deallocate_all(); unsetenv("HIPR_DEVICE_MATERIAL_UPDATE"); }

    static std::filesystem::path data_directory() {   // <repo>/bifrost3d_amd/data, found from the location of this executable
        if (const char* dir = std::getenv("HIPR_DATA_DIRECTORY")) return dir;
        std::error_code error;
        std::filesystem::path executable = std::filesystem::read_symlink("/proc/self/exe", error);
        return executable.parent_path() / ".." / ".." / "bifrost3d_amd" / "data";
    }

    // The Cornell box of RendererTest.cpp with every wall a plane of 4 x 4 quads: 184 triangles. The box of 34 triangles is searched exhaustively, and a scene
    // that carries the exhaustive search's items is the one hipr_update_scene_materials refuses; this one is traced through the 8-wide tree.
    struct CornellBox { Assets::Material copper, red; Assets::MeshModelID small_box; };
    static CornellBox create_cornell_box(Scene::CameraID camera_ID, Scene::SceneNode root_node) {
        using namespace Bifrost::Assets;
        using namespace Bifrost::Math;
        using namespace Bifrost::Scene;
        auto thin_dielectric = [](const char* name, RGB tint) {
            Materials::Data data = Materials::Data::create_dielectric(tint, 1.0f, 0.02f);
            data.flags = MaterialFlag::ThinWalled;
            return Material(Materials::create(name, data));
        };
        Material white = thin_dielectric("White", RGB(0.98f));
        Material red = thin_dielectric("Red", RGB(0.98f, 0.02f, 0.02f));
        Material green = thin_dielectric("Green", RGB(0.02f, 0.98f, 0.02f));
        Material iron = Material::create_metal("Iron", RGB(0.560f, 0.570f, 0.580f), 0.4f);
        Material copper = Material::create_metal("Copper", RGB(0.955f, 0.637f, 0.538f), 0.02f);

        Transform camera_transform = Cameras::get_transform(camera_ID);
        camera_transform.translation = Vector3f(0, 0.0f, -1.5f);
        Cameras::set_transform(camera_ID, camera_transform);

        SceneNode light_node = SceneNode("Light", Transform(Vector3f(0.0f, 0.45f, 0.0f)));
        light_node.set_parent(root_node);
        LightSources::create_sphere_light(light_node.get_ID(), RGB(2.0f), 0.05f);

        const float half_pi = PI<float>() * 0.5f;
        struct Wall { const char* name; Material material; Transform transform; };
        const Wall walls[] = {
            {"Floor", white, Transform(Vector3f(0.0f, -0.5f, 0.0f))},
            {"Roof", white, Transform(Vector3f(0.0f, 0.5f, 0.0f), Quaternionf::from_angle_axis(PI<float>(), Vector3f::forward()))},
            {"Back", white, Transform(Vector3f(0.0f, 0.0f, 0.5f), Quaternionf::from_angle_axis(-half_pi, Vector3f::right()))},
            {"Left", red, Transform(Vector3f(-0.5f, 0.0f, 0.0f), Quaternionf::from_angle_axis(-half_pi, Vector3f::forward()))},
            {"Right", green, Transform(Vector3f(0.5f, 0.0f, 0.0f), Quaternionf::from_angle_axis(half_pi, Vector3f::forward()))},
        };
        Mesh plane_mesh = MeshCreation::plane(4, MeshFlag::GeometryBuffers);
        for (const Wall& wall : walls) {
            SceneNode node = SceneNode(wall.name, wall.transform);
            MeshModel(node, plane_mesh, wall.material);
            node.set_parent(root_node);
        }

        CornellBox out = {copper, red, MeshModelID::invalid_UID()};
        struct Box { const char* name; Material material; float y_stretch; Transform transform; };
        const Box boxes[] = {
            {"Small box", iron, 1.0f, Transform(Vector3f(0.2f, -0.35f, -0.2f), Quaternionf::from_angle_axis(PI<float>() / 6.0f, Vector3f::up()), 0.3f)},
            {"Big box", copper, 2.0f, Transform(Vector3f(-0.2f, -0.2f, 0.2f), Quaternionf::from_angle_axis(-PI<float>() / 6.0f, Vector3f::up()), 0.3f)},
        };
        for (const Box& box : boxes) {
            Mesh mesh = MeshCreation::box(1);
            for (unsigned int v = 0; v < mesh.get_vertex_count(); ++v) mesh.get_positions()[v].y *= box.y_stretch;
            SceneNode node = SceneNode(box.name, box.transform);
            MeshModel model(node, mesh, box.material);
            if (out.small_box == MeshModelID::invalid_UID()) out.small_box = model.get_ID();
            node.set_parent(root_node);
        }
        return out;
    }

    // Two accumulations, then ONE tick with a Materials update (the copper turns rough and coated) and a MeshModels::Change::Material (the small box takes the
    // red wall's thin-walled material), then three more. Returns the accumulation after the edit; `before` receives the one before it.
    std::vector<double> render_with_edited_materials(bool on_the_device, std::vector<double>& before, Renderer::SceneUpdateCounts& at_edit, Renderer::SceneUpdateCounts& updates) {
        setenv("HIPR_DEVICE_MATERIAL_UPDATE", on_the_device ? "1" : "0", 1);
        deallocate_all();
        std::vector<double> edited;
        Renderer* renderer = Renderer::initialize(0, data_directory());
        EXPECT_TRUE(renderer != nullptr);
        if (!renderer) return edited;
        {
            const Math::Vector2i frame_size(64, 36);
            Scene::SceneRoot scene = Scene::SceneRoot("Cornell", Math::RGB(0.68f, 0.92f, 1.0f));
            const Scene::CameraID camera_ID = Scene::Cameras::create("Camera", scene.get_ID(), Math::Matrix4x4f::identity(), Math::Matrix4x4f::identity());
            CornellBox box = create_cornell_box(camera_ID, scene.get_root_node());
            Math::Matrix4x4f projection, inverse_projection;
            Scene::CameraUtils::compute_perspective_projection(0.1f, 100.0f, Math::PI<float>() / 4.0f, float(frame_size.x) / float(frame_size.y), projection, inverse_projection);
            Scene::Cameras::set_projection_matrices(camera_ID, projection, inverse_projection);
            Scene::Cameras::set_renderer_ID(camera_ID, renderer->get_renderer_ID());
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
            EXPECT_TRUE(renderer->read_accumulation(before));
            at_edit = renderer->scene_update_counts();

            Assets::Materials::Data copper = Assets::Materials::get_data(box.copper.get_ID());
            copper.roughness = 0.6f;
            copper.coat = 0.5f;
            copper.coat_roughness = 0.1f;
            Assets::Materials::set_data(box.copper.get_ID(), copper);
            Assets::MeshModels::set_material_ID(box.small_box, box.red.get_ID());
            EXPECT_EQ(1u, tick());      // restarted
            EXPECT_EQ(2u, tick());
            EXPECT_EQ(3u, tick());
            EXPECT_TRUE(renderer->read_accumulation(edited));
            updates = renderer->scene_update_counts();
            if (target) (void)hipFree(target);
        }
        delete renderer;
        deallocate_all();
        return edited;
    }
};

GPU_TEST_F(MaterialUpdateFixture, edited_materials_give_the_same_accumulation_on_the_device_and_with_a_new_scene) {
    std::vector<double> before_device, before_host;
    Renderer::SceneUpdateCounts device_at_edit = {}, host_at_edit = {}, device_updates = {}, host_updates = {};
    const std::vector<double> device = render_with_edited_materials(true, before_device, device_at_edit, device_updates);
    const std::vector<double> host = render_with_edited_materials(false, before_host, host_at_edit, host_updates);
    // the device leg applied the edit to the resident scene, once, with no upload behind it; the other leg made a new scene and uploaded it
    EXPECT_EQ(1u, device_updates.material_updates);
    EXPECT_EQ(device_at_edit.uploads, device_updates.uploads);
    EXPECT_EQ(0u, host_updates.material_updates);
    EXPECT_EQ(host_at_edit.uploads + 1u, host_updates.uploads);
    EXPECT_TRUE(!device.empty());
    EXPECT_EQ(device.size(), host.size());
    EXPECT_TRUE(before_device == before_host);
    EXPECT_TRUE(before_device != device);      // the edit shows in the picture
    size_t different = 0;
    for (size_t i = 0; i < device.size() && i < host.size(); ++i) different += std::memcmp(&device[i], &host[i], sizeof(double)) != 0;
    if (different) fprintf(stderr, "device material update vs new scene: %zu of %zu accumulated values differ\n", different, device.size());
    EXPECT_EQ(size_t(0), different);
}

} // namespace HIPRenderer
