// TexelUpdateTest.cpp -- the pixels of an image the scene already shows rewritten in place (Images::get_mutable_pixels), through HIPRenderer::Renderer: with
// HIPR_DEVICE_TEXEL_UPDATE=1 the tick writes the image into the resident texel pools and has the flags that follow texels decided again on the device
// (hipr_update_scene_texels; the reference asserts "Pixel update not implemented yet", OR/Renderer.cpp:697-698) while the scene builder follows without a rebuild: the
// counter moves, no further upload, and the frame of a renderer created after the edit bit for bit. With the variable unset the counter stays 0, the scene is
// retired and the camera takes the upload, as before -- and the frame is the same.
#include "MiniTest.h"

#include "../../bifrost3d_amd/host/HIPRenderer/Renderer.h"
#include "../../bifrost3d_amd/host/MaterialScene.h"
#include "../../include/hiprenderer_c.h"

#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <vector>

using namespace Bifrost;

namespace HIPRenderer {

class TexelUpdateFixture {
public:
    bool usable() const { return hipr_device_count() > 0; }
    void SetUp() { deallocate_all(); }
    void TearDown() { deallocate_all(); unsetenv("HIPR_DEVICE_TEXEL_UPDATE"); }

    static std::filesystem::path data_directory() {   // <repo>/bifrost3d_amd/data, found from the location of this executable
        if (const char* dir = std::getenv("HIPR_DATA_DIRECTORY")) return dir;
        std::error_code error;
        std::filesystem::path executable = std::filesystem::read_symlink("/proc/self/exe", error);
        return executable.parent_path() / ".." / ".." / "bifrost3d_amd" / "data";
    }

    static constexpr unsigned LACE = 32;
    // The hole of the edit: a square of 12 x 12 texels in the middle of the lace.
    static void punch_hole(unsigned char* pixels) {
        for (unsigned y = 10; y < 22; ++y)
            for (unsigned x = 10; x < 22; ++x) pixels[x + y * LACE] = 0;
    }

    // A banner in front of the camera: a plane of 8 x 8 quads under a cut-out material whose coverage texture is a solid 32 x 32 lace image (`with_hole`: the hole
    // punched before the renderer sees it). Returns the image.
    static Assets::ImageID create_banner(Scene::SceneNode root, bool with_hole) {
        std::vector<unsigned char> pixels(LACE * LACE, 255);
        if (with_hole) punch_hole(pixels.data());
        const Assets::ImageID image = Assets::Images::create2D("lace", Assets::PixelFormat::Intensity8, false, LACE, LACE, pixels.data(), pixels.size());
        const Assets::TextureID texture = Assets::Textures::create2D(image, Assets::MagnificationFilter::None, Assets::MinificationFilter::None, Assets::WrapMode::Repeat, Assets::WrapMode::Repeat);
        Assets::Materials::Data data = Assets::Materials::Data::create_dielectric(Math::RGB(0.9f, 0.2f, 0.1f), 0.7f);
        data.flags = Assets::MaterialFlag::Cutout;
        data.coverage = 0.5f;
        data.coverage_texture_ID = texture;
        const Assets::MaterialID material = Assets::Materials::create("Lace", data);
        Assets::MeshFlags buffers = Assets::MeshFlag::Position; buffers |= Assets::MeshFlag::Normal; buffers |= Assets::MeshFlag::Texcoord;
        Assets::Mesh plane = Assets::MeshCreation::plane(8, buffers);
        // three units ahead of the atrium's camera (which stands at (-12.6, 2.2, -0.5) and looks along +x), turned a quarter about z so that it faces the camera
        Scene::SceneNode node = Scene::SceneNodes::create("Banner", Math::Transform(Math::Vector3f(-9.6f, 2.45f, -0.35f), Math::Quaternionf(0.0f, 0.0f, 0.70710678f, 0.70710678f), 1.5f));
        node.set_parent(root);
        Assets::MeshModels::create(node.get_ID(), plane.get_ID(), material);
        return image;
    }

    // The small atrium with the banner. `edit`: 0 none; 1 two accumulations, then the hole punched into the resident image and two more; 2 the hole is there from
    // the start. Then, in every case, the environment's tint set to what it is -- a change that restarts the accumulation on either path and leaves the scene alone: the
    // full path keeps accumulating over a pixel edit (as the reference does), the device path restarts, and the frames to compare are those of the scene as it stands
    // after the edit -- and three accumulations. Returns the last accumulation; `at_edit`: the counts before the edit's tick.
    std::vector<double> render(const char* device_texel_update, int edit, Renderer::SceneUpdateCounts& at_edit, Renderer::SceneUpdateCounts& updates) {
        if (device_texel_update) setenv("HIPR_DEVICE_TEXEL_UPDATE", device_texel_update, 1); else unsetenv("HIPR_DEVICE_TEXEL_UPDATE");
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
            const Assets::ImageID lace = create_banner(scene.get_root_node(), edit == 2);
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
            at_edit = renderer->scene_update_counts();
            if (edit == 1) {
                punch_hole(static_cast<unsigned char*>(Assets::Images::get_mutable_pixels(lace)));      // nothing else: the tick's only dirt
                EXPECT_EQ(device_texel_update ? 1u : 3u, tick());      // on the device the edit restarts the accumulation; the full path goes on, as it always did
                EXPECT_EQ(device_texel_update ? 2u : 4u, tick());
            }
            scene.set_environment_tint(Math::RGB(0.68f, 0.92f, 1.0f));
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

GPU_TEST_F(TexelUpdateFixture, a_hole_punched_into_the_lace_image_stays_on_the_device) {
    Renderer::SceneUpdateCounts device_at_edit = {}, device_updates = {}, host_at_edit = {}, host_updates = {}, ignored = {}, after_updates = {}, still_updates = {};
    const std::vector<double> device = render("1", 1, device_at_edit, device_updates);
    const std::vector<double> host = render(nullptr, 1, host_at_edit, host_updates);
    const std::vector<double> created_after = render(nullptr, 2, ignored, after_updates);
    const std::vector<double> still = render(nullptr, 0, ignored, still_updates);
    EXPECT_EQ(0u, device_at_edit.texel_updates);
    EXPECT_EQ(1u, device_updates.texel_updates);
    EXPECT_EQ(device_at_edit.uploads, device_updates.uploads);      // the uploads stay where they were
    EXPECT_EQ(1u, device_updates.uploads);
    // with the variable unset: the counter stays 0, the scene is retired and the camera takes the whole description again
    EXPECT_EQ(0u, host_updates.texel_updates);
    EXPECT_EQ(2u, host_updates.uploads);
    EXPECT_TRUE(!device.empty());
    EXPECT_EQ(size_t(0), differing(device, created_after));      // the frame of a renderer created after the edit
    EXPECT_EQ(size_t(0), differing(host, created_after));
    EXPECT_TRUE(differing(device, still) != 0);                  // the edit shows
}

} // namespace HIPRenderer
