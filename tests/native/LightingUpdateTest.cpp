// LightingUpdateTest.cpp -- a lamp created, and the scene's environment map set to a texture the scene already holds, through HIPRenderer::Renderer: with
// HIPR_DEVICE_LIGHTING=1 the tick replaces the resident light list and builds the environment's PDF image and samples on the device (hipr_update_scene_lighting;
// OR/Renderer.cpp:852-1008, :1136-1196) and the scene builder adopts the outcome: the counter moves, no further upload, and the frame of the host path bit for bit.
// With the variable unset the counter stays 0, the scene is retired and the camera takes the upload, as before.
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

class LightingUpdateFixture {
public:
    bool usable() const { return hipr_device_count() > 0; }
    void SetUp() { deallocate_all(); }
    void TearDown() { deallocate_all(); unsetenv("HIPR_DEVICE_LIGHTING"); }

    static std::filesystem::path data_directory() {   // <repo>/bifrost3d_amd/data, found from the location of this executable
        if (const char* dir = std::getenv("HIPR_DATA_DIRECTORY")) return dir;
        std::error_code error;
        std::filesystem::path executable = std::filesystem::read_symlink("/proc/self/exe", error);
        return executable.parent_path() / ".." / ".." / "bifrost3d_amd" / "data";
    }

    // A 48 x 24 RGBA float sky -- lower than the PDF image: resampled and blurred -- with a gradient and one bright texel, made before the first upload.
    static Assets::TextureID create_sky() {
        const unsigned width = 48, height = 24;
        std::vector<float> pixels(size_t(width) * height * 4);
        for (unsigned y = 0; y < height; ++y)
            for (unsigned x = 0; x < width; ++x) {
                float* p = pixels.data() + 4 * (x + size_t(y) * width);
                p[0] = 0.2f + 0.01f * float(x); p[1] = 0.3f + 0.02f * float(y); p[2] = 0.9f - 0.01f * float(x + y); p[3] = 1.0f;
            }
        pixels[4 * (30 + 16 * width)] = 50.0f;
        const Assets::ImageID image = Assets::Images::create2D("sky", Assets::PixelFormat::RGBA_Float, false, width, height, pixels.data(), pixels.size() * 4);
        return Assets::Textures::create2D(image, Assets::MagnificationFilter::Linear, Assets::MinificationFilter::Linear, Assets::WrapMode::Repeat, Assets::WrapMode::Clamp);
    }

    // The small atrium: two accumulations, the lighting edit(s), three more. Returns the last accumulation. `edits`: bit 0 a lamp created, bit 1 the sky set.
    std::vector<double> render(const char* device_lighting, int edits, Renderer::SceneUpdateCounts& updates) {
        if (device_lighting) setenv("HIPR_DEVICE_LIGHTING", device_lighting, 1); else unsetenv("HIPR_DEVICE_LIGHTING");
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
            const Assets::TextureID sky = create_sky();
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
            if (edits & 1) {
                Scene::SceneNode node = Scene::SceneNodes::create("New lamp", Math::Transform(Math::Vector3f(0.6f, 1.2f, -0.8f), Math::Quaternionf::identity(), 1.0f));
                node.set_parent(scene.get_root_node());
                Scene::LightSources::create_sphere_light(node.get_ID(), Math::RGB(40.0f, 30.0f, 20.0f), 0.05f);
            }
            if (edits & 2) scene.set_environment_map(sky);
            const unsigned int first = edits ? 1u : 3u;      // an edit resets the accumulation
            EXPECT_EQ(first, tick());
            EXPECT_EQ(first + 1u, tick());
            EXPECT_EQ(first + 2u, tick());
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

    void compare(int edits) {
        Renderer::SceneUpdateCounts device_updates = {}, host_updates = {}, still_updates = {};
        const std::vector<double> device = render("1", edits, device_updates);
        const std::vector<double> host = render(nullptr, edits, host_updates);
        const std::vector<double> still = render(nullptr, 0, still_updates);
        EXPECT_EQ(1u, device_updates.lighting_updates);
        EXPECT_EQ(1u, device_updates.uploads);             // the first one: one upload instead of two
        // with the variable unset: the counter stays 0, the scene is retired and the camera takes the whole description again
        EXPECT_EQ(0u, host_updates.lighting_updates);
        EXPECT_EQ(2u, host_updates.uploads);
        EXPECT_TRUE(!device.empty());
        EXPECT_EQ(size_t(0), differing(device, host));
        EXPECT_TRUE(differing(device, still) != 0);        // the edit shows
    }
};

GPU_TEST_F(LightingUpdateFixture, a_lamp_created_replaces_the_resident_light_list) { compare(1); }
GPU_TEST_F(LightingUpdateFixture, an_environment_map_set_is_built_on_the_device) { compare(2); }
GPU_TEST_F(LightingUpdateFixture, a_lamp_and_an_environment_in_one_tick) { compare(3); }

} // namespace HIPRenderer
