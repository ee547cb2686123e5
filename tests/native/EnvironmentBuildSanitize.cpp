// EnvironmentBuildSanitize.cpp -- a stand-alone program around SceneBuilder::staged_environment_build, build_host_environment (EnvironmentBuildHost.hip: the routines
// of csrc/environment_build.h walked on the host in the kernels' shape) and SceneBuilder::set_lights / adopt_lighting for a run under AddressSanitizer /
// UndefinedBehaviorSanitizer on the CPU: `make -C bifrost3d_amd sanitize-environment-build` builds and runs it, the scene builder and its tree builders compiled in; it
// links no product library.
// The scene: a 6 x 6 quad mesh with one lamp and three textures. Each map is staged, walked and adopted: 37 x 19 floats, bilinear (resampled to 128 rows, blurred;
// an odd width under one tile); 70 x 131 sRGB bytes, nearest (the table, rows past four bands, a second tile of six columns); 9 x 5 black floats (the disabled form).
// Between them the light list is replaced -- grown past 32, emptied -- and at the end the environment is removed.
#include "../../bifrost3d_amd/host/SceneBuilder.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace HIPRenderer;
extern "C" int build_host_environment(const HiprTexture* texture, const uint8_t* texels, const HiprEnvironmentBuild* build, float* out_per_pixel_PDF, uint64_t pdf_capacity, HiprLightSample* out_samples,
                                      uint32_t sample_capacity, HiprLightingResult* out);
static MeshData grid(int cells) {
    MeshData m;
    for (int i = 0; i <= cells; ++i)
        for (int j = 0; j <= cells; ++j) m.positions.push_back(Vector3f(float(i) / cells, float(j) / cells, 0.05f * (rand() / float(RAND_MAX))));
    auto at = [&](int i, int j) { return uint32_t(i * (cells + 1) + j); };
    for (int i = 0; i < cells; ++i)
        for (int j = 0; j < cells; ++j) { m.primitives.push_back(Vector3ui{at(i, j), at(i + 1, j), at(i + 1, j + 1)}); m.primitives.push_back(Vector3ui{at(i, j), at(i + 1, j + 1), at(i, j + 1)}); }
    return m;
}
static ImageData image(uint32_t width, uint32_t height, uint8_t format, bool srgb, float scale) {
    ImageData data;
    data.width = width; data.height = height; data.format = format; data.is_sRGB = srgb;
    for (size_t k = 0; k < size_t(width) * height * 4; ++k) {
        const float value = scale * (rand() / float(RAND_MAX));
        if (format == HIPR_TEXEL_RGBA32F) { uint8_t bytes[4]; std::memcpy(bytes, &value, 4); data.pixels.insert(data.pixels.end(), bytes, bytes + 4); }
        else data.pixels.push_back(uint8_t(255.0f * value));
    }
    return data;
}
static int fail(const char* what) { printf("FAILED: %s\n", what); return 1; }
// Staged, walked, adopted; the description must carry what the walk made. Returns false on any disagreement.
static bool staged_walked_and_adopted(SceneBuilder& sb, uint32_t texture, uint32_t sample_count, const std::vector<HiprLight>& lights, bool expect_disabled) {
    SceneBuilder::StagedEnvironmentBuild staged;
    if (!sb.staged_environment_build(texture, sample_count, staged)) return false;
    const HiprSceneDesc& d = sb.desc();
    const HiprTexture t = d.textures[texture];
    std::vector<uint8_t> texels(d.texels + t.texel_offset, d.texels + d.texel_bytes);      // the texture's own texels first, as the device addresses them
    std::vector<float> pdf(size_t(t.width) * staged.build.pdf_height);
    std::vector<HiprLightSample> samples(staged.build.sample_count);
    HiprLightingResult result = {};
    if (build_host_environment(&t, texels.data(), &staged.build, pdf.data(), pdf.size(), samples.data(), uint32_t(samples.size()), &result) != 0) return false;
    if ((result.importance_sampling_disabled != 0) != expect_disabled) return false;
    pdf.resize(size_t(result.pdf_width) * result.pdf_height);
    samples.resize(result.sample_count);
    const std::vector<float> kept_pdf = pdf;
    if (!sb.adopt_lighting(lights, HIPR_ENVIRONMENT_BUILD, texture, result, std::move(pdf), std::move(samples))) return false;
    const HiprSceneDesc& after = sb.desc();
    if (!after.environment || after.environment->environment_map_ID != int32_t(texture) || after.environment->sample_count != result.sample_count) return false;
    if (std::memcmp(after.environment->per_pixel_PDF, kept_pdf.data(), kept_pdf.size() * sizeof(float)) != 0) return false;
    return after.light_count == lights.size() + (expect_disabled ? 0u : 1u) && (expect_disabled || (after.lights[after.light_count - 1].flags & HIPR_LIGHT_TYPE_MASK) == HIPR_LIGHT_PRESAMPLED_ENVIRONMENT);
}
int main() {
    srand(7);
    SceneBuilder sb;
    const uint32_t matte = sb.add_material(SceneBuilder::make_material(RGB(0.8f), 0.7f, 0.04f, 0.0f));
    const uint32_t mesh = sb.add_mesh(grid(6));
    sb.add_model(mesh, matte, Transform(Vector3f(0, 0, 0)));
    const HiprLight lamp = SceneBuilder::sphere_light(Vector3f(0, 2, 0), RGB(1.0f), 0.1f);
    sb.add_light(lamp);
    const uint32_t smooth = sb.add_texture(image(37, 19, HIPR_TEXEL_RGBA32F, false, 2.0f), true, false, true, true);
    const uint32_t bytes = sb.add_texture(image(70, 131, HIPR_TEXEL_RGBA8, true, 1.0f), false, true, false, false);
    const uint32_t black = sb.add_texture(image(9, 5, HIPR_TEXEL_RGBA32F, false, 0.0f), true, true, true, false);
    sb.finalize();
    std::vector<HiprLight> many(40, lamp);
    for (size_t k = 0; k < many.size(); ++k) many[k].data[3] = 0.1f * float(k);
    if (!staged_walked_and_adopted(sb, smooth, 100, {lamp}, false)) return fail("37 x 19 floats, bilinear");
    if (!sb.set_lights(many) || sb.desc().light_count != 41) return fail("40 lights over a lit scene");
    if (!staged_walked_and_adopted(sb, bytes, 2, {}, false)) return fail("70 x 131 sRGB bytes, nearest");
    if (!staged_walked_and_adopted(sb, black, 16, many, true)) return fail("9 x 5 black floats");
    if (!sb.set_lights({}) || sb.desc().light_count != 0) return fail("no lights under the disabled form");
    HiprLight own = {};
    own.flags = HIPR_LIGHT_PRESAMPLED_ENVIRONMENT;
    if (sb.set_lights({own})) return fail("the environment's light was taken in a list");
    if (!sb.adopt_lighting({lamp}, HIPR_ENVIRONMENT_REMOVE, 0, HiprLightingResult{}, {}, {}) || sb.desc().environment || sb.desc().light_count != 1) return fail("the environment removed");
    SceneBuilder::StagedEnvironmentBuild none;
    if (sb.staged_environment_build(0, 16, none) || sb.staged_environment_build(uint32_t(sb.texture_count()), 16, none)) return fail("a texture the builder does not hold was staged");
    sb.rebuild();
    if (sb.desc().environment || sb.desc().light_count != 1) return fail("a rebuild after the adoptions");
    printf("3 environments staged, walked and adopted; the light list replaced 4 times; the environment removed\n");
    return 0;
}
