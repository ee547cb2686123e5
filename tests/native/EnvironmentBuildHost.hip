// EnvironmentBuildHost.hip -- the routines of hipr_update_scene_lighting's environment build (csrc/environment_build.h), compiled for the HOST by hipcc's host
// pass (tests/native/libenvironment_build_host.so).
//
// Test infrastructure (tests/test_environment_build_on_host_cpu.py, tests/native/EnvironmentBuildSanitize.cpp); nothing here is linked into or loaded by the
// product, which has no CPU path.
//
// build_host_environment walks what ResidentScene::update_lighting queues, in its order and in the kernels' shape: every per-element pass as blocks of ENV_BLOCK
// "threads", the threads of a launch taken BACKWARDS, those past the count doing nothing; the row sums as bands of ENV_BAND_ROWS rows over tiles of
// ENV_TILE_COLUMNS columns staged with the kernel's pitch; the marginal 64 row totals at a time; the normalisation out of the separate buffers; the host's finish.
// The CPU suite holds the result to InfiniteAreaLight + presample_environment byte for byte.
#define HIPR_REBUILD_HOST_ONLY 1
#include <hip/hip_runtime.h>

#include "../../bifrost3d_amd/csrc/environment_build.h"

#include <cstring>
#include <vector>

using namespace hipr;

namespace {

// One launch of a per-element pass: blocks x ENV_BLOCK virtual threads, backwards.
template <typename BODY>
void launch_backwards(size_t count, BODY body) {
    const size_t blocks = (count + ENV_BLOCK - 1) / ENV_BLOCK;
    for (size_t block = blocks; block-- > 0;)
        for (size_t thread = ENV_BLOCK; thread-- > 0;) {
            const size_t i = block * ENV_BLOCK + thread;
            if (i < count) body(i);
        }
}

// k_env_row_sums: one band per block, the tile staged with the kernel's pitch, one virtual lane per row.
void walk_row_sums(const float* function, uint32_t width, uint32_t height, float* conditional) {
    const uint32_t bands = (height + ENV_BAND_ROWS - 1) / ENV_BAND_ROWS;
    for (uint32_t band = bands; band-- > 0;) {
        std::vector<float> tile(size_t(ENV_BAND_ROWS) * ENV_TILE_PITCH, -1.0f);
        float running[ENV_BAND_ROWS] = {};
        const uint32_t first_row = band * uint32_t(ENV_BAND_ROWS);
        for (uint32_t r = 0; r < uint32_t(ENV_BAND_ROWS); ++r)
            if (first_row + r < height) conditional[size_t(first_row + r) * (width + 1)] = 0.0f;
        for (uint32_t first_column = 0; first_column < width; first_column += ENV_TILE_COLUMNS) {
            const uint32_t columns = width - first_column < uint32_t(ENV_TILE_COLUMNS) ? width - first_column : uint32_t(ENV_TILE_COLUMNS);
            for (uint32_t r = ENV_BAND_ROWS; r-- > 0;)
                for (uint32_t lane = ENV_TILE_COLUMNS; lane-- > 0;)
                    if (first_row + r < height && lane < columns) tile[r * ENV_TILE_PITCH + lane] = function[size_t(first_row + r) * width + first_column + lane];
            for (uint32_t r = ENV_BAND_ROWS; r-- > 0;)
                if (first_row + r < height) running[r] = env_sum_tile_row(tile.data() + r * ENV_TILE_PITCH, columns, running[r]);
            for (uint32_t r = ENV_BAND_ROWS; r-- > 0;)
                for (uint32_t lane = ENV_TILE_COLUMNS; lane-- > 0;)
                    if (first_row + r < height && lane < columns) conditional[size_t(first_row + r) * (width + 1) + first_column + lane + 1] = tile[r * ENV_TILE_PITCH + lane];
        }
    }
}

// k_env_marginal: 64 totals staged, one lane sums them in order.
float walk_marginal(const float* conditional, uint32_t width, uint32_t height, float* marginal_raw, float* totals) {
    float staged[64], running = 0.0f;
    marginal_raw[0] = 0.0f;
    for (uint32_t first = 0; first < height; first += 64u) {
        for (uint32_t lane = 64; lane-- > 0;)
            if (first + lane < height) { staged[lane] = conditional[size_t(first + lane) * (width + 1) + width]; totals[first + lane] = staged[lane]; }
        for (uint32_t k = 0; k < 64u && first + k < height; ++k) { running = running + staged[k]; marginal_raw[first + k + 1] = running; }
    }
    return running / float(int(width * height));
}

} // namespace

extern "C" {

// The environment of `texture` (its texels at `texels`) built as hipr_update_scene_lighting builds it. `build` as the entry point takes it (its
// environment_map_ID is not read). Outputs as the entry point's; 0 = done, -1 = what the entry point refuses on the host.
int build_host_environment(const HiprTexture* texture, const uint8_t* texels, const HiprEnvironmentBuild* build, float* out_per_pixel_PDF, uint64_t pdf_capacity, HiprLightSample* out_samples,
                           uint32_t sample_capacity, HiprLightingResult* out) {
    if (!texture || !texels || !build || !out_per_pixel_PDF || !out_samples || !out || !build->row_sines || !build->draw_points) return -1;
    const HiprTexture& t = *texture;
    if ((t.format != HIPR_TEXEL_RGBA8 && t.format != HIPR_TEXEL_RGBA32F) || (t.is_sRGB != 0) != (build->srgb_decode != nullptr) || (t.is_sRGB && t.format == HIPR_TEXEL_RGBA32F)) return -1;
    const uint32_t width = t.width, height = build->pdf_height, samples = build->sample_count;
    if (height != (t.height > ENV_MINIMUM_PDF_HEIGHT ? t.height : ENV_MINIMUM_PDF_HEIGHT) || samples < 2u || (samples & (samples - 1u))) return -1;
    const size_t texel_count = size_t(width) * height;
    if (pdf_capacity < texel_count || sample_capacity < samples) return -1;
    const EnvTexture texture_on_host = {t.width, t.height, t.format, t.wrap_u, t.wrap_v, t.filter, texels, build->srgb_decode};
    const bool blurs = (t.filter & 1u) != 0 || height != t.height;
    std::vector<float> importance(texel_count), blurred(blurs ? texel_count : 0), conditional(size_t(width + 1) * height), marginal_raw(size_t(height) + 1), marginal(size_t(height) + 1), totals(height);
    launch_backwards(texel_count, [&](size_t i) { importance[i] = env_importance(texture_on_host, height, build->row_sines, uint32_t(i % width), uint32_t(i / width)); });
    if (blurs) launch_backwards(texel_count, [&](size_t i) { blurred[i] = env_blur(importance.data(), int(width), int(height), int(i % width), int(i / width)); });
    walk_row_sums(blurs ? blurred.data() : importance.data(), width, height, conditional.data());
    const float integral = walk_marginal(conditional.data(), width, height, marginal_raw.data(), totals.data());
    *out = {};
    if (integral < 0.00001f) {
        out_per_pixel_PDF[0] = 0.0f;
        out_samples[0] = HiprLightSample{{0, 0, 0}, 0.0f, {0, 1, 0}, 0.0f};
        out->pdf_width = out->pdf_height = out->sample_count = 1u;
        out->importance_sampling_disabled = 1u;
        return 0;
    }
    launch_backwards(conditional.size(), [&](size_t i) {
        if (i <= height) marginal[i] = env_normalised_marginal(marginal_raw.data(), height, uint32_t(i));
        conditional[i] = env_normalised_conditional(conditional[i], totals[i / (width + 1)], width, uint32_t(i % (width + 1)));
    });
    const float PDF_scale = float(int(width) * int(height)) * (1.0f / (2.0f * 3.14159265358979323846f * 3.14159265358979323846f));
    launch_backwards(texel_count, [&](size_t i) { out_per_pixel_PDF[i] = env_pdf_texel(marginal.data(), conditional.data(), width, uint32_t(i % width), uint32_t(i / width), PDF_scale); });
    launch_backwards(samples, [&](size_t i) { out_samples[i] = env_draw(texture_on_host, marginal.data(), conditional.data(), width, height, build->draw_points[2 * i], build->draw_points[2 * i + 1]); });
    for (uint32_t i = 0; i < samples; ++i) finish_environment_sample(out_samples[i]);
    out->pdf_width = width; out->pdf_height = height; out->sample_count = samples;
    return 0;
}

}
