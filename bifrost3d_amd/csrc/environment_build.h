// environment_build.h -- the device work of hipr_update_scene_lighting's environment rebuild: the per-texel PDF image and the presampled light samples of a
// latitude-longitude environment map made ON THE DEVICE from the texture the resident texel pool already holds, so that swapping the sky costs no flatten, no
// tree build and no upload of any pool (the reference builds its presampled environment without touching geometry, OR/Renderer.cpp:1136-1196,
// OR/PresampledEnvironmentMap.cpp:19-101).
//
// The yardstick is BYTE EQUALITY with the host path: Assets::InfiniteAreaLight (host/InfiniteAreaLight.cpp: compute_distribution, Distribution2D's constructor,
// sample_continuous, reconstruct_solid_angle_PDF_sans_sin_theta) and HIPRenderer::presample_environment. The routines below restate those, and the host's own
// get_pixel / sample2D for RGBA8 and RGBA32F, term for term -- NOT kernels.h's sample_texture, whose arithmetic differs (truncation against floorf, the
// magnification bit against the minification bit). What the host evaluates through libm comes in as tables that do not depend on the texels: the sine of every PDF
// row (std::sin) and the linear value of every sRGB byte (std::pow), microseconds to fill, and the PMJ-BN draw points, which depend on the sample count alone (61 ms at
// 8192 points: the scene builder makes them once per count). What is left is + - * /, comparisons and conversions, correctly rounded
// f32 without contraction on both sides (Makefile: -ffp-contract=off), denormals kept, no float atomics: equality holds by construction.
//
// Passes, one launch each, nothing waits on another block:
//   k_env_importance   one thread per PDF texel: (r + g + b) * row_sines[y]; the pixel by get_pixel, or -- a texture lower than the PDF image -- by sample2D at
//                      ((x + .5) / w, (y + .5) / pdf_height)
//   k_env_blur         where the texture magnifies linearly or was resampled: the 3x3 tent in the host's accumulation order, repeating horizontally, clamped vertically
//   k_env_row_sums     row[x + 1] = row[x] + f[x], a strictly sequential f32 chain per row (a scan would reassociate it): parallel over rows only. A block takes a
//                      band of ENV_BAND_ROWS rows and walks it in tiles of ENV_TILE_COLUMNS columns: the tile is loaded coalesced -- a wave instruction reads 64
//                      consecutive floats of ONE row -- into LDS with an odd row pitch (65 words: the lanes of a wave's load and the lanes that then walk one row
//                      each both fall on distinct banks), each of the band's lanes adds its own row's values in order from LDS and leaves the running sums there,
//                      and they go back to memory the way the values came
//   k_env_marginal     one wave: the row totals staged 64 at a time, ONE lane sums them in order; leaves the running sums, the totals and the integral
//   k_env_normalise    one thread per entry, out of the marginal's separate unnormalised buffer and the separate totals: no thread reads what another overwrites
//   k_env_pdf_image    one thread per texel, straight into the new resident PDF buffer
//   k_env_draws        one thread per sample: two binary searches, the inverse lerps, the discrete PDF x w x h, uv, the radiance by sample2D; writes uv, that PDF and
//                      the radiance into the sample's record
// The finish runs on the HOST inside the library (finish_environment_sample): the direction by std::sin / std::cos, sin_theta, PDF / (2 pi^2 sin_theta), the
// distance -- sample_count x 32 bytes read back and uploaded once. That keeps libm out of the device.
//
// Everything but the kernels is __host__ __device__ so that the CPU suite can walk it against the host path (tests/native/EnvironmentBuildHost.hip).
#pragma once

#include "../../include/hiprenderer_c.h"

#include <cmath>
#include <cstddef>
#include <cstdint>

#ifndef BHD
#define BHD __host__ __device__ inline
#endif

namespace hipr {

constexpr int ENV_BLOCK = 256;            // the per-element passes
constexpr int ENV_BAND_ROWS = 32;         // rows of a block of k_env_row_sums: one lane each in the sequential phase
constexpr int ENV_TILE_COLUMNS = 64;      // one wave load instruction = 64 consecutive floats of one row
constexpr int ENV_TILE_PITCH = ENV_TILE_COLUMNS + 1;
constexpr uint32_t ENV_MINIMUM_PDF_HEIGHT = 128;      // InfiniteAreaLight::MINIMUM_PDF_HEIGHT

// The resident environment texture: its record, its texels where the pool holds them, and the sRGB table (null for a linear texture).
struct EnvTexture {
    uint32_t width, height;
    uint8_t format, wrap_u, wrap_v, filter;
    const uint8_t* texels;
    const float* srgb_decode;
};
struct EnvRGB { float r, g, b; };

// Assets::get_pixel for RGBA32 and RGBA_Float, colour channels only (nothing here reads alpha). The index is clamped into the image: the host's are in range, a
// clamp changes none of them, and no lane ever reads outside the texture.
BHD EnvRGB env_get_pixel(const EnvTexture& t, uint32_t x, uint32_t y) {
    x = x < t.width ? x : t.width - 1u;
    y = y < t.height ? y : t.height - 1u;
    const size_t index = x + size_t(y) * t.width;
    if (t.format == HIPR_TEXEL_RGBA32F) {
        const float* floats = reinterpret_cast<const float*>(t.texels);
        return {floats[4 * index], floats[4 * index + 1], floats[4 * index + 2]};
    }
    const uint8_t* bytes = t.texels + 4 * index;
    if (t.srgb_decode) return {t.srgb_decode[bytes[0]], t.srgb_decode[bytes[1]], t.srgb_decode[bytes[2]]};
    const float unorm8 = 1.0f / 255.0f;
    return {bytes[0] * unorm8, bytes[1] * unorm8, bytes[2] * unorm8};
}

BHD float env_wrap(float t, bool clamp) {
    const float nearly_one = 0xffffff / float(1 << 24);
    if (clamp) return fminf(fmaxf(t, 0.0f), nearly_one);
    t -= float(int(t));
    return t < -0.0f ? t + 1.0f : t;
}

BHD EnvRGB env_lerp(EnvRGB a, EnvRGB b, float t) { return {a.r + (b.r - a.r) * t, a.g + (b.g - a.g) * t, a.b + (b.b - a.b) * t}; }

// Assets::sample2D: the MINIFICATION bit chooses between nearest and bilinear, as on the host.
BHD EnvRGB env_sample2D(const EnvTexture& t, float u, float v) {
    const bool clamp_u = t.wrap_u == 0, clamp_v = t.wrap_v == 0;
    u = env_wrap(u, clamp_u);
    v = env_wrap(v, clamp_v);
    const int width = int(t.width), height = int(t.height);
    if (!(t.filter & 2u)) return env_get_pixel(t, unsigned(u * float(width)), unsigned(v * float(height)));

    const float px = u * float(width) - 0.5f, py = v * float(height) - 0.5f;
    const int x0 = int(px), y0 = int(py);
    float u_lerp = px - float(x0), v_lerp = py - float(y0);
    if (u_lerp < 0.0f) u_lerp += 1.0f;
    if (v_lerp < 0.0f) v_lerp += 1.0f;
    auto lookup = [&](int x, int y) {
        x = clamp_u ? (x < 0 ? 0 : (x > width - 1 ? width - 1 : x)) : (x + width) % width;
        y = clamp_v ? (y < 0 ? 0 : (y > height - 1 ? height - 1 : y)) : (y + height) % height;
        return env_get_pixel(t, unsigned(x), unsigned(y));
    };
    const EnvRGB lower = env_lerp(lookup(x0, y0), lookup(x0 + 1, y0), u_lerp), upper = env_lerp(lookup(x0, y0 + 1), lookup(x0 + 1, y0 + 1), u_lerp);
    return env_lerp(lower, upper, v_lerp);
}

// compute_distribution's first loop for PDF texel (x, y). `pdf_height` = max(texture height, 128); a lower texture is resampled.
BHD float env_importance(const EnvTexture& t, uint32_t pdf_height, const float* row_sines, uint32_t x, uint32_t y) {
    const int width = int(t.width), height = int(pdf_height);
    const EnvRGB pixel = pdf_height != t.height ? env_sample2D(t, (int(x) + 0.5f) / width, (int(y) + 0.5f) / height) : env_get_pixel(t, x, y);
    return (pixel.r + pixel.g + pixel.b) * row_sines[y];
}

// compute_distribution's second loop: left column, right column, middle column, centre last.
BHD float env_blur(const float* importance, int width, int height, int x, int y) {
    const int below = y - 1 < 0 ? 0 : y - 1, above = y + 1 > height - 1 ? height - 1 : y + 1;
    const int left = x - 1 < 0 ? width - 1 : x - 1, right = x + 1 == width ? 0 : x + 1;
    auto at = [&](int px, int py) { return importance[px + size_t(py) * width]; };
    float sum = 0.0f;
    sum += at(left, below); sum += at(left, y) * 2.0f; sum += at(left, above);
    sum += at(right, below); sum += at(right, y) * 2.0f; sum += at(right, above);
    sum += at(x, below) * 2.0f; sum += at(x, above) * 2.0f;
    sum += at(x, y) * 20.0f;
    return sum / 32.0f;
}

// Distribution2D's normalisation. Entry i of the marginal (height + 1 entries), out of the unnormalised sums.
BHD float env_normalised_marginal(const float* raw, uint32_t height, uint32_t i) {
    if (i == 0) return raw[0];
    if (i == height) return 1.0f;
    return raw[i] / raw[height];
}
// Entry x of a conditional row (width + 1 entries), given its value and the row's unnormalised total.
BHD float env_normalised_conditional(float value, float total, uint32_t width, uint32_t x) {
    if (x == width) return 1.0f;
    if (x == 0 || !(total > 0.0f)) return value;
    return value / total;
}

// reconstruct_solid_angle_PDF_sans_sin_theta for one texel.
BHD float env_pdf_texel(const float* marginal, const float* conditional, uint32_t width, uint32_t x, uint32_t y, float PDF_scale) {
    const float marginal_PDF = marginal[y + 1] - marginal[y];
    const float* c = conditional + x + size_t(y) * (width + 1);
    return marginal_PDF * (c[1] - c[0]) * PDF_scale;
}

BHD int env_find_interval(float random_sample, const float* CDF, int count) {
    int lower = 0, upper = count;
    while (lower + 1 != upper) {
        const int middle = (lower + upper) / 2;
        if (random_sample < CDF[middle]) upper = middle;
        else lower = middle;
    }
    return lower;
}

// Distribution2D::sample_continuous + InfiniteAreaLight::sample's radiance. The record leaves here with uv in direction_to_light[0..1] and the image-space PDF in
// PDF; finish_environment_sample turns it into the light sample.
BHD HiprLightSample env_draw(const EnvTexture& t, const float* marginal, const float* conditional, uint32_t pdf_width, uint32_t pdf_height, float draw_x, float draw_y) {
    const int width = int(pdf_width), height = int(pdf_height);
    const int y = env_find_interval(draw_y, marginal, height);
    const float dy = (draw_y - marginal[y]) / (marginal[y + 1] - marginal[y]);
    const float* row = conditional + size_t(y) * (width + 1);
    const int x = env_find_interval(draw_x, row, width);
    const float dx = (draw_x - row[x]) / (row[x + 1] - row[x]);
    const float PDF = (marginal[y + 1] - marginal[y]) * (row[x + 1] - row[x]) * width * height;
    const float u = float(x + dx) / width, v = float(y + dy) / height;
    const EnvRGB radiance = env_sample2D(t, u, v);
    return {{radiance.r, radiance.g, radiance.b}, PDF, {u, v, 0.0f}, 0.0f};
}

// The host's finish of a drawn record, restated beside latlong_texcoord_to_direction (host/Math.h:59-63) and InfiniteAreaLight::sample: libm stays on the host.
inline void finish_environment_sample(HiprLightSample& s) {
    const float pi = 3.14159265358979323846f;
    const float phi = s.direction_to_light[0] * 2.0f * pi, theta = s.direction_to_light[1] * pi;
    const float sin_theta_uv = std::sin(theta);
    const float dx = -(sin_theta_uv * std::cos(phi)), dy = -std::cos(theta), dz = -(sin_theta_uv * std::sin(phi));
    s.direction_to_light[0] = dx; s.direction_to_light[1] = dy; s.direction_to_light[2] = dz;
    s.distance = 1e30f;
    const float sin_theta = std::fabs(std::sqrt(1.0f - dy * dy));
    const float pdf = s.PDF / (2.0f * pi * pi * sin_theta);
    s.PDF = sin_theta == 0.0f ? 0.0f : pdf;
}

// One band of k_env_row_sums in the kernel's shape, for one "thread" `row_in_band` of the sequential phase over one staged tile: adds the tile's `columns` values
// to `running` in order and leaves the running sums in their place.
BHD float env_sum_tile_row(float* tile_row, uint32_t columns, float running) {
    for (uint32_t c = 0; c < columns; ++c) { running = running + tile_row[c]; tile_row[c] = running; }
    return running;
}

#if defined(__HIPCC__) && !defined(HIPR_REBUILD_HOST_ONLY)      // the kernels; a host build of the routines (tests/native/EnvironmentBuildHost.hip) leaves them out

__global__ __launch_bounds__(ENV_BLOCK) void k_env_importance(EnvTexture t, uint32_t pdf_height, const float* __restrict__ row_sines, float* __restrict__ importance) {
    const size_t i = size_t(blockIdx.x) * ENV_BLOCK + threadIdx.x;
    if (i >= size_t(t.width) * pdf_height) return;
    importance[i] = env_importance(t, pdf_height, row_sines, uint32_t(i % t.width), uint32_t(i / t.width));
}

__global__ __launch_bounds__(ENV_BLOCK) void k_env_blur(const float* __restrict__ importance, uint32_t width, uint32_t height, float* __restrict__ blurred) {
    const size_t i = size_t(blockIdx.x) * ENV_BLOCK + threadIdx.x;
    if (i >= size_t(width) * height) return;
    blurred[i] = env_blur(importance, int(width), int(height), int(i % width), int(i / width));
}

// conditional: (width + 1) entries per row, unnormalised.
__global__ __launch_bounds__(ENV_BLOCK) void k_env_row_sums(const float* __restrict__ function, uint32_t width, uint32_t height, float* __restrict__ conditional) {
    __shared__ float tile[ENV_BAND_ROWS * ENV_TILE_PITCH];
    const uint32_t first_row = blockIdx.x * uint32_t(ENV_BAND_ROWS);
    const uint32_t lane = threadIdx.x % ENV_TILE_COLUMNS, wave = threadIdx.x / ENV_TILE_COLUMNS;
    constexpr uint32_t WAVES = ENV_BLOCK / ENV_TILE_COLUMNS;
    const bool walks = threadIdx.x < uint32_t(ENV_BAND_ROWS) && first_row + threadIdx.x < height;
    float running = 0.0f;
    if (walks) conditional[size_t(first_row + threadIdx.x) * (width + 1)] = 0.0f;
    for (uint32_t first_column = 0; first_column < width; first_column += ENV_TILE_COLUMNS) {
        const uint32_t columns = width - first_column < uint32_t(ENV_TILE_COLUMNS) ? width - first_column : uint32_t(ENV_TILE_COLUMNS);
        for (uint32_t r = wave; r < uint32_t(ENV_BAND_ROWS); r += WAVES)
            if (first_row + r < height && lane < columns) tile[r * ENV_TILE_PITCH + lane] = function[size_t(first_row + r) * width + first_column + lane];
        __syncthreads();
        if (walks) running = env_sum_tile_row(tile + threadIdx.x * ENV_TILE_PITCH, columns, running);
        __syncthreads();
        for (uint32_t r = wave; r < uint32_t(ENV_BAND_ROWS); r += WAVES)
            if (first_row + r < height && lane < columns) conditional[size_t(first_row + r) * (width + 1) + first_column + lane + 1] = tile[r * ENV_TILE_PITCH + lane];
        __syncthreads();
    }
}

// One wave. marginal_raw: height + 1 running sums; totals: the row totals as the conditional rows hold them; integral[0] = marginal_raw[height] / (width * height).
__global__ __launch_bounds__(64) void k_env_marginal(const float* __restrict__ conditional, uint32_t width, uint32_t height, float* __restrict__ marginal_raw, float* __restrict__ totals,
                                                     float* __restrict__ integral) {
    __shared__ float staged[64];
    float running = 0.0f;
    if (threadIdx.x == 0) marginal_raw[0] = 0.0f;
    for (uint32_t first = 0; first < height; first += 64u) {
        const uint32_t y = first + threadIdx.x;
        if (y < height) { const float total = conditional[size_t(y) * (width + 1) + width]; staged[threadIdx.x] = total; totals[y] = total; }
        __syncthreads();
        if (threadIdx.x == 0)
            for (uint32_t k = 0; k < 64u && first + k < height; ++k) { running = running + staged[k]; marginal_raw[first + k + 1] = running; }
        __syncthreads();
    }
    if (threadIdx.x == 0) integral[0] = running / float(int(width * height));
}

__global__ __launch_bounds__(ENV_BLOCK) void k_env_normalise(const float* __restrict__ marginal_raw, const float* __restrict__ totals, uint32_t width, uint32_t height, float* __restrict__ marginal,
                                                             float* __restrict__ conditional) {
    const size_t i = size_t(blockIdx.x) * ENV_BLOCK + threadIdx.x;
    if (i <= height) marginal[i] = env_normalised_marginal(marginal_raw, height, uint32_t(i));
    if (i >= size_t(width + 1) * height) return;
    const uint32_t x = uint32_t(i % (width + 1)), y = uint32_t(i / (width + 1));
    conditional[i] = env_normalised_conditional(conditional[i], totals[y], width, x);
}

__global__ __launch_bounds__(ENV_BLOCK) void k_env_pdf_image(const float* __restrict__ marginal, const float* __restrict__ conditional, uint32_t width, uint32_t height, float PDF_scale,
                                                             float* __restrict__ per_pixel_PDF) {
    const size_t i = size_t(blockIdx.x) * ENV_BLOCK + threadIdx.x;
    if (i >= size_t(width) * height) return;
    per_pixel_PDF[i] = env_pdf_texel(marginal, conditional, width, uint32_t(i % width), uint32_t(i / width), PDF_scale);
}

__global__ __launch_bounds__(ENV_BLOCK) void k_env_draws(EnvTexture t, const float* __restrict__ marginal, const float* __restrict__ conditional, uint32_t pdf_height,
                                                         const float* __restrict__ draw_points, uint32_t sample_count, HiprLightSample* __restrict__ samples) {
    const uint32_t i = blockIdx.x * uint32_t(ENV_BLOCK) + threadIdx.x;
    if (i >= sample_count) return;
    samples[i] = env_draw(t, marginal, conditional, t.width, pdf_height, draw_points[2 * i], draw_points[2 * i + 1]);
}

#endif

} // namespace hipr
