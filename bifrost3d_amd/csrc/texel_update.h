// texel_update.h -- pixel edits of resident images applied to the resident scene on the device (hipr_update_scene_texels): rectangles of new texels are a copy into
// the texel pool plus what an upload DERIVES from texels -- HiprTriangle::flags & HIPR_TRIANGLE_OPAQUE of the triangles whose material leaves the decision to its
// coverage texture (covered_everywhere, material_rules.h), its copy in the trace records, bits 0..3 of the leaf records and all_triangles_opaque. (The reference
// asserts "Pixel update not implemented yet", OR/Renderer.cpp:697-698.)
//
// The yardstick is BYTE EQUALITY with a fresh upload of the edited scene. A texel moves no corner and no tree builder reads a flag, so the trees, the triangle order
// and the record pairing of a fresh build are the resident ones. The passes, all on the context's stream, one after the other; no block waits on another, the
// reductions are an integer AND and two counts, which are order independent:
//   pass 1  k_write_texel_rectangle       once per rectangle, in list order (where two overlap the later one wins): the rows the host packed into ONE staging buffer
//                                         go into the pool, a thread per 4 bytes of a row; no byte outside the rectangle is written, and a row of R8 texels may begin
//                                         at any byte address (the ends of such a row go byte by byte).
//   pass 2  k_reflag_touched_triangles    one thread per triangle: the body of the material edit's pass (update_triangle_material, material_update.h) with `touched`
//                                         set for every instance whose material's deciding coverage texture is an edited one -- each such triangle scans its box of
//                                         texels again -- and, around it, the counts of the triangles decided again and of those whose flags changed, by wave ballots
//                                         and at most one atomic per wave and word.
//   pass 3  k_update_leaf_flags           (material_update.h, unchanged) when a flag changed.
// Pass 2 was measured against a two-pass form -- one thread per triangle marks the triangles whose box of texels (coverage_box) meets a rectangle, one wave per
// marked triangle decides it with its lanes over the columns of the box -- on the 251 k atrium's lace banners, and is 3 to 10 times faster there
// (profiles/texel_update_wave_per_candidate_rejected.txt): the banners' boxes are a few texels wide, so 64 lanes per box idle more than one lane scans. That form was
// removed. Nothing was done about narrow loads of R8 rows either: a lane reads its own box, a few bytes per row.
//
// The bodies are __host__ __device__ so that tests/native/TexelUpdateHost.hip can compile them for the host and the CPU suite can hold them to
// SceneBuilder::update_texels without a GPU. This header includes material_rules.h: it must NEVER reach the fast-math shade unit (see there).
#pragma once

#include "material_update.h"

#include <cstring>

namespace hipr {

inline uint32_t texel_bytes_of(uint8_t format) { return format == HIPR_TEXEL_R8 ? 1u : (format == HIPR_TEXEL_RGBA8 || format == HIPR_TEXEL_R32F ? 4u : (format == HIPR_TEXEL_RGBA32F ? 16u : 0u)); }

// One rectangle as the device takes it. Its rows lie in the staging buffer from `staging_offset` on, `staging_pitch` (a multiple of 4) apart.
struct TexelRectangle {
    uint64_t staging_offset;
    uint64_t pool_offset;               // of the rectangle's first byte in the texel pool
    uint64_t pool_pitch;                // bytes of a row of the texture
    uint64_t row_bytes, staging_pitch;
    uint32_t height, pad;
};

// The rectangle of edit `e` of texture `t` (checked: hipr_update_scene_texels' refusals), its rows placed at the end of a staging buffer of `staging_bytes` so far.
inline TexelRectangle planned_rectangle(const HiprTexelEdit& e, const HiprTexture& t, uint64_t& staging_bytes) {
    const uint64_t size = texel_bytes_of(t.format), row_bytes = uint64_t(e.width) * size;
    const TexelRectangle r = {staging_bytes, t.texel_offset + (uint64_t(e.y) * t.width + e.x) * size, uint64_t(t.width) * size, row_bytes, (row_bytes + 3u) & ~uint64_t(3), e.height, 0u};
    staging_bytes += r.staging_pitch * e.height;
    return r;
}
// ... and its rows packed there, from the caller's pitch.
inline void pack_rectangle_rows(const HiprTexelEdit& e, const TexelRectangle& r, uint8_t* staging) {
    for (uint32_t row = 0; row < e.height; ++row)
        std::memcpy(staging + r.staging_offset + row * r.staging_pitch, static_cast<const uint8_t*>(e.texels) + row * e.row_pitch_bytes, r.row_bytes);
}

// Pass 1 for 4-byte chunk `chunk` of row `row`: aligned words where the pool's address allows, bytes at a row's odd ends.
MRHD void write_texel_chunk(const TexelRectangle& r, const uint8_t* staging, uint8_t* pool, uint32_t row, uint32_t chunk) {
    const uint64_t at = uint64_t(chunk) * 4u;
    if (row >= r.height || at >= r.row_bytes) return;
    const uint8_t* from = staging + r.staging_offset + uint64_t(row) * r.staging_pitch + at;
    uint8_t* to = pool + r.pool_offset + uint64_t(row) * r.pool_pitch + at;
    const uint32_t n = r.row_bytes - at < 4u ? uint32_t(r.row_bytes - at) : 4u;
    if (n == 4u && (reinterpret_cast<uintptr_t>(to) & 3u) == 0) *reinterpret_cast<uint32_t*>(to) = *reinterpret_cast<const uint32_t*>(from);
    else for (uint32_t b = 0; b < n; ++b) to[b] = from[b];
}

// The words of pass 2: the AND of "opaque" (preset to 1), the triangles decided again, the triangles whose flags changed.
constexpr uint32_t TEXEL_WORD_OPAQUE = 0, TEXEL_WORD_DECIDED = 1, TEXEL_WORD_CHANGED = 2, TEXEL_SCRATCH_WORDS = 16;

// Pass 2 for triangle t: the material edit's pass, which recomputes a triangle of a touched instance from the texels as they now stand and leaves the others alone
// (the material index and the class byte it writes beside the flags are the resident ones again), and what the triangle adds to the AND and the two counts.
MRHD void reflag_triangle(const MaterialUpdateArrays& a, uint32_t t, bool& opaque, bool& decided, bool& changed) {
    const uint32_t before = a.triangles[t].flags;
    decided = a.touched[a.triangles[t].instance_index] != 0;
    bool coated;
    update_triangle_material(a, t, opaque, coated);
    changed = a.triangles[t].flags != before;
}

#if defined(__HIPCC__) && !defined(HIPR_MATERIAL_UPDATE_HOST_ONLY)      // the kernels; a host build of the bodies (tests/native/TexelUpdateHost.hip) leaves them out

constexpr int TEXEL_UPDATE_BLOCK = 256;

// grid: (chunks of a row / block, rows), rows folded into blockIdx.y up to the grid's limit and walked beyond it
__global__ __launch_bounds__(TEXEL_UPDATE_BLOCK) void k_write_texel_rectangle(TexelRectangle r, const uint8_t* __restrict__ staging, uint8_t* __restrict__ pool) {
    const uint32_t chunk = blockIdx.x * uint32_t(TEXEL_UPDATE_BLOCK) + threadIdx.x;
    for (uint32_t row = blockIdx.y; row < r.height; row += gridDim.y) write_texel_chunk(r, staging, pool, row, chunk);
}

// words[TEXEL_WORD_OPAQUE] preset to 1, the others to 0
__global__ __launch_bounds__(TEXEL_UPDATE_BLOCK) void k_reflag_touched_triangles(MaterialUpdateArrays a, uint32_t* __restrict__ words) {
    const uint32_t t = blockIdx.x * uint32_t(TEXEL_UPDATE_BLOCK) + threadIdx.x;
    bool opaque = true, decided = false, changed = false;      // neutral: the threads past the end
    if (t < a.triangle_count) reflag_triangle(a, t, opaque, decided, changed);
    const unsigned long long not_opaque = __ballot(!opaque), were_decided = __ballot(decided), have_changed = __ballot(changed);
    if ((threadIdx.x & 63u) == 0) {
        if (not_opaque) atomicAnd(&words[TEXEL_WORD_OPAQUE], 0u);
        if (were_decided) atomicAdd(&words[TEXEL_WORD_DECIDED], uint32_t(__popcll(were_decided)));
        if (have_changed) atomicAdd(&words[TEXEL_WORD_CHANGED], uint32_t(__popcll(have_changed)));
    }
}

#endif // the kernels

} // namespace hipr
