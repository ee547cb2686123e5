// material_rules.h -- what a triangle's flags owe to its material: ONE text for the host's scene builder (host/SceneBuilder.cpp finalize, update_materials) and for
// the kernels that apply a material edit to the resident scene (csrc/material_update.h, hipr_update_scene_materials).
//
// The yardstick of a material edit on the device is BYTE EQUALITY with a fresh upload of the edited scene, so both sides run these statements: IEEE f32
// arithmetic in a fixed order, floorf / fabsf exact on either side, and ONE division, float(value) / 255.0f, which is correctly rounded on the host and in the
// device library's scene unit (csrc/scene.hip, built with the traversal unit's flags: correctly rounded division, -ffp-contract=off). NEVER include this header in the fast-math shade unit
// (csrc/shade.hip): its division there is a reciprocal and a product, and a texel at the threshold would flag a triangle differently.
//
// Plain C++ for the host's compiler, __host__ __device__ under hipcc; no HIP header is needed.
#pragma once

#include "../../include/hiprenderer_c.h"

#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define MRHD __host__ __device__ inline
#else
#define MRHD inline
#endif

namespace hipr {

// get_coverage (OptiXRenderer/Types.h:405-414) with no coverage texture: cutout -> (1 < threshold ? 0 : 1), else coverage.
MRHD bool statically_opaque(const HiprMaterial& m) {
    if (m.coverage_texture_ID) return false;
    if (m.flags & HIPR_MATERIAL_CUTOUT) return !(1.0f < m.coverage);
    return m.coverage >= 1.0f;
}

// backside_cull of the hit program (OptiXRenderer/Shading/MonteCarlo.cu:147-164): !hit_from_front && !thin_walled && !transmissive, thin_walled = cut-out or thin-walled.
MRHD bool refuses_hits_from_behind(const HiprMaterial& m) {
    return !(m.flags & (HIPR_MATERIAL_CUTOUT | HIPR_MATERIAL_THIN_WALLED)) && m.shading_model != HIPR_SHADING_TRANSMISSIVE;
}

// The class byte of the listing pass (k_classify_hits): bit 0 = the material carries a coat.
MRHD uint32_t coated_class(const HiprMaterial& m) { return m.coat != 0 ? 1u : 0u; }

// The smaller / larger of two floats as std::min / std::max give them -- the first argument stays unless the second is strictly beyond it -- spelled as a
// comparison and a select, which is one text for both compilers; fminf / fmaxf agree with it on every pair of numbers (the sign of a zero does not survive the
// floorf below) and differ only where a texture coordinate is a NaN, and there the builder's result is the one to keep.
MRHD float rule_min(float a, float b) { return b < a ? b : a; }
MRHD float rule_max(float a, float b) { return a < b ? b : a; }

// A triangle of a material that is NOT statically opaque can still be: where its coverage texture covers it everywhere -- a finely tessellated cut-out surface
// (a fence, a lace banner) has many triangles that lie wholly on solid texels. Those get HIPR_TRIANGLE_OPAQUE too, and a shadow ray that hits one ends without
// the material -> texture -> texel lookups; get_coverage (OptiXRenderer/Types.h:405-414) would have returned 1 for every point of the triangle, so nothing changes
// for the reference's any-hit program, the oracle's or the kernels'. Decided conservatively from the texels the sampler can touch for ANY point of the triangle:
// the texture coordinates of its points lie in the bounding box of its corners' (the interpolation's rounding is covered by a texel of slack on every side), so
// every texel under that box, plus the bilinear neighbour, must pass. 8-bit linear textures only; boxes of more than 64 x 64 texels are left to the sampler.
MRHD bool covered_everywhere(const HiprMaterial& m, const HiprTexture& t, const uint8_t* texels, const float (&uv)[3][2]) {
    if ((t.format != HIPR_TEXEL_R8 && t.format != HIPR_TEXEL_RGBA8) || t.is_sRGB || t.width == 0 || t.height == 0) return false;
    const bool cutout = (m.flags & HIPR_MATERIAL_CUTOUT) != 0;
    if (!cutout && !(m.coverage >= 1.0f)) return false;
    const bool linear = (t.filter & 1) != 0;
    const int size[2] = {int(t.width), int(t.height)};
    int first[2], last[2];
    for (int a = 0; a < 2; ++a) {
        const float lo = rule_min(uv[0][a], rule_min(uv[1][a], uv[2][a])) * float(size[a]), hi = rule_max(uv[0][a], rule_max(uv[1][a], uv[2][a])) * float(size[a]);
        if (!(fabsf(lo) < 1048576.0f) || !(fabsf(hi) < 1048576.0f)) return false;      // also NaN
        first[a] = int(floorf(lo - (linear ? 0.5f : 0.0f))) - 1;
        last[a] = int(floorf(hi - (linear ? 0.5f : 0.0f))) + (linear ? 1 : 0) + 1;
        if (last[a] - first[a] + 1 > 64) return false;
    }
    const int channels = t.format == HIPR_TEXEL_RGBA8 ? 4 : 1;
    const uint8_t* base = texels + t.texel_offset;
    for (int y = first[1]; y <= last[1]; ++y)
        for (int x = first[0]; x <= last[0]; ++x) {
            int wrapped[2] = {x, y};
            for (int a = 0; a < 2; ++a) {
                int i = wrapped[a];
                const int n = size[a];
                if (a == 0 ? t.wrap_u != 0 : t.wrap_v != 0) { i %= n; i = i < 0 ? i + n : i; }
                else i = i < 0 ? 0 : (i >= n ? n - 1 : i);
                wrapped[a] = i;
            }
            const uint8_t value = base[(size_t(wrapped[1]) * t.width + size_t(wrapped[0])) * size_t(channels)];      // the sampler's .x
            // cut-out: the sampled value must not fall below the threshold -- with a margin that a bilinear blend of passing texels cannot round through;
            // plain coverage: coverage * texture must be 1, i.e. every texel exactly 1
            if (cutout ? !(float(value) / 255.0f > m.coverage + 1e-5f) : value != 255) return false;
        }
    return true;
}

// The coverage texture that can still make a triangle of `m` opaque, or nullptr: the material is not statically opaque and names a texture of the pool.
MRHD const HiprTexture* deciding_coverage_texture(const HiprMaterial& m, const HiprTexture* textures, uint32_t texture_count) {
    if (statically_opaque(m) || !(m.coverage_texture_ID > 0) || uint32_t(m.coverage_texture_ID) >= texture_count) return nullptr;
    return textures + m.coverage_texture_ID;
}

// HiprTriangle::flags of a triangle of material `m`. `texture`: deciding_coverage_texture(m, ...); `uv`: the texture coordinates of the triangle's corners (zeros
// for a mesh without), read only when `texture` is not null.
MRHD uint32_t triangle_flags(const HiprMaterial& m, const HiprTexture* texture, const uint8_t* texels, const float (&uv)[3][2]) {
    const bool opaque = texture ? covered_everywhere(m, *texture, texels, uv) : statically_opaque(m);
    return (opaque ? uint32_t(HIPR_TRIANGLE_OPAQUE) : 0u) | (refuses_hits_from_behind(m) ? uint32_t(HIPR_TRIANGLE_ONE_SIDED) : 0u);
}

// ... with the corners' texture coordinates fetched the way the builder and the shading records do: through the instance's index triple into the pooled
// attribute, when the mesh has the attribute. `texcoords` may be null when no mesh has.
MRHD uint32_t triangle_flags(const HiprMaterial& m, const HiprInstance& inst, uint32_t primitive_index, const uint32_t* indices, const float* texcoords,
                             const HiprTexture* textures, uint32_t texture_count, const uint8_t* texels) {
    const HiprTexture* texture = deciding_coverage_texture(m, textures, texture_count);
    float uv[3][2] = {{0, 0}, {0, 0}, {0, 0}};
    if (texture && (inst.mesh_flags & HIPR_MESH_TEXCOORDS) && texcoords) {
        const uint32_t* idx = indices + 3 * size_t(inst.index_offset + primitive_index);
        for (int k = 0; k < 3; ++k) { uv[k][0] = texcoords[2 * size_t(inst.vertex_offset + idx[k])]; uv[k][1] = texcoords[2 * size_t(inst.vertex_offset + idx[k]) + 1]; }
    }
    return triangle_flags(m, texture, texels, uv);
}

// Bits 0..3 of HiprLeaf8::flags from the flags of the record's triangles (host/Wide8Builder.cpp make_record): A / B opaque, A / B one-sided.
MRHD uint32_t leaf_material_bits(const HiprTriangle* triangles, const HiprLeaf8& leaf) {
    const uint32_t a = triangles[leaf.triangle[0]].flags;
    uint32_t bits = (a & HIPR_TRIANGLE_OPAQUE ? 1u : 0u) | (a & HIPR_TRIANGLE_ONE_SIDED ? 4u : 0u);
    if (leaf.triangle[1] != HIPR_LEAF8_NONE) {
        const uint32_t b = triangles[leaf.triangle[1]].flags;
        bits |= (b & HIPR_TRIANGLE_OPAQUE ? 2u : 0u) | (b & HIPR_TRIANGLE_ONE_SIDED ? 8u : 0u);
    }
    return bits;
}

} // namespace hipr
