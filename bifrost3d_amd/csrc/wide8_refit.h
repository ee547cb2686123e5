// wide8_refit.h -- transform-only scene changes on the device: the 8-wide tree (include/hiprenderer_c.h "wide8") refitted to moved instances by a few
// kernels over the arrays that are resident anyway, instead of a host refit and a re-upload of the scene (hipr_refit_scene_transforms; the reference refits
// its root acceleration structure when a node moves, OR/Renderer.cpp:472,1010-1041).
//
// The yardstick is BIT EQUALITY with the host's refit (host/Wide8Builder.cpp refit_wide8 after host/SceneBuilder.cpp update_model_transforms): the routines
// below restate make_record, quantise_node and set_grid of Wide8Builder.cpp operation for operation -- the two libraries do not link each other -- as
// __host__ __device__ functions, so that tests/native/DeviceRefitHost.hip can compile them for the host and the CPU suite can compare them with refit_wide8
// without a GPU. Everything is IEEE f32 / f64 arithmetic in a fixed order (the unit is built with -ffp-contract=off); floor, ceil, ldexp and the f64 division
// are exact / correctly rounded on both sides.
//
// The one place where the host's code is not a specification: quantise_node seeds its search for the smallest fitting exponent with
// ceil(std::log2(extent / 255)), and the last bit of log2 is the C library's business. refit_quantise_node starts from k - 8 instead, k = ilogb(extent) taken
// from the bits, and takes the first exponent that fits. That is the host's result, because
//   (1) no exponent e <= k - 8 fits: a fit needs origin + hi * 2^e >= all.hi with hi <= 255 for the child that reaches all.hi, but 255 * 2^(k - 8) falls short
//       of extent >= 2^k by 2^(k - 8), far more than the rounding of that f64 sum can bridge (origin and all.hi are f32 values, so a non-zero extent is at
//       least 2^-24 of their magnitude and 2^(k - 8) at least 2^-32 of it, against a half ulp of 2^-53);
//   (2) the host's seed is k - 7 or k - 6: 2^(k - 8) * 256 / 255 <= extent / 255 < 2^(k - 7) * 256 / 255, so log2 lies in [k - 8 + 0.0056, k - 7 + 0.0056), which
//       any log2 accurate to a few ulp rounds up to k - 7 or k - 6;
//   (3) where the seed is k - 6, k - 7 does not fit: log2(q) > k - 7 means q = fl(extent / 255) > 2^(k - 7) (log2 of a power of two is exact and log2 is
//       monotone), hence all.hi - origin > 255 * 2^(k - 7) in the reals, and origin + 255 * 2^(k - 7) -- exact in f64 for f32 operands this close -- stays below all.hi.
// So both searches return the first fitting exponent from k - 7 on. tests/test_device_refit_on_host_cpu.py sweeps the corner cases (extents of 255 * 2^n and
// their neighbours, zero extents, boxes at the ends of the grid) against the host's routine.
//
// Passes (all on the context's stream, one after the other; nothing waits on another block, nothing spins):
//   1  k_refit_triangles   one thread per triangle: triangles of moved instances recomputed from the object-space pools with SceneBuilder's expression; the
//                          scene's bounds reduced by min / max (wave shuffles, LDS, per-block partials), k_refit_bounds_final folds the partials. No atomics.
//   2  k_refit_leaves      one thread per leaf record: the record rebuilt, its exact box written. A record that can no longer hold both of its triangles
//                          raises the rebuild flag and is left as it was.
//   3  k_refit_nodes       one launch per level, deepest first: a node gathers its children's exact boxes and requantises them.
//   4  k_refit_area        half area of every child box (f32, as Box::half_area), summed in f64 by a fixed-shape reduction: equal run to run.
#pragma once

#include "../../include/hiprenderer_c.h"

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#define RHD __host__ __device__ inline

namespace hipr {

struct RefitBox { float lo[3], hi[3]; };

// std::min(a, b) / std::max(a, b) as Wide8Builder.cpp's Box uses them: the first argument stays unless the second is strictly beyond it (the sign of a zero).
RHD float refit_min(float a, float b) { return b < a ? b : a; }
RHD float refit_max(float a, float b) { return a < b ? b : a; }
RHD void refit_box_reset(RefitBox& b) { for (int a = 0; a < 3; ++a) { b.lo[a] = FLT_MAX; b.hi[a] = -FLT_MAX; } }
RHD void refit_box_grow(RefitBox& b, const float* p) { for (int a = 0; a < 3; ++a) { b.lo[a] = refit_min(b.lo[a], p[a]); b.hi[a] = refit_max(b.hi[a], p[a]); } }
RHD void refit_box_grow(RefitBox& b, const RefitBox& o) { for (int a = 0; a < 3; ++a) { b.lo[a] = refit_min(b.lo[a], o.lo[a]); b.hi[a] = refit_max(b.hi[a], o.hi[a]); } }
RHD float refit_half_area(const RefitBox& b) {
    const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    return dx * dy + dy * dz + dz * dx;
}
RHD const float* refit_corner(const HiprTriangle& t, int k) { return k % 3 == 0 ? t.v0 : (k % 3 == 1 ? t.v1 : t.v2); }
RHD uint32_t refit_bits(float v) { union { float f; uint32_t u; } x; x.f = v; return x.u; }
RHD bool refit_same_point(const float* p, const float* q) { return refit_bits(p[0]) == refit_bits(q[0]) && refit_bits(p[1]) == refit_bits(q[1]) && refit_bits(p[2]) == refit_bits(q[2]); }
RHD RefitBox refit_triangle_box(const HiprTriangle& t) {
    RefitBox b; refit_box_reset(b);
    refit_box_grow(b, t.v0); refit_box_grow(b, t.v1); refit_box_grow(b, t.v2);
    return b;
}

// SceneBuilder.cpp:310 -- a corner of a moved instance's triangle: three products summed left to right, then the translation.
RHD void refit_world_corner(const float* M, const float* p, float* out) {
    for (int r = 0; r < 3; ++r) out[r] = M[4 * r] * p[0] + M[4 * r + 1] * p[1] + M[4 * r + 2] * p[2] + M[4 * r + 3];
}

// Wide8Builder.cpp make_record. false: B no longer shares exactly two bit-identical corners with A (`out` is then not to be used).
RHD bool refit_make_record(const HiprTriangle* triangles, uint32_t index_a, uint32_t index_b, int rotation_a, HiprLeaf8& out) {
    const HiprTriangle& A = triangles[index_a];
    const float *a = refit_corner(A, rotation_a), *b = refit_corner(A, rotation_a + 1), *c = refit_corner(A, rotation_a + 2);
    for (int k = 0; k < 3; ++k) { out.a[k] = a[k]; out.e1[k] = b[k] - a[k]; out.e2[k] = c[k] - a[k]; out.e3[k] = 0.0f; }
    out.triangle[0] = index_a;
    out.triangle[1] = HIPR_LEAF8_NONE;
    uint32_t flags = (A.flags & HIPR_TRIANGLE_OPAQUE ? 1u : 0u) | (A.flags & HIPR_TRIANGLE_ONE_SIDED ? 4u : 0u) | uint32_t((1 - rotation_a + 3) % 3) << 8 | uint32_t((2 - rotation_a + 3) % 3) << 10;
    if (index_b != HIPR_LEAF8_NONE) {
        const HiprTriangle& B = triangles[index_b];
        int where[3] = {-1, -1, -1};      // record corner (0 = a, 1 = c, 2 = d) of B's vertex j
        const float* d = nullptr;
        for (int j = 0; j < 3; ++j) {
            if (refit_same_point(refit_corner(B, j), a)) where[j] = 0;
            else if (refit_same_point(refit_corner(B, j), c)) where[j] = 1;
            else { where[j] = 2; d = refit_corner(B, j); }
        }
        if (!d || where[0] == where[1] || where[0] == where[2] || where[1] == where[2]) return false;
        for (int k = 0; k < 3; ++k) out.e3[k] = d[k] - a[k];
        out.triangle[1] = index_b;
        flags |= (B.flags & HIPR_TRIANGLE_OPAQUE ? 2u : 0u) | (B.flags & HIPR_TRIANGLE_ONE_SIDED ? 8u : 0u) | uint32_t(where[1]) << 12 | uint32_t(where[2]) << 14;
        const bool even = (where[0] == 0 && where[1] == 1) || (where[0] == 1 && where[1] == 2) || (where[0] == 2 && where[1] == 0);
        if (!even) flags |= 16u;
    }
    out.flags = flags;
    float squares = 0.0f;
    for (int k = 0; k < 3; ++k) squares += out.e1[k] * out.e1[k] + out.e2[k] * out.e2[k] + out.e3[k] * out.e3[k];
    out.facing_margin = squares * (1.0f / 8192.0f);
    return true;
}

// One leaf slot of refit_wide8: the record rebuilt from the stored triangle indices and A's stored rotation, and its exact box.
RHD bool refit_leaf(const HiprTriangle* triangles, const HiprLeaf8& stored, HiprLeaf8& rebuilt, RefitBox& exact) {
    const uint32_t index_a = stored.triangle[0], index_b = stored.triangle[1];
    const int rotation_a = int((1 - int((stored.flags >> 8) & 3u) + 3) % 3);
    exact = refit_triangle_box(triangles[index_a]);
    if (index_b != HIPR_LEAF8_NONE) refit_box_grow(exact, refit_triangle_box(triangles[index_b]));
    return refit_make_record(triangles, index_a, index_b, rotation_a, rebuilt);
}

// Wide8Builder.cpp quantise_node, in binary64 as written there, except for the seed of the exponent search (see the head of this file).
RHD void refit_quantise_node(const RefitBox* boxes, uint32_t valid, const RefitBox& all, const float* grid_min, const float* grid_cell, HiprNode8& node) {
    unsigned long long packed_origin = 0;
    for (int a = 0; a < 3; ++a) {
        double m = ::floor((double(all.lo[a]) - double(grid_min[a])) / double(grid_cell[a]));
        m = m < 0.0 ? 0.0 : m;            // std::min(std::max(m, 0.0), 2097151.0)
        m = 2097151.0 < m ? 2097151.0 : m;
        while (m > 0.0 && ::fmaf(float(m), grid_cell[a], grid_min[a]) > all.lo[a]) m -= 1.0;
        packed_origin |= (unsigned long long)(m) << (21 * a);
        const float origin_f = ::fmaf(float(m), grid_cell[a], grid_min[a]);      // what the traversal computes
        const double origin = origin_f, extent = double(all.hi[a]) - origin;
        int e = extent > 0.0 ? int(::ilogb(extent)) - 8 : -126;
        e = e < -126 ? -126 : (e > 127 ? 127 : e);
        for (;; ++e) {
            const double scale = ::ldexp(1.0, e);
            bool fits = true;
            uint8_t lo8[8] = {255, 255, 255, 255, 255, 255, 255, 255}, hi8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int s = 0; s < 8 && fits; ++s) {
                if (!(valid >> s & 1u)) { lo8[s] = 255; hi8[s] = 0; continue; }
                double lo = ::floor((double(boxes[s].lo[a]) - origin) / scale), hi = ::ceil((double(boxes[s].hi[a]) - origin) / scale);
                while (lo > 0.0 && origin + lo * scale > double(boxes[s].lo[a])) lo -= 1.0;
                while (origin + hi * scale < double(boxes[s].hi[a])) hi += 1.0;
                lo = lo < 0.0 ? 0.0 : lo;
                if (hi > 255.0) { fits = false; break; }
                lo8[s] = uint8_t(lo); hi8[s] = uint8_t(hi);
            }
            if (fits || e >= 127) {
                for (int s = 0; s < 8; ++s) { node.qlo[a][s] = lo8[s]; node.qhi[a][s] = hi8[s]; }
                break;
            }
        }
        node.exponent[a] = uint8_t(e + 127);
    }
    node.origin[0] = uint32_t(packed_origin);
    node.origin[1] = uint32_t(packed_origin >> 32);
}

// One node slot of refit_wide8: `exact` holds the boxes of all slots behind this one (children live in higher slots).
RHD void refit_node(HiprNode8& n, const RefitBox* exact, const float* grid_min, const float* grid_cell, RefitBox& all, bool quantise = true) {
    const uint32_t base = n.base_valid & 0xFFFFFFu, valid = n.base_valid >> 24;
    RefitBox boxes[8];
    refit_box_reset(all);
    uint32_t rank = 0;
    for (int s = 0; s < 8; ++s) {
        refit_box_reset(boxes[s]);
        if (!(valid >> s & 1u)) continue;
        boxes[s] = exact[base + rank++];
        refit_box_grow(all, boxes[s]);
    }
    if (quantise) refit_quantise_node(boxes, valid, all, grid_min, grid_cell, n);
}

// Wide8Builder.cpp set_grid from the scene's bounds (host only: std::nextafter).
inline void refit_grid(const float* lo, const float* hi, float* grid_min, float* grid_cell) {
    for (int a = 0; a < 3; ++a) {
        grid_min[a] = lo[a];
        const float extent = hi[a] - lo[a];
        float cell = extent > 0.0f ? extent / 2097151.0f : 1.0f;
        while (double(cell) * 2097151.0 < double(hi[a]) - double(lo[a])) cell = std::nextafter(cell, FLT_MAX);
        grid_cell[a] = cell > 0.0f ? cell : FLT_MIN;
    }
}

// SceneBuilder.cpp mirrors(): does the 3x4 matrix turn its object inside out?
inline bool refit_mirrors(const float* M) {
    const double det = double(M[0]) * (double(M[5]) * M[10] - double(M[6]) * M[9]) - double(M[1]) * (double(M[4]) * M[10] - double(M[6]) * M[8]) +
                       double(M[2]) * (double(M[4]) * M[9] - double(M[5]) * M[8]);
    return det < 0.0;
}

// A bound and the ordinal of the corner it came from. Among equal values the EARLIEST corner wins, which is what the host's sweep in storage order keeps
// (it replaces a bound only by a strictly smaller / larger value): equal values are the same bits except for the two zeros, and with this rule the sign of a
// zero bound is the host's too, whatever the shape of the reduction.
struct RefitBound { float v; uint32_t i; };
RHD RefitBound refit_lower(RefitBound a, RefitBound b) { return (b.v < a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
RHD RefitBound refit_upper(RefitBound a, RefitBound b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }

#if defined(__HIPCC__) && !defined(HIPR_REFIT_HOST_ONLY)      // the kernels; a host build of the routines (tests/native/DeviceRefitHost.hip) leaves them out

constexpr int REFIT_BLOCK = 256;

__device__ __forceinline__ RefitBound refit_shuffle(RefitBound a, int mask) { return {__shfl_xor(a.v, mask, 64), uint32_t(__shfl_xor(int(a.i), mask, 64))}; }

// Reduces the six bounds of a block's threads; thread 0 writes them to partial[6 * block ...].
__device__ __forceinline__ void refit_reduce_bounds(RefitBound (&bound)[6], RefitBound* __restrict__ partial) {
    __shared__ RefitBound across[REFIT_BLOCK / 64][6];
    for (int mask = 32; mask >= 1; mask >>= 1)
        for (int k = 0; k < 6; ++k) bound[k] = k < 3 ? refit_lower(bound[k], refit_shuffle(bound[k], mask)) : refit_upper(bound[k], refit_shuffle(bound[k], mask));
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (lane == 0) for (int k = 0; k < 6; ++k) across[wave][k] = bound[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 0; k < 6; ++k) {
            RefitBound r = across[0][k];
            for (int w = 1; w < REFIT_BLOCK / 64; ++w) r = k < 3 ? refit_lower(r, across[w][k]) : refit_upper(r, across[w][k]);
            partial[6 * size_t(blockIdx.x) + k] = r;
        }
    }
}

// Pass 1. `moved`: one word per instance. Every thread of the grid takes part in the reduction (threads past the end with neutral bounds).
__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_triangles(HiprTriangle* __restrict__ triangles, uint32_t triangle_count, const HiprInstance* __restrict__ instances,
                                                                 const uint32_t* __restrict__ moved, const uint32_t* __restrict__ indices, const HiprVertexGeometry* __restrict__ geometry,
                                                                 RefitBound* __restrict__ partial) {
    const uint32_t t = blockIdx.x * uint32_t(REFIT_BLOCK) + threadIdx.x;
    RefitBound bound[6];
    for (int k = 0; k < 6; ++k) bound[k] = {k < 3 ? FLT_MAX : -FLT_MAX, 0xFFFFFFFFu};
    if (t < triangle_count) {
        HiprTriangle tri = triangles[t];
        if (moved[tri.instance_index]) {
            const HiprInstance& inst = instances[tri.instance_index];
            const uint32_t* idx = indices + 3 * size_t(inst.index_offset + tri.primitive_index);
            float* corners[3] = {tri.v0, tri.v1, tri.v2};
            for (int k = 0; k < 3; ++k) refit_world_corner(inst.object_to_world, geometry[inst.vertex_offset + idx[k]].position, corners[k]);
            for (int r = 0; r < 3; ++r) { triangles[t].v0[r] = tri.v0[r]; triangles[t].v1[r] = tri.v1[r]; triangles[t].v2[r] = tri.v2[r]; }
        }
        const float* corners[3] = {tri.v0, tri.v1, tri.v2};
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) {
                const RefitBound p = {corners[k][a], 3u * t + uint32_t(k)};
                bound[a] = refit_lower(bound[a], p);
                bound[3 + a] = refit_upper(bound[3 + a], p);
            }
    }
    refit_reduce_bounds(bound, partial);
}

// One block folds the partials of pass 1 into out[0..6) = lo xyz, hi xyz.
__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_bounds_final(const RefitBound* __restrict__ partial, uint32_t partial_blocks, RefitBound* __restrict__ out) {
    RefitBound bound[6];
    for (int k = 0; k < 6; ++k) bound[k] = {k < 3 ? FLT_MAX : -FLT_MAX, 0xFFFFFFFFu};
    for (uint32_t b = threadIdx.x; b < partial_blocks; b += uint32_t(REFIT_BLOCK))
        for (int k = 0; k < 6; ++k) bound[k] = k < 3 ? refit_lower(bound[k], partial[6 * size_t(b) + k]) : refit_upper(bound[k], partial[6 * size_t(b) + k]);
    refit_reduce_bounds(bound, out);      // a grid of one block: written to out[0..6)
}

// Pass 2. WRITE = false: only the exact boxes (at upload, for the area the scene starts with).
template <bool WRITE>
__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_leaves(HiprSlot8* __restrict__ slots, const uint32_t* __restrict__ leaf_slots, uint32_t leaf_count, const HiprTriangle* __restrict__ triangles,
                                                              RefitBox* __restrict__ exact, uint32_t* __restrict__ rebuild_flag) {
    const uint32_t i = blockIdx.x * uint32_t(REFIT_BLOCK) + threadIdx.x;
    if (i >= leaf_count) return;
    const uint32_t slot = leaf_slots[i];
    const HiprLeaf8 stored = slots[slot].leaf;
    HiprLeaf8 rebuilt;
    RefitBox box;
    const bool ok = refit_leaf(triangles, stored, rebuilt, box);
    exact[slot] = box;
    if (!WRITE) return;
    if (ok) slots[slot].leaf = rebuilt;
    else *rebuild_flag = 1u;      // every thread that gets here stores the same word
}

// Pass 3, one launch per level: node_slots[0 .. node_count) are the nodes of ONE level, whose children (deeper levels, or leaves) have their exact boxes.
template <bool WRITE>
__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_nodes(HiprSlot8* __restrict__ slots, const uint32_t* __restrict__ node_slots, uint32_t node_count, RefitBox* __restrict__ exact,
                                                             float gx, float gy, float gz, float cx, float cy, float cz) {
    const uint32_t i = blockIdx.x * uint32_t(REFIT_BLOCK) + threadIdx.x;
    if (i >= node_count) return;
    const uint32_t slot = node_slots[i];
    HiprNode8 n = slots[slot].node;
    const float grid_min[3] = {gx, gy, gz}, grid_cell[3] = {cx, cy, cz};
    RefitBox all;
    refit_node(n, exact, grid_min, grid_cell, all, WRITE);
    exact[slot] = all;
    if (WRITE) slots[slot].node = n;
}

// Pass 4: the half areas of slots [1, slot_count) -- every slot but the root is the child box of exactly one node -- summed per block in a fixed shape.
__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_area(const RefitBox* __restrict__ exact, uint32_t slot_count, double* __restrict__ partial) {
    __shared__ double sums[REFIT_BLOCK];
    const uint32_t i = blockIdx.x * uint32_t(REFIT_BLOCK) + threadIdx.x;
    sums[threadIdx.x] = (i >= 1u && i < slot_count) ? double(refit_half_area(exact[i])) : 0.0;
    __syncthreads();
    for (uint32_t step = REFIT_BLOCK / 2; step >= 1u; step >>= 1) {
        if (threadIdx.x < step) sums[threadIdx.x] += sums[threadIdx.x + step];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = sums[0];
}
// One block: thread j adds the partials j, j + 256, ... in order, then the same tree.
__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_area_final(const double* __restrict__ partial, uint32_t partial_count, double* __restrict__ out) {
    __shared__ double sums[REFIT_BLOCK];
    double s = 0.0;
    for (uint32_t b = threadIdx.x; b < partial_count; b += uint32_t(REFIT_BLOCK)) s += partial[b];
    sums[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t step = REFIT_BLOCK / 2; step >= 1u; step >>= 1) {
        if (threadIdx.x < step) sums[threadIdx.x] += sums[threadIdx.x + step];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sums[0];
}

#endif // the kernels

} // namespace hipr
