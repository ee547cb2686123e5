// vertex_pose.h -- skinned and morphed meshes of the resident scene posed on the device (hipr_set_scene_rigs, hipr_pose_scene_rigs): the rest data of a rig -- rest
// positions and normals, joint indices and weights, morph-target deltas -- stay in device memory beside the pools; a pose is a few dozen 3x4 matrices and a handful
// of target weights, and ONE launch of k_pose_vertices writes the posed HiprVertexGeometry rows into the geometry pool and marks them. What follows the pool
// writes is the vertex update's continuation (vertex_update.h pass 2 on: ResidentScene::queue_refit_of_marked, finish_vertex_writes).
//
// ONE text of the arithmetic for the kernel, for SceneBuilder (host/SceneBuilder.cpp pose_rigs, posed_geometry) and for the CPU suite's host build
// (tests/native/VertexPoseHost.hip). The yardstick is BYTE EQUALITY between them, so: IEEE f32, every product and every sum rounded once in the written order
// (-ffp-contract=off on all three builds, no fmaf anywhere: the host library is not built with -mfma), division and square root correctly rounded (as the refit
// relies on already). NEVER include this header in the fast-math shade unit (csrc/shade.hip).
//
// A posed vertex is a pure function of (rest data, pose): it never reads the pool. The chain, per vertex, and its roundings:
//   morph   p = rest position, n = rest normal; for each target t = 0 .. target_count-1 in index order whose weight w_t is not exactly 0:
//           p.c = p.c + w_t * dp_t.c, and with target normals n.c = n.c + w_t * dn_t.c                                   2 roundings per target and component
//   skin    (joint_count > 0) for the slots k = 0..3 in slot order whose weight w_k is not exactly 0, with m = the matrix of joint j_k (row-major 3x4):
//           q_k.r = ((m[r][0]*p.x + m[r][1]*p.y) + m[r][2]*p.z) + m[r][3]                                                 6 roundings
//           p' = (..(w_0*q_0 + w_1*q_1) + ..) over the slots taken                                                         1 per slot + 1 per slot after the first
//           the normal goes the same way through the UPPER 3x3 of each matrix, no translation: g_k.r = (m[r][0]*n.x + m[r][1]*n.y) + m[r][2]*n.z. The rule is
//           the upper 3x3, NOT the inverse transpose: exact for rotations and uniform scales, which is what skeletons are made of.
//   A position component thus sees at most POSE_ROUNDINGS(target_count) = 2 * target_count + 4 * 7 + 3 roundings (the count the CPU suite's bound repeats).
//   normal  d = (n.x*n.x + n.y*n.y) + n.z*n.z; n' = n / sqrt(d); encoded by pose_encode_octahedral, a restatement of OctahedralNormal::encode_precise with its
//           decode (host/Math.h). When d is not finite or not > 0 (a zero matrix collapsed a limb) the vertex takes the encoding of the REST normal normalised the
//           same way (hipr_set_scene_rigs has checked that its d is finite and > 0). A rig bound without rest normals (a mesh without HIPR_MESH_NORMALS) gives
//           oct_normal = {0, 0}, as SceneBuilder::vertex_geometry(position, nullptr).
// No posed position can overflow: |rest|, |delta|, |matrix entry| <= 2^30 and |target weight| <= 2^10 with at most 256 targets give |p| <= 2^30 + 256 * 2^10 * 2^30
// < 2^49 after the morph, |q| <= 3 * 2^30 * 2^49 + 2^30 < 2^81, and four slots of weight <= 1 stay under 2^83 << 2^128. The kernel never has to refuse.
//
// The resident layout, chosen for the kernel's loads (a thread per vertex, neighbouring lanes neighbouring vertices):
//   rest rows      32 bytes per vertex: position, normal, the four joint indices as two words (j0 | j1 << 16, j2 | j3 << 16) -- two 16-byte loads per lane, a wave
//                  reads 2 KB contiguous;
//   weight rows    16 bytes per vertex (rigs with joints only): one 16-byte load per lane;
//   targets        target-major float3 deltas as the caller gives them: per target a wave reads 768 contiguous bytes, every byte of every line used.
// Each section begins on a 16-byte boundary of ONE buffer for all rigs (rig_data); a PoseRig record per rig names the sections.
// The per-call staging copy carries the block table (a block of 256 threads belongs to exactly one pose), a PoseCall per pose and all matrices and target weights.
//
// Joint matrices: neighbouring vertices share joints. A block whose rig has at most POSE_LDS_JOINTS joints copies the matrices to LDS (rows of POSE_LDS_STRIDE
// words) and reads them there; a rig with more joints gathers them from the staging copy in global memory (the L2 serves the repeats). Both paths run the same
// statements on the same values and give the same bytes. The budget a context applies can be set for a measurement, up to POSE_LDS_CAPACITY
// (hipr_debug_set_pose_lds_joints). Measured (tools/vertex_pose_probe.py, profiles/vertex_pose_device_vs_host.txt; the pose kernel with its memsets between events,
// 2 684 and 100 471 vertices): 32 joints -- LDS 0.0199 / 0.0204 ms, gathered 0.0196 / 0.0201 ms, no difference beyond the spread; 300 joints -- LDS 0.0266 / 0.0258 ms,
// gathered 0.0191 / 0.0206 ms: every block of 256 vertices copies 14 KB to read a few rows of it, and loses. These spans are a launch floor of about 0.02 ms (two
// memsets and a launch-bound kernel): they cannot show a gain of either path, only the cost of staging where it exceeds the floor. Said plainly: the LDS path has NO
// measured benefit at any size. The gather never lost; it is the faster path wherever the two differ. LDS staging is kept because the kernel is asked to have both
// paths, and its budget of 32 joints is the largest measured size at which it costs nothing; larger rigs gather. The rows' stride in LDS is the plain 12 words; a
// padded stride was NOT measured, and with no gain to protect there is nothing a conflict-free layout could be shown to win here.
// Compiler figures of k_pose_vertices (gfx950, -O3): see the note above the kernel.
#pragma once

#include "../../include/hiprenderer_c.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define VPHD __host__ __device__ inline
#else
#define VPHD inline
#endif

namespace hipr {

constexpr uint32_t POSE_BLOCK = 256;
constexpr uint32_t POSE_LDS_CAPACITY = 320;    // the joints the kernel's LDS array holds: 320 x 48 bytes = 15 KB, which leaves a CU its 32 waves
constexpr uint32_t POSE_LDS_JOINTS = 32;       // the LDS budget in joints that ships, from the measurement above
constexpr uint32_t POSE_LDS_STRIDE = 12;       // words between two matrices in LDS: 16-byte aligned rows, read as three 16-byte words
constexpr uint32_t POSE_MAX_TARGETS = 256;
constexpr uint32_t POSE_RIG_NORMALS = 1u, POSE_RIG_TARGET_NORMALS = 2u;
constexpr float POSE_MAX_MAGNITUDE = 1073741824.0f;      // 2^30: rest positions, deltas, matrix entries
constexpr float POSE_MAX_TARGET_WEIGHT = 1024.0f;        // 2^10
VPHD uint32_t pose_roundings(uint32_t target_count) { return 2u * target_count + 4u * 7u + 3u; }

// A resident rig: its range of the geometry pool and where its sections begin in rig_data, in 4-byte words.
struct PoseRig {
    uint32_t first_vertex, vertex_count, joint_count, target_count, flags, pad;
    uint64_t rest, weights, target_positions, target_normals;
    uint64_t pad2;
};
static_assert(sizeof(PoseRig) == 64, "a rig record is 64 bytes");
// A block of the launch: the pose of the call it belongs to and the first vertex of the rig it poses.
struct PoseBlock { uint32_t call, first; };
// A pose of the call: its rig and where its matrices and target weights lie in the staging copy's floats, in words.
struct PoseCall { uint32_t rig, matrices, target_weights, pad; };

// The sections of a rig as pointers (device or host).
struct PoseRigView {
    uint32_t first_vertex, vertex_count, joint_count, target_count, flags;
    const uint32_t* rest;      // 8 words per vertex
    const float* weights;      // 4 per vertex
    const float* target_positions;
    const float* target_normals;
};
VPHD PoseRigView view_of(const PoseRig& r, const uint32_t* rig_data) {
    return {r.first_vertex, r.vertex_count, r.joint_count, r.target_count, r.flags, rig_data + r.rest, reinterpret_cast<const float*>(rig_data + r.weights),
            reinterpret_cast<const float*>(rig_data + r.target_positions), reinterpret_cast<const float*>(rig_data + r.target_normals)};
}

VPHD float pose_word_as_float(uint32_t w) { float f; memcpy(&f, &w, 4); return f; }

// OctahedralNormal::decode (host/Math.h:251-258) for the code (x, y). fmax(-z, 0) is written as a comparison: the two differ in the sign of a zero, which the sums
// below cannot tell (float(short) is never -0).
VPHD void pose_decode_octahedral(int x, int y, float out[3]) {
    const float fx = float(x), fy = float(y);
    float nx = fx, ny = fy;
    const float nz = (32767.0f - fabsf(fx)) - fabsf(fy);
    const float t = nz < 0.0f ? -nz : 0.0f;
    nx = nx + (nx >= 0.0f ? -t : t);
    ny = ny + (ny >= 0.0f ? -t : t);
    const float m = sqrtf((nx * nx + ny * ny) + nz * nz);
    out[0] = nx / m; out[1] = ny / m; out[2] = nz / m;
}
VPHD float pose_code_distance(int x, int y, const float n[3]) {
    float d[3];
    pose_decode_octahedral(x, y, d);
    const float a = d[0] - n[0], b = d[1] - n[1], c = d[2] - n[2];
    return (a * a + b * b) + c * c;
}
// OctahedralNormal::encode_precise (host/Math.h:260-279): the floored code and its three neighbours, the first of the nearest kept. short(int) wraps as there.
VPHD void pose_encode_octahedral(const float n[3], int16_t out[2]) {
    const float denom = (fabsf(n[0]) + fabsf(n[1])) + fabsf(n[2]);
    const float px = n[0] / denom, py = n[1] / denom;
    float p2x = px, p2y = py;
    if (n[2] < 0.0f) {
        p2x = (1.0f - fabsf(py)) * (px >= 0.0f ? 1.0f : -1.0f);
        p2y = (1.0f - fabsf(px)) * (py >= 0.0f ? 1.0f : -1.0f);
    }
    p2x = p2x < -1.0f ? -1.0f : (p2x > 1.0f ? 1.0f : p2x);
    p2y = p2y < -1.0f ? -1.0f : (p2y > 1.0f ? 1.0f : p2y);
    const int16_t fx = int16_t(floorf(p2x * 32767.0f)), fy = int16_t(floorf(p2y * 32767.0f));
    int16_t bx = fx, by = fy;
    float lowest = pose_code_distance(fx, fy, n);
    const int dx[3] = {0, 1, 1}, dy[3] = {1, 0, 1};
    for (int k = 0; k < 3; ++k) {
        const int16_t cx = int16_t(int(fx) + dx[k]), cy = int16_t(int(fy) + dy[k]);
        const float m = pose_code_distance(cx, cy, n);
        if (m < lowest) { bx = cx; by = cy; lowest = m; }
    }
    out[0] = bx; out[1] = by;
}

// n / sqrt(n.n) into out; false when n.n is not finite or not > 0.
VPHD bool pose_normalise(const float n[3], float out[3]) {
    const float d = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    if (!(d > 0.0f) || !(d <= 3.402823466e+38f)) return false;
    const float len = sqrtf(d);
    out[0] = n[0] / len; out[1] = n[1] / len; out[2] = n[2] / len;
    return true;
}

// The chain above for vertex v of `rig`: matrix j at matrices + j * stride (12 floats, row-major 3x4), the pose's target weights.
VPHD HiprVertexGeometry pose_vertex(const PoseRigView& rig, uint32_t v, const float* matrices, uint32_t stride, const float* target_weights) {
    const uint32_t* row = rig.rest + 8u * size_t(v);
    float p[3] = {pose_word_as_float(row[0]), pose_word_as_float(row[1]), pose_word_as_float(row[2])};
    const float rest_normal[3] = {pose_word_as_float(row[3]), pose_word_as_float(row[4]), pose_word_as_float(row[5])};
    float n[3] = {rest_normal[0], rest_normal[1], rest_normal[2]};
    const bool normals = (rig.flags & POSE_RIG_NORMALS) != 0, target_normals = normals && (rig.flags & POSE_RIG_TARGET_NORMALS) != 0;
    for (uint32_t t = 0; t < rig.target_count; ++t) {
        const float w = target_weights[t];
        if (w == 0.0f) continue;
        const size_t at = 3u * (size_t(t) * rig.vertex_count + v);
        for (int c = 0; c < 3; ++c) p[c] = p[c] + w * rig.target_positions[at + c];
        if (target_normals)
            for (int c = 0; c < 3; ++c) n[c] = n[c] + w * rig.target_normals[at + c];
    }
    if (rig.joint_count) {
        const float* weights = rig.weights + 4u * size_t(v);
        const uint32_t joints[4] = {row[6] & 0xFFFFu, row[6] >> 16, row[7] & 0xFFFFu, row[7] >> 16};
        float sp[3] = {0.0f, 0.0f, 0.0f}, sn[3] = {0.0f, 0.0f, 0.0f};
        bool first = true;
        for (int k = 0; k < 4; ++k) {
            const float w = weights[k];
            if (w == 0.0f) continue;
            const float* m = matrices + size_t(joints[k]) * stride;
            for (int r = 0; r < 3; ++r) {
                const float q = ((m[4 * r] * p[0] + m[4 * r + 1] * p[1]) + m[4 * r + 2] * p[2]) + m[4 * r + 3];
                const float g = (m[4 * r] * n[0] + m[4 * r + 1] * n[1]) + m[4 * r + 2] * n[2];
                sp[r] = first ? w * q : sp[r] + w * q;
                sn[r] = first ? w * g : sn[r] + w * g;
            }
            first = false;
        }
        for (int c = 0; c < 3; ++c) { p[c] = sp[c]; n[c] = sn[c]; }
    }
    HiprVertexGeometry out;
    out.position[0] = p[0]; out.position[1] = p[1]; out.position[2] = p[2];
    out.oct_normal[0] = 0; out.oct_normal[1] = 0;
    if (normals) {
        float unit[3];
        if (!pose_normalise(n, unit)) (void)pose_normalise(rest_normal, unit);      // the rest normal's d is finite and > 0: checked when the rig was bound
        pose_encode_octahedral(unit, out.oct_normal);
    }
    return out;
}

// ---- the host's side: the checks (ONE text for hipr_set_scene_rigs / hipr_pose_scene_rigs and SceneBuilder), the packing, the plan of a call ----

// What the host keeps of a bound rig: poses are checked against it.
struct RigBook { uint32_t first_vertex, vertex_count, joint_count, target_count, flags; };

inline bool pose_magnitude_ok(float v) { return std::fabs(v) <= POSE_MAX_MAGNITUDE; }      // false for a NaN and an infinity as well

// Every refusal of a rig list over a pool of `pool_vertices` vertices; null when it is sound, otherwise what is wrong.
inline const char* check_rig_descs(const HiprRigDesc* rigs, uint32_t count, uint64_t pool_vertices) {
    if (count && !rigs) return "null array with a non-zero count";
    std::vector<std::pair<uint64_t, uint64_t>> ranges;
    for (uint32_t k = 0; k < count; ++k) {
        const HiprRigDesc& d = rigs[k];
        if (d.vertex_count == 0) return "a rig has no vertices";
        if (uint64_t(d.first_vertex) + d.vertex_count > pool_vertices) return "a rig's range reaches past the resident pool";
        if (d.joint_count == 0 && d.target_count == 0) return "a rig has neither joints nor targets";
        if (d.joint_count > 65536u) return "a rig has more joints than a 16-bit index names";
        if (d.target_count > POSE_MAX_TARGETS) return "a rig has more than 256 targets";
        if (!d.rest_positions || (d.joint_count && (!d.joints || !d.weights)) || (d.target_count && !d.target_positions)) return "a null array where a count asks for data";
        ranges.push_back({d.first_vertex, uint64_t(d.first_vertex) + d.vertex_count});
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t k = 1; k < ranges.size(); ++k)
        if (ranges[k].first < ranges[k - 1].second) return "two rigs' ranges overlap";
    for (uint32_t k = 0; k < count; ++k) {
        const HiprRigDesc& d = rigs[k];
        for (size_t i = 0; i < 3u * size_t(d.vertex_count); ++i)
            if (!pose_magnitude_ok(d.rest_positions[i])) return "a rest position is not finite or above 2^30 in magnitude";
        if (d.rest_normals)
            for (uint32_t v = 0; v < d.vertex_count; ++v) {
                float unit[3];
                const float* n = d.rest_normals + 3u * size_t(v);
                if (!(std::isfinite(n[0]) && std::isfinite(n[1]) && std::isfinite(n[2])) || !pose_normalise(n, unit)) return "a rest normal is not finite or its squared length is not finite and > 0";
            }
        for (size_t i = 0; i < 3u * size_t(d.vertex_count) * d.target_count; ++i) {
            if (!pose_magnitude_ok(d.target_positions[i])) return "a target delta is not finite or above 2^30 in magnitude";
            if (d.target_normals && !pose_magnitude_ok(d.target_normals[i])) return "a target delta is not finite or above 2^30 in magnitude";
        }
        if (d.joint_count)
            for (uint32_t v = 0; v < d.vertex_count; ++v) {
                bool any = false;
                for (int s = 0; s < 4; ++s) {
                    const float w = d.weights[4u * size_t(v) + s];
                    if (d.joints[4u * size_t(v) + s] >= d.joint_count) return "a joint index is not below the rig's joint count";
                    if (!(w >= 0.0f && w <= 1.0f)) return "a weight is not finite or outside [0, 1]";
                    any = any || w != 0.0f;
                }
                if (!any) return "a vertex's four weights are all 0";
            }
    }
    return nullptr;
}

// Every refusal of a pose list against the bound rigs (BOOK: RigBook, or a struct with its first four members); null when it is sound.
template <typename BOOK>
inline const char* check_rig_poses(const HiprRigPose* poses, uint32_t count, const BOOK* rigs, size_t rig_count) {
    if (count && !poses) return "null array with a non-zero count";
    std::vector<bool> posed(rig_count, false);
    for (uint32_t k = 0; k < count; ++k) {
        const HiprRigPose& p = poses[k];
        if (p.rig >= rig_count) return "a pose names a rig that is not bound";
        if (posed[p.rig]) return "the same rig twice in one call";
        posed[p.rig] = true;
        const BOOK& r = rigs[p.rig];
        if ((r.joint_count && !p.joint_matrices) || (r.target_count && !p.target_weights)) return "a null array that the rig needs";
        for (size_t i = 0; i < 12u * size_t(r.joint_count); ++i)
            if (!pose_magnitude_ok(p.joint_matrices[i])) return "a matrix entry is not finite or above 2^30 in magnitude";
        for (uint32_t t = 0; t < r.target_count; ++t)
            if (!(std::fabs(p.target_weights[t]) <= POSE_MAX_TARGET_WEIGHT)) return "a target weight is not finite or above 2^10 in magnitude";
    }
    return nullptr;
}

// A checked rig appended to `words` in the resident layout; its record and its book.
inline void pack_rig(const HiprRigDesc& d, std::vector<uint32_t>& words, PoseRig& record, RigBook& book) {
    const auto section = [&](size_t count) { const size_t at = words.size(); words.resize(at + ((count + 3u) & ~size_t(3)), 0u); return at; };
    const uint32_t flags = (d.rest_normals ? POSE_RIG_NORMALS : 0u) | (d.rest_normals && d.target_count && d.target_normals ? POSE_RIG_TARGET_NORMALS : 0u);
    record = {};
    record.first_vertex = d.first_vertex; record.vertex_count = d.vertex_count; record.joint_count = d.joint_count; record.target_count = d.target_count; record.flags = flags;
    book = {d.first_vertex, d.vertex_count, d.joint_count, d.target_count, flags};
    const size_t n = d.vertex_count;
    record.rest = section(8u * n);
    for (size_t v = 0; v < n; ++v) {
        uint32_t* row = words.data() + record.rest + 8u * v;
        std::memcpy(row, d.rest_positions + 3u * v, 12);
        if (d.rest_normals) std::memcpy(row + 3, d.rest_normals + 3u * v, 12);
        if (d.joint_count) {
            const uint16_t* j = d.joints + 4u * v;
            row[6] = uint32_t(j[0]) | uint32_t(j[1]) << 16; row[7] = uint32_t(j[2]) | uint32_t(j[3]) << 16;
        }
    }
    if (d.joint_count) {
        record.weights = section(4u * n);
        std::memcpy(words.data() + record.weights, d.weights, 16u * n);
    }
    if (d.target_count) {
        record.target_positions = section(3u * n * d.target_count);
        std::memcpy(words.data() + record.target_positions, d.target_positions, 12u * n * d.target_count);
        if (flags & POSE_RIG_TARGET_NORMALS) {
            record.target_normals = section(3u * n * d.target_count);
            std::memcpy(words.data() + record.target_normals, d.target_normals, 12u * n * d.target_count);
        }
    }
}

// The staging copy of a checked call: the block table, the calls, the floats; each part a multiple of 16 bytes.
struct PosePlan {
    std::vector<uint8_t> staging;
    uint32_t block_count = 0;
    size_t calls_at = 0, floats_at = 0;      // byte offsets into staging
    uint64_t vertices = 0;
};
template <typename BOOK>
inline void plan_rig_poses(const HiprRigPose* poses, uint32_t count, const BOOK* rigs, PosePlan& plan) {
    plan = {};
    std::vector<PoseBlock> blocks;
    std::vector<PoseCall> calls(count);
    std::vector<float> floats;
    for (uint32_t k = 0; k < count; ++k) {
        const BOOK& r = rigs[poses[k].rig];
        calls[k] = {poses[k].rig, uint32_t(floats.size()), 0u, 0u};
        floats.insert(floats.end(), poses[k].joint_matrices, poses[k].joint_matrices + (r.joint_count ? 12u * size_t(r.joint_count) : 0u));
        calls[k].target_weights = uint32_t(floats.size());
        floats.insert(floats.end(), poses[k].target_weights, poses[k].target_weights + (r.target_count ? r.target_count : 0u));
        floats.resize((floats.size() + 3u) & ~size_t(3), 0.0f);      // the next pose's matrices on a 16-byte boundary
        for (uint32_t first = 0; first < r.vertex_count; first += POSE_BLOCK) blocks.push_back({k, first});
        plan.vertices += r.vertex_count;
    }
    const auto padded = [](size_t bytes) { return (bytes + 15u) & ~size_t(15); };
    plan.block_count = uint32_t(blocks.size());
    plan.calls_at = padded(blocks.size() * sizeof(PoseBlock));
    plan.floats_at = plan.calls_at + padded(calls.size() * sizeof(PoseCall));
    plan.staging.assign(plan.floats_at + padded(floats.size() * sizeof(float)) + 16u, uint8_t(0));
    if (!blocks.empty()) std::memcpy(plan.staging.data(), blocks.data(), blocks.size() * sizeof(PoseBlock));
    if (!calls.empty()) std::memcpy(plan.staging.data() + plan.calls_at, calls.data(), calls.size() * sizeof(PoseCall));
    if (!floats.empty()) std::memcpy(plan.staging.data() + plan.floats_at, floats.data(), floats.size() * sizeof(float));
}

#if defined(__HIPCC__) && !defined(HIPR_VERTEX_POSE_HOST_ONLY)      // the kernel; a host build of the bodies leaves it out

// grid: the block table's length; a block poses vertices [first, first + 256) of its call's rig. lds_joints <= POSE_LDS_CAPACITY: the budget applied.
// Every thread of a block takes the same way to the barrier (call, rig and budget are the block's). One 16-byte store per vertex and an idempotent byte store for the
// mark; nothing outside the rig's range is written; no atomics, no block waits on another.
// Compiler figures (gfx950, -O3, -ffp-contract=off, both matrix paths and the four decodes of the encoder inlined): 47 VGPRs, 46 SGPRs, no scratch, nothing
// spilled, 15 360 bytes of LDS per block, 8 waves per SIMD.
__global__ __launch_bounds__(POSE_BLOCK) void k_pose_vertices(const PoseBlock* __restrict__ blocks, const PoseCall* __restrict__ calls, const float* __restrict__ floats,
                                                              const PoseRig* __restrict__ rigs, const uint32_t* __restrict__ rig_data, uint32_t lds_joints,
                                                              HiprVertexGeometry* __restrict__ geometry, uint8_t* __restrict__ marks) {
    __shared__ __attribute__((aligned(16))) float staged[POSE_LDS_CAPACITY * POSE_LDS_STRIDE];
    const PoseBlock block = blocks[blockIdx.x];
    const PoseCall call = calls[block.call];
    const PoseRigView rig = view_of(rigs[call.rig], rig_data);
    const float* matrices = floats + call.matrices;
    const bool in_lds = rig.joint_count && rig.joint_count <= lds_joints;
    if (in_lds) {
        for (uint32_t i = threadIdx.x; i < 12u * rig.joint_count; i += POSE_BLOCK) staged[(i / 12u) * POSE_LDS_STRIDE + i % 12u] = matrices[i];
        __syncthreads();
    }
    const uint32_t v = block.first + threadIdx.x;
    if (v >= rig.vertex_count) return;
    // two calls, so that each is compiled for its address space (LDS reads, global loads) and not for a generic pointer
    const HiprVertexGeometry g = in_lds ? pose_vertex(rig, v, staged, POSE_LDS_STRIDE, floats + call.target_weights) : pose_vertex(rig, v, matrices, 12u, floats + call.target_weights);
    uint4 row;
    memcpy(&row, &g, 16);
    reinterpret_cast<uint4*>(geometry)[size_t(rig.first_vertex) + v] = row;
    marks[size_t(rig.first_vertex) + v] = uint8_t(1);
}

#endif // the kernel

} // namespace hipr
