// wide4_build.h -- the collapse of the BVH2 into the compressed 4-wide tree (host/BvhBuilder.cpp WideCollapse) on the device (hipr_build_wide4; the reference asks
// OptiX for a "Trbvh" build, which runs on the GPU, OR/Renderer.cpp:161-182,471-476).
//
// The yardstick is BYTE EQUALITY with the host's collapse: the same HiprWideNode array, node count and stack entries. The host's result depends only on its input --
// its threaded path (WideCollapse::run, layout) is written to produce the pre-order of the sequential recursion -- so a level-synchronous restatement can equal it.
// The routines below restate WideCollapse::collapse, child_of, compute_binary_need and quantise_children operation for operation -- the two libraries do not link
// each other -- as __host__ __device__ functions on top of wide8_refit.h's box routines, so that tests/native/Wide4CollapseHost.hip can compile them for the host
// and the CPU suite can hold them to the host's collapse without a GPU.
//
// Why the two agree. Which child a node adopts is decided by f32 half areas, dx * dy + dy * dz + dz * dx with one rounding per operation (both units are built with
// -ffp-contract=off, and gfx950 keeps f32 denormals in this unit as x86 does), compared with a strict > scanning the children upwards, so the first of equals wins
// on both sides; whether it adopts is integer arithmetic on binary_need and the budget. A node's position is its pre-order rank: the host's recursion appends a node
// before it descends into its children in k = 0 .. 3, so position(child k) = position(node) + 1 + the sizes of the subtrees below the inner children before k --
// pass 4 computes the sizes bottom-up, pass 5 the positions top-down, and neither depends on the order in which a level's frontier was filled. Box corners are
// copies; the union's low corner is taken with the first-of-equals min the host's Box::grow uses (the sign of a zero origin).
//
// The quantisation is quantise_children's binary64 floor / ceil / ldexp with its outward-rounding steps, every operation correctly rounded on gfx950 and on x86.
// The one place where the host's code is not a specification is the seed of its exponent search, ceil(std::log2(extent / 255)): the last bit of log2 is the C
// library's business. w4_quantise starts from k - 8 instead, k = ilogb(extent), and takes the first exponent that fits -- refit_quantise_node's search, and the
// argument at the head of wide8_refit.h carries over word for word, because the seed formula and the 255 are the same and the origin is again an f32 value (here the
// union's low corner itself, which only makes `extent` the exact difference of two f32 values rounded once): (1) no exponent <= k - 8 fits, since 255 * 2^(k - 8)
// falls short of extent >= 2^k by 2^(k - 8); (2) the host's seed is k - 7 or k - 6; (3) where it is k - 6, k - 7 does not fit. Both searches therefore return the
// first fitting exponent from k - 7 on, and both clamp at -126 from below (a seed below the floor starts at the floor on both sides, and nothing below the host's
// seed fits). The host's loops have no bound; these have one written into each, which finite boxes cannot reach:
//   * the exponent search takes at most three steps -- at e = k - 6 every bound is at most ceil(2^(k + 1) / 2^(k - 6)) = 128 -- and is given W4_EXPONENT_STEPS = 8;
//   * an outward-rounding loop takes at most one step: lo / hi is the floor / ceil of a quotient whose numerator was rounded once (relative error 2^-53) and whose
//     value is below 2^10 from e = k - 8 on, so it is off by less than one -- and is given W4_ROUNDING_STEPS = 4.
// A box that is not finite would reach them, and on the host would keep quantise_children running for ever: pass 2, which reads every child box anyway, raises a
// flag the host reads with the root's need, and the collapse is refused before a wide node is made.
//
// Passes (all on the context's stream; one launch per level, no block waits on another, nothing spins, the only atomics are integer adds):
//   host  w8_check_input    wide8_build.h's depth-first walk over the child indices before the device is touched: indices and leaf ranges in bounds, every node reached
//                           once, at most W8_MAX_LEVELS levels. Yields the level lists. (Its leaf-order condition is the 8-wide collapse's alone and is not asked.)
//   2  k_w4_need            one launch per BVH2 level, deepest first: binary_need, and the finite check of both child boxes. The host reads need[0] and the flag
//                           and chooses the root's budget as build_bvh does: 32 where need[0] <= 32, else 0xFFFF.
//   3  k_w4_collapse        one launch per wide level, top down, one thread per frontier entry (BVH2 node, budget): the adoption loop, the quantised node with its
//                           children numbered in frontier order, the inner children appended to the next level (one integer atomic add per node). The host reads the
//                           level's size.
//   4  k_w4_size            bottom-up: subtree sizes and stack_need = max over the children of (children - 1 + below). The host reads the root's.
//   5  k_w4_place_emit      top-down: a node's position is known when its level runs (its parent set it); it sets its inner children's and writes itself to its
//                           position with the child indices remapped. Unused child slots hold HIPR_WIDE_EMPTY; _pad and the unused bytes of qlo / qhi are zero.
//
// Compiled for gfx950 (hipcc -O3 with the product unit's flags, -Rpass-analysis=kernel-resource-usage), VGPRs / scratch bytes per lane, 8 waves per SIMD each:
// k_w4_need 11 / 0, k_w4_collapse 40 / 112 (box[4] and ref[4], which the adoption indexes by run-time values), k_w4_size 14 / 0, k_w4_place_emit 26 / 0 plus 12 KiB
// of LDS the compiler moves the node under remapping into. None of them is bound by registers; each runs once per level over data it streams.
#pragma once

#include "wide8_build.h"

namespace hipr {

constexpr uint32_t W4_MAX_WIDE_LEVELS = W8_MAX_LEVELS + 2;      // a wide level descends at least one BVH2 level
constexpr uint32_t W4_SMALL_BUDGET = 32u, W4_LARGE_BUDGET = 0xFFFFu;      // build_bvh: the 32-entry LDS stack where the BVH2 itself allows it
constexpr int W4_EXPONENT_STEPS = 8, W4_ROUNDING_STEPS = 4;
// W4State::status, in words: a child box that is not finite, a wide node past the capacity, then the size of every wide level.
constexpr uint32_t W4_STATUS_NOT_FINITE = 0, W4_STATUS_OVERFLOW = 1, W4_STATUS_LEVELS = 2, W4_STATUS_WORDS = W4_STATUS_LEVELS + W4_MAX_WIDE_LEVELS + 2;

struct W4State {
    const HiprBvhNode* nodes; uint32_t node_count;
    const uint32_t* level_nodes;       // the reachable BVH2 nodes, level by level (w8_check_input)
    uint32_t* need;                    // per BVH2 node: binary_need
    uint32_t wide_capacity;
    uint32_t *wide_root, *wide_budget;      // per wide node, in frontier order: the BVH2 node it is rooted at, the stack entries its subtree may need
    HiprWideNode* made;                // per wide node, in frontier order, children >= 0 numbered likewise
    uint32_t *wide_size, *wide_stack, *wide_at;      // per wide node: nodes in its subtree, its stack_need, its position in the output
    HiprWideNode* out;
    uint32_t* status;
};

RHD uint32_t w4_need_of(const W4State& S, int32_t ref) { return ref >= 0 ? S.need[ref] : 0u; }

// compute_binary_need of one node whose children are done, and the finite check of its child boxes.
RHD void w4_need(const W4State& S, uint32_t i) {
    const HiprBvhNode& n = S.nodes[i];
    uint32_t deepest = 0;
    for (int c = 0; c < 2; ++c) {
        const uint32_t below = 1u + w4_need_of(S, n.child[c]);
        deepest = deepest < below ? below : deepest;
        const RefitBox box = w8_child_box(n, c);
        for (int a = 0; a < 3; ++a) if (!w8_finite(box.lo[a]) || !w8_finite(box.hi[a])) S.status[W4_STATUS_NOT_FINITE] = 1u;      // every thread that gets here stores the same word
    }
    S.need[i] = deepest;
}

// quantise_children: origin = the low corner of the union, one power-of-two grid per axis, 8 bit bounds rounded outwards. `w` arrives zeroed.
RHD void w4_quantise(const RefitBox* boxes, uint32_t count, HiprWideNode& w) {
    RefitBox all; refit_box_reset(all);
    for (uint32_t k = 0; k < count; ++k) refit_box_grow(all, boxes[k]);
    w.exponents = 0;
    for (int a = 0; a < 3; ++a) {
        w.origin[a] = all.lo[a];
        const double origin = all.lo[a], extent = double(all.hi[a]) - origin;
        int e = extent > 0.0 ? int(::ilogb(extent)) - 8 : -126;
        e = e < -126 ? -126 : e;
        uint32_t qlo = 0, qhi = 0;
        for (int step = 0; step < W4_EXPONENT_STEPS; ++step) {      // grow the grid until every bound fits in [0, 255] after rounding outwards
            const double scale = ::ldexp(1.0, e);
            bool fits = true;
            qlo = 0; qhi = 0;
            for (uint32_t k = 0; k < count && fits; ++k) {
                const double box_lo = boxes[k].lo[a], box_hi = boxes[k].hi[a];
                double lo = ::floor((box_lo - origin) / scale), hi = ::ceil((box_hi - origin) / scale);
                for (int r = 0; r < W4_ROUNDING_STEPS && lo > 0.0 && origin + lo * scale > box_lo; ++r) lo -= 1.0;
                for (int r = 0; r < W4_ROUNDING_STEPS && origin + hi * scale < box_hi; ++r) hi += 1.0;
                lo = lo < 0.0 ? 0.0 : lo;      // std::max(lo, 0.0)
                if (hi > 255.0) { fits = false; break; }
                qlo |= uint32_t(lo) << (8 * k);
                qhi |= uint32_t(hi) << (8 * k);
            }
            if (fits) break;
            ++e;
        }
        w.qlo[a] = qlo; w.qhi[a] = qhi;
        w.exponents |= uint32_t(e + 127) << (8 * a);
    }
}

// WideCollapse::collapse of the frontier entry w of wide level `level` without the recursion: the node in S.made[w], its inner children appended from `next_base`
// on. Returns whether the adoption loop ended because one more child would not fit the budget (the tests' counter; the kernel drops it).
RHD bool w4_collapse(const W4State& S, uint32_t w, uint32_t level, uint32_t next_base) {
    const uint32_t budget = S.wide_budget[w];
    const HiprBvhNode& root = S.nodes[S.wide_root[w]];
    RefitBox box[4];
    int32_t ref[4];
    uint32_t count = 2;
    for (int c = 0; c < 2; ++c) { box[c] = w8_child_box(root, c); ref[c] = root.child[c]; }
    if (ref[0] == ref[1] && ref[0] < 0) count = 1;      // the single-leaf root references its leaf twice
    bool did_not_fit = false;
    for (int round = 0; round < 2 && count < 4; ++round) {      // an adoption adds one child
        int widest = -1;
        float widest_area = -1.0f;
        for (uint32_t i = 0; i < count; ++i) {
            if (ref[i] < 0) continue;
            const float area = refit_half_area(box[i]);
            if (area > widest_area) { widest = int(i); widest_area = area; }
        }
        if (widest < 0) break;
        const HiprBvhNode& inner = S.nodes[ref[widest]];
        const uint32_t held = count;      // entries held once this node has one more child
        const uint32_t need0 = w4_need_of(S, inner.child[0]), need1 = w4_need_of(S, inner.child[1]);
        bool fits = held + (need0 < need1 ? need1 : need0) <= budget;
        for (uint32_t i = 0; i < count && fits; ++i)
            if (int(i) != widest) fits = held + w4_need_of(S, ref[i]) <= budget;
        if (!fits) { did_not_fit = true; break; }
        for (uint32_t i = count; i > uint32_t(widest) + 1u; --i) { box[i] = box[i - 1]; ref[i] = ref[i - 1]; }      // the two newcomers take the adopted child's place, in order
        box[widest] = w8_child_box(inner, 0); ref[widest] = inner.child[0];
        box[widest + 1] = w8_child_box(inner, 1); ref[widest + 1] = inner.child[1];
        ++count;
    }

    HiprWideNode node;
    node.exponents = 0;
    for (int a = 0; a < 3; ++a) { node.origin[a] = 0.0f; node.qlo[a] = 0u; node.qhi[a] = 0u; }
    node._pad[0] = 0u; node._pad[1] = 0u;
    w4_quantise(box, count, node);

    const uint32_t held = count - 1u, child_budget = budget > held ? budget - held : 0u;
    uint32_t inner_children = 0;
    for (uint32_t k = 0; k < count; ++k) inner_children += ref[k] >= 0 ? 1u : 0u;
    uint32_t next = inner_children ? next_base + w8_atomic_add(S.status + W4_STATUS_LEVELS + level + 1u, inner_children) : 0u;
    for (uint32_t k = 0; k < 4; ++k) {
        int32_t entry = int32_t(HIPR_WIDE_EMPTY);
        if (k < count) {
            entry = ref[k];
            if (entry >= 0) {
                if (next < S.wide_capacity) { S.wide_root[next] = uint32_t(entry); S.wide_budget[next] = child_budget; entry = int32_t(next); }
                else { S.status[W4_STATUS_OVERFLOW] = 1u; entry = int32_t(HIPR_WIDE_EMPTY); }      // cannot happen: every wide node is rooted at a distinct BVH2 node; nothing is written past the arrays if it does
                ++next;
            }
        }
        node.child[k] = entry;
    }
    S.made[w] = node;
    return did_not_fit;
}

RHD bool w4_is_inner(int32_t entry) { return entry >= 0 && entry != int32_t(HIPR_WIDE_EMPTY); }

// The subtree size and the stack_need of wide node w, whose inner children are done.
RHD void w4_size(const W4State& S, uint32_t w) {
    const HiprWideNode& node = S.made[w];
    uint32_t children = 0;
    for (int k = 0; k < 4; ++k) children += node.child[k] != int32_t(HIPR_WIDE_EMPTY) ? 1u : 0u;
    uint32_t size = 1, stack = 0;
    for (int k = 0; k < 4; ++k) {
        const int32_t entry = node.child[k];
        if (entry == int32_t(HIPR_WIDE_EMPTY)) continue;
        uint32_t below = 0;
        if (entry >= 0) { below = S.wide_stack[entry]; size += S.wide_size[entry]; }
        const uint32_t here = children - 1u + below;
        stack = stack < here ? here : stack;
    }
    S.wide_size[w] = size;
    S.wide_stack[w] = stack;
}

// The pre-order: wide_at[w] is set (the root: 0). Sets the inner children's and writes w to its position.
RHD void w4_place_emit(const W4State& S, uint32_t w) {
    HiprWideNode node = S.made[w];
    const uint32_t at = S.wide_at[w];
    uint32_t cursor = at + 1u;
    for (int k = 0; k < 4; ++k) {
        const int32_t entry = node.child[k];
        if (!w4_is_inner(entry)) continue;
        S.wide_at[entry] = cursor;
        node.child[k] = int32_t(cursor);
        cursor += S.wide_size[entry];
    }
    S.out[at] = node;
}

#if defined(__HIPCC__) && !defined(HIPR_COLLAPSE_HOST_ONLY)      // the kernels; a host build of the routines (tests/native/Wide4CollapseHost.hip) leaves them out

__global__ __launch_bounds__(W8_BLOCK) void k_w4_need(W4State S, uint32_t first, uint32_t count) {
    const uint32_t k = blockIdx.x * uint32_t(W8_BLOCK) + threadIdx.x;
    if (k < count) w4_need(S, S.level_nodes[first + k]);
}
__global__ __launch_bounds__(W8_BLOCK) void k_w4_collapse(W4State S, uint32_t first, uint32_t count, uint32_t level) {
    const uint32_t k = blockIdx.x * uint32_t(W8_BLOCK) + threadIdx.x;
    if (k < count) (void)w4_collapse(S, first + k, level, first + count);
}
__global__ __launch_bounds__(W8_BLOCK) void k_w4_size(W4State S, uint32_t first, uint32_t count) {
    const uint32_t k = blockIdx.x * uint32_t(W8_BLOCK) + threadIdx.x;
    if (k < count) w4_size(S, first + k);
}
__global__ __launch_bounds__(W8_BLOCK) void k_w4_place_emit(W4State S, uint32_t first, uint32_t count) {
    const uint32_t k = blockIdx.x * uint32_t(W8_BLOCK) + threadIdx.x;
    if (k < count) w4_place_emit(S, first + k);
}

#endif // the kernels

} // namespace hipr
