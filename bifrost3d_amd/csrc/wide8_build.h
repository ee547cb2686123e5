// wide8_build.h -- the collapse of the BVH2 into the 8-wide tree (host/Wide8Builder.cpp build_wide8) on the device (hipr_build_wide8; the reference asks OptiX for
// a "Trbvh" build, which runs on the GPU, OR/Renderer.cpp:161-182,471-476).
//
// The yardstick is BYTE EQUALITY with build_wide8 in its default configuration (leaf cost 0.6, depth-first layout): the same slots, height, grid and counters.
// build_wide8's result depends only on its input, not on the number of host threads, so a level-synchronous restatement can equal it. The routines below restate
// records_of_leaf, add_subtree's chains, optimise_node, collect_roots, assign_positions, prepare_node and emit_node's layout operation for operation -- the two
// libraries do not link each other -- as __host__ __device__ functions on top of the record, box and quantisation routines of wide8_refit.h, so that
// tests/native/DeviceCollapseHost.hip can compile them for the host and the CPU suite can hold them to build_wide8 without a GPU.
//
// Why the two agree. Every value that reaches a slot, or a decision that shapes the tree, is IEEE f32 / f64 arithmetic in the host's order: box corners are copies,
// min / max keep the first of two equal values as std::min / std::max do (the sign of a zero), half areas are dx * dy + dy * dz + dz * dx with one rounding per
// operation, the dynamic program adds two f32 costs and compares with <, scanning k upwards, and the position scores are sums of three f32 terms. Both units are
// built with -ffp-contract=off (CXXFLAGS for the host, HIPFLAGS for the device and the host pass of hipcc), so no product is fused into a sum on either side, and
// gfx950 keeps f32 denormals in this unit as x86 does. area * NODE_COST has NODE_COST = 1, which is exact. The quantisation is wide8_refit.h's, whose header says
// why its exponent search is the host's.
//
// The tree the collapse works on is the host's binary tree -- every BVH2 leaf turned into the chain ((r0, r1), r2) ... of its records -- under a numbering of its own,
// which never reaches the output: BVH2 inner node i is tree node i; the chain node covering records 0 .. k of a leaf whose first record is R is N + R + k (k >= 1);
// record R is the tree leaf N + Rt + R (N BVH2 nodes, Rt records). A full binary tree over Rt leaves has Rt - 1 inner nodes, which bounds the wide nodes.
//
// Passes (all on the context's stream; one launch per level, no block waits on another, nothing spins, the only atomics are integer adds):
//   host  w8_check_input    one O(n) depth-first walk over the child indices before the device is touched: indices and leaf ranges in bounds, every node reached once,
//                           at most W8_MAX_LEVELS levels, and the leaves met in ascending order of their first triangle -- the order record numbers are scanned in.
//                           A tree that fails the last is not malformed, only not what the scan assumes: it DECLINES (the host collapses it). Yields the level lists.
//   1  k_w8_bounds          the scene's bounds over the triangles in storage order (wide8_refit.h's reduction: the earliest of equal bounds wins); the host takes the
//                           grid from them with refit_grid. A corner (here) or a child box (pass 2) that is not finite is refused when the host reads these results.
//   2  k_w8_count_leaf      one thread per BVH2 child reference: a leaf's records counted (records_of_leaf without the writes) at the position of its first triangle;
//      k_w8_scan_local, k_build_scan_sums: the exclusive scan of the counts = the record numbers; the host reads the total.
//   3  k_w8_leaf            the same threads: records, their boxes, the chain with its prefix boxes and its dynamic program; inner children get their boxes.
//   4  k_w8_optimise        one launch per BVH2 level, deepest first: optimise_node.
//   5  k_w8_prepare         one launch per wide level, top down: collect_roots (iterative; the allowance is at most 8, so is the stack), assign_positions, the children
//                           by position; the inner children become the next level's wide nodes (one integer atomic add per node). The host reads the level's size.
//   6  k_w8_size            bottom-up: size_below(n) = child_count + the sum over inner children. The host reads the root's: slots needed = 1 + size_below(root).
//   7  k_w8_place           top-down: a node's children block, then the blocks below its inner children in position order, as emit_node appends them.
//   8  k_w8_emit_nodes, k_w8_emit_leaves   one thread per wide node quantises (refit_quantise_node) and writes its slot; one thread per record copies it to its slot.
//
// Compiled for gfx950 (hipcc -O3 with the product unit's flags, -Rpass-analysis=kernel-resource-usage), VGPRs / scratch bytes per lane: k_w8_bounds 33 / 0,
// k_w8_count_leaf 38 / 112 and k_w8_leaf 74 / 112 (the two triangles under test, fetched through run-time corner indices), k_w8_scan_local 13 / 0, k_w8_optimise 33 / 0
// (the tables of both children and distribute[] stay in registers: the loops unroll), k_w8_prepare 38 / 272 (the 8 x 8 score matrix, the root list and the walk's
// stack are indexed by run-time values), k_w8_size 8 / 0, k_w8_place 14 / 0, k_w8_emit_nodes 46 / 208 plus 16 KiB of LDS the compiler moves boxes[8] into (the exponent
// search indexes it by position, as in k_refit_nodes), k_w8_emit_leaves 20 / 0. None of them is bound by registers; each runs once per level over data it streams,
// and the scratch of the three that have some is a few hundred bytes touched a handful of times per thread.
#pragma once

#include "bvh2_build.h"
#include "wide8_refit.h"

#include <cstdio>
#include <vector>

namespace hipr {

constexpr float W8_NODE_COST = 1.0f, W8_LEAF_COST = 0.6f;      // Wide8Builder.cpp NODE_COST and the default LEAF_COST
constexpr uint32_t W8_MAX_LEVELS = 64;                          // BVH2 levels: what a 64-entry walk allows
constexpr uint32_t W8_MAX_WIDE_LEVELS = W8_MAX_LEVELS + 8;      // a wide level descends at least one tree level; a chain adds at most seven
constexpr uint32_t W8_MAX_SLOTS = 0xFFFFFFu;                    // HiprNode8::base_valid keeps the base in 24 bits
constexpr int32_t W8_EMPTY = 0x7FFFFFFF;
// W8State::status, in words: paired records, a wide node past the capacity, a corner or a child box that is not finite, then the size of every wide level.
constexpr uint32_t W8_STATUS_PAIRED = 0, W8_STATUS_OVERFLOW = 1, W8_STATUS_NOT_FINITE = 2, W8_STATUS_LEVELS = 3, W8_STATUS_WORDS = W8_STATUS_LEVELS + W8_MAX_WIDE_LEVELS + 2;

struct W8State {
    const HiprBvhNode* nodes; uint32_t node_count;
    const HiprTriangle* triangles; const uint32_t* order; uint32_t triangle_count;
    const uint32_t* level_nodes;       // the reachable BVH2 nodes, level by level (w8_check_input)
    uint32_t reachable, single_leaf;   // single_leaf: the root references one leaf twice; the tree is that leaf's chain
    uint32_t *counts, *block_sums;     // per triangle position: the records of the leaf that starts there, then their scan
    uint32_t record_total, leaf_base, wide_capacity;      // leaf_base = node_count + record_total: tree ids from there on are records
    RefitBox* box;                     // per tree node
    int32_t *left, *right;             // per inner tree node
    float* cost; uint8_t *split, *roots_used;      // per inner tree node, seven each
    HiprLeaf8* records; uint32_t* record_slot;
    uint32_t* wide_tree; int32_t* wide_child; RefitBox* wide_all; uint32_t *wide_size, *wide_base, *wide_slot;      // per wide node; wide_tree[0] is the tree's root: 0, or the single leaf's chain; wide_child: eight, by position
    HiprSlot8* slots;
    uint32_t* status;
    float grid_min[3], grid_cell[3];
};

RHD RefitBox w8_child_box(const HiprBvhNode& n, int c) {
    RefitBox b;
    const float* xy = c == 0 ? n.c0xy : n.c1xy;
    b.lo[0] = xy[0]; b.hi[0] = xy[1]; b.lo[1] = xy[2]; b.hi[1] = xy[3];
    b.lo[2] = n.cz[2 * c]; b.hi[2] = n.cz[2 * c + 1];
    return b;
}
RHD const HiprTriangle& w8_triangle(const W8State& S, uint32_t k) { return S.triangles[S.order ? S.order[k] : k]; }
RHD bool w8_is_leaf(const W8State& S, int32_t id) { return uint32_t(id) >= S.leaf_base; }
RHD bool w8_finite(float v) { return (refit_bits(v) & 0x7F800000u) != 0x7F800000u; }
// An infinite bound would keep quantise_node's rounding loops going for ever, on the host as on the device: passes 1 and 2, which read every corner and every child
// box anyway, raise a flag the host reads with their results, and the collapse is refused before a later pass runs.
RHD bool w8_triangle_finite(const HiprTriangle& t) {
    bool finite = true;
    for (int k = 0; k < 3; ++k) finite = finite && w8_finite(t.v0[k]) && w8_finite(t.v1[k]) && w8_finite(t.v2[k]);
    return finite;
}
RHD uint32_t w8_atomic_add(uint32_t* p, uint32_t v) { return build_atomic_add(p, v); }

// cost_of(n, i): a record's is area * LEAF_COST for every i.
RHD float w8_cost(const W8State& S, int32_t id, int i) { return w8_is_leaf(S, id) ? refit_half_area(S.box[id]) * W8_LEAF_COST : S.cost[7 * size_t(id) + size_t(i - 1)]; }

// optimise_node of an inner tree node whose box and children are in place and whose children are done.
RHD void w8_optimise(const W8State& S, int32_t n) {
    const float area = refit_half_area(S.box[n]);
    float cl[7], cr[7];
    for (int i = 1; i <= 7; ++i) { cl[i - 1] = w8_cost(S, S.left[n], i); cr[i - 1] = w8_cost(S, S.right[n], i); }
    float distribute[9];
    for (int j = 2; j <= 8; ++j) {
        float best = FLT_MAX;
        int best_k = 1;
        for (int k = 1; k < j; ++k) {
            const float c = cl[(k < 7 ? k : 7) - 1] + cr[(j - k < 7 ? j - k : 7) - 1];
            if (c < best) { best = c; best_k = k; }
        }
        distribute[j] = best;
        S.split[7 * size_t(n) + size_t(j - 2)] = uint8_t(best_k);
    }
    float* cost = S.cost + 7 * size_t(n);
    uint8_t* used = S.roots_used + 7 * size_t(n);
    float previous = area * W8_NODE_COST + distribute[8];
    uint8_t previous_used = 1;
    cost[0] = previous; used[0] = 1;
    for (int i = 2; i <= 7; ++i) {
        if (distribute[i] < previous) { previous = distribute[i]; previous_used = uint8_t(i); }
        cost[i - 1] = previous; used[i - 1] = previous_used;
    }
}

// records_of_leaf over positions [first, first + count), count <= 8, and -- `write` -- add_subtree's chain over them with its dynamic program: record R + k, its tree leaf,
// the chain node covering records 0 .. k. Returns the records; `paired` those of two triangles; `chain` the chain's root.
RHD uint32_t w8_leaf(const W8State& S, uint32_t first, uint32_t count, uint32_t R, bool write, uint32_t& paired, int32_t& chain) {
    uint32_t used = 0, made = 0;
    paired = 0; chain = -1;
    RefitBox prefix; refit_box_reset(prefix);
    for (uint32_t i = 0; i < count; ++i) {
        if (used >> i & 1u) continue;
        used |= 1u << i;
        HiprTriangle pair[2];
        pair[0] = w8_triangle(S, first + i);
        HiprLeaf8 record;
        uint32_t partner = HIPR_LEAF8_NONE;
        for (uint32_t j = i + 1; j < count && partner == HIPR_LEAF8_NONE; ++j) {
            if (used >> j & 1u) continue;
            pair[1] = w8_triangle(S, first + j);
            if (pair[1].instance_index != pair[0].instance_index) continue;
            int shared = 0, own_a = -1;
            for (int x = 0; x < 3; ++x) {
                bool found = false;
                for (int y = 0; y < 3; ++y) found = found || refit_same_point(refit_corner(pair[0], x), refit_corner(pair[1], y));
                if (found) ++shared; else own_a = x;
            }
            if (shared != 2) continue;
            if (refit_make_record(pair, 0u, 1u, (own_a + 2) % 3, record)) { used |= 1u << j; partner = j; }
        }
        if (partner != HIPR_LEAF8_NONE) ++paired;
        if (write) {
            RefitBox box = refit_triangle_box(pair[0]);
            if (partner == HIPR_LEAF8_NONE) refit_make_record(pair, 0u, HIPR_LEAF8_NONE, 0, record);
            else refit_box_grow(box, refit_triangle_box(pair[1]));
            record.triangle[0] = first + i;
            record.triangle[1] = partner == HIPR_LEAF8_NONE ? HIPR_LEAF8_NONE : first + partner;
            const int32_t leaf = int32_t(S.leaf_base + R + made);
            S.records[R + made] = record;
            S.box[leaf] = box;
            if (made == 0) { prefix = box; chain = leaf; }
            else {
                refit_box_grow(prefix, box);
                const int32_t inner = int32_t(S.node_count + R + made);
                S.box[inner] = prefix;
                S.left[inner] = chain; S.right[inner] = leaf;
                w8_optimise(S, inner);
                chain = inner;
            }
        }
        ++made;
    }
    return made;
}
// Thread t of passes 2 and 3: child t & 1 of the reachable node t >> 1. false: nothing to do there.
RHD bool w8_leaf_of_thread(const W8State& S, uint32_t t, uint32_t& node, int& c, uint32_t& first, uint32_t& count) {
    node = S.level_nodes[t >> 1]; c = int(t & 1u);
    if (S.single_leaf && c == 1) return false;
    const int32_t ref = S.nodes[node].child[c];
    if (ref >= 0) return false;
    const uint32_t code = uint32_t(~ref);
    first = code >> 3; count = (code & 7u) + 1u;
    return true;
}
RHD void w8_count_leaf(const W8State& S, uint32_t t) {
    uint32_t node, first, count, paired; int c; int32_t chain;
    const RefitBox box = w8_child_box(S.nodes[S.level_nodes[t >> 1]], int(t & 1u));
    for (int a = 0; a < 3; ++a) if (!w8_finite(box.lo[a]) || !w8_finite(box.hi[a])) S.status[W8_STATUS_NOT_FINITE] = 1u;      // every thread that gets here stores the same word
    if (w8_leaf_of_thread(S, t, node, c, first, count)) S.counts[first] = w8_leaf(S, first, count, 0u, false, paired, chain);
}
// Returns the paired records of the thread's leaf.
RHD uint32_t w8_build_leaf(const W8State& S, uint32_t t, uint32_t scan_block) {
    uint32_t node, first, count, paired = 0; int c; int32_t chain;
    if (w8_leaf_of_thread(S, t, node, c, first, count)) {
        w8_leaf(S, first, count, S.block_sums[first / scan_block] + S.counts[first], true, paired, chain);
        if (S.single_leaf) S.wide_tree[0] = uint32_t(chain);      // the tree is this chain
        else (c == 0 ? S.left : S.right)[node] = chain;
    } else if (!S.single_leaf) {
        const HiprBvhNode& n = S.nodes[node];
        const int32_t child = n.child[c];
        S.box[child] = w8_child_box(n, c);
        (c == 0 ? S.left : S.right)[node] = child;
    }
    if (t == 0 && !S.single_leaf) {
        RefitBox all = w8_child_box(S.nodes[0], 0);
        refit_box_grow(all, w8_child_box(S.nodes[0], 1));
        S.box[0] = all;
        S.wide_tree[0] = 0u;
    }
    return paired;
}

// collect_roots of both subtrees of n under the distribution of eight roots, left to right. At most eight roots; the stack holds at most the allowance.
RHD uint32_t w8_collect(const W8State& S, int32_t n, int32_t* roots) {
    if (w8_is_leaf(S, n)) { roots[0] = n; return 1; }      // a scene of a single record: the root node holds it
    int32_t stack_node[8]; int stack_allowance[8];
    const int k8 = S.split[7 * size_t(n) + 6];
    int top = 0;
    uint32_t found = 0;
    stack_node[top] = S.right[n]; stack_allowance[top++] = 8 - k8;
    stack_node[top] = S.left[n]; stack_allowance[top++] = k8;
    while (top > 0) {
        const int32_t t = stack_node[--top];
        const int allowance = stack_allowance[top];
        int used = 1;
        if (!w8_is_leaf(S, t)) used = S.roots_used[7 * size_t(t) + size_t((allowance < 7 ? allowance : 7) - 1)];
        if (used <= 1 || top + 2 > 8) { if (found < 8) roots[found++] = t; continue; }
        const int k = S.split[7 * size_t(t) + size_t(used - 2)];
        stack_node[top] = S.right[t]; stack_allowance[top++] = used - k;
        stack_node[top] = S.left[t]; stack_allowance[top++] = k;
    }
    return found;
}
// assign_positions: greedy on the signed centroid offsets, the first of equal scores in (child, position) order.
RHD void w8_assign_positions(const W8State& S, const int32_t* children, uint32_t child_count, const RefitBox& all, int* position_of) {
    float score[8][8];
    for (uint32_t c = 0; c < child_count; ++c) {
        const RefitBox& box = S.box[children[c]];
        float d[3];
        for (int a = 0; a < 3; ++a) d[a] = 0.5f * (box.lo[a] + box.hi[a]) - 0.5f * (all.lo[a] + all.hi[a]);
        for (int s = 0; s < 8; ++s) score[c][s] = ((s & 1) ? d[0] : -d[0]) + ((s & 2) ? d[1] : -d[1]) + ((s & 4) ? d[2] : -d[2]);
    }
    uint32_t child_done = 0, position_taken = 0;
    for (uint32_t round = 0; round < child_count; ++round) {
        int best_c = -1, best_s = -1;
        for (uint32_t c = 0; c < child_count; ++c) {
            if (child_done >> c & 1u) continue;
            for (int s = 0; s < 8; ++s)
                if (!(position_taken >> s & 1u) && (best_c < 0 || score[c][s] > score[best_c][best_s])) { best_c = int(c); best_s = s; }
        }
        child_done |= 1u << best_c; position_taken |= 1u << best_s;
        position_of[best_c] = best_s;
    }
}
// prepare_node without the quantisation: the children of wide node w by position; its inner children become wide nodes from `next_base` on (level `level + 1`).
RHD void w8_prepare(const W8State& S, uint32_t w, uint32_t level, uint32_t next_base) {
    const int32_t n = int32_t(S.wide_tree[w]);
    int32_t children[8];
    const uint32_t child_count = w8_collect(S, n, children);
    RefitBox all; refit_box_reset(all);
    for (uint32_t c = 0; c < child_count; ++c) refit_box_grow(all, S.box[children[c]]);
    int position_of[8];
    w8_assign_positions(S, children, child_count, all, position_of);
    int32_t child_at[8];
    for (int s = 0; s < 8; ++s) child_at[s] = W8_EMPTY;
    uint32_t inner = 0;
    for (uint32_t c = 0; c < child_count; ++c) { child_at[position_of[c]] = children[c]; inner += w8_is_leaf(S, children[c]) ? 0u : 1u; }
    uint32_t next = inner ? next_base + w8_atomic_add(S.status + W8_STATUS_LEVELS + level + 1u, inner) : 0u;
    for (int s = 0; s < 8; ++s) {
        int32_t entry = child_at[s];
        if (entry != W8_EMPTY && !w8_is_leaf(S, entry)) {
            if (next < S.wide_capacity) { S.wide_tree[next] = uint32_t(entry); entry = -int32_t(next) - 1; }
            else { S.status[W8_STATUS_OVERFLOW] = 1u; entry = W8_EMPTY; }      // cannot happen in a full binary tree; nothing is written past the arrays if it does
            ++next;
        }
        S.wide_child[8 * size_t(w) + s] = entry;
    }
    S.wide_all[w] = all;
}
RHD void w8_size(const W8State& S, uint32_t w) {
    uint32_t size = 0;
    for (int s = 0; s < 8; ++s) {
        const int32_t entry = S.wide_child[8 * size_t(w) + s];
        if (entry == W8_EMPTY) continue;
        size += 1u + (entry < 0 ? S.wide_size[uint32_t(-(entry + 1))] : 0u);
    }
    S.wide_size[w] = size;
}
// emit_node's layout: wide_slot / wide_base of w are set (the root: slot 0, base 1).
RHD void w8_place(const W8State& S, uint32_t w) {
    const uint32_t base = S.wide_base[w];
    uint32_t rank = 0, count = 0;
    for (int s = 0; s < 8; ++s) count += S.wide_child[8 * size_t(w) + s] != W8_EMPTY ? 1u : 0u;
    uint32_t cursor = base + count;
    for (int s = 0; s < 8; ++s) {
        const int32_t entry = S.wide_child[8 * size_t(w) + s];
        if (entry == W8_EMPTY) continue;
        const uint32_t slot = base + rank++;
        if (entry < 0) {
            const uint32_t child = uint32_t(-(entry + 1));
            S.wide_slot[child] = slot;
            S.wide_base[child] = cursor;
            cursor += S.wide_size[child];
        } else S.record_slot[uint32_t(entry) - S.leaf_base] = slot;
    }
}
RHD void w8_emit_node(const W8State& S, uint32_t w) {
    RefitBox boxes[8];
    uint32_t valid = 0, inner_mask = 0;
    for (int s = 0; s < 8; ++s) {
        refit_box_reset(boxes[s]);
        const int32_t entry = S.wide_child[8 * size_t(w) + s];
        if (entry == W8_EMPTY) continue;
        valid |= 1u << s;
        if (entry < 0) { inner_mask |= 1u << s; boxes[s] = S.box[S.wide_tree[uint32_t(-(entry + 1))]]; }
        else boxes[s] = S.box[entry];
    }
    HiprSlot8 slot;
    for (int k = 0; k < 16; ++k) slot.words[k] = 0u;
    slot.node.inner_mask = uint8_t(inner_mask);
    refit_quantise_node(boxes, valid, S.wide_all[w], S.grid_min, S.grid_cell, slot.node);
    slot.node.base_valid = valid << 24 | (S.wide_base[w] & 0xFFFFFFu);
    S.slots[S.wide_slot[w]] = slot;
}
RHD void w8_emit_leaf(const W8State& S, uint32_t r) { S.slots[S.record_slot[r]].leaf = S.records[r]; }

// ---- the host's part: the checks, and the level lists the launches go by ----
struct W8Input {
    std::vector<uint32_t> level_nodes, level_first;      // level l: level_nodes[level_first[l] .. level_first[l + 1])
    bool single_leaf = false;
};
enum { W8_INPUT_OK = 0, W8_INPUT_INVALID = 1, W8_INPUT_DECLINED = 2 };
// One depth-first walk, left before right, over the child indices. `message` receives the reason of a refusal.
inline int w8_check_input(const HiprBvhNode* nodes, uint32_t node_count, const uint32_t* order, uint32_t triangle_count, W8Input& in, char* message, size_t message_size) {
    if (order)
        for (uint32_t k = 0; k < triangle_count; ++k)
            if (order[k] >= triangle_count) { snprintf(message, message_size, "order[%u] = %u of %u triangles", k, order[k], triangle_count); return W8_INPUT_INVALID; }
    const HiprBvhNode& root = nodes[0];
    in.single_leaf = root.child[0] == root.child[1] && root.child[0] < 0;
    std::vector<uint8_t> depth_of(node_count, 0);      // 0: not reached yet; 0xFF: referenced, not walked yet
    struct Pending { int32_t ref; uint32_t depth; };
    std::vector<Pending> pending = {{in.single_leaf ? root.child[0] : 0, 1u}};
    uint64_t expected_first = 0;
    uint32_t levels = in.single_leaf ? 1u : 0u;
    std::vector<uint32_t> level_count(W8_MAX_LEVELS + 1, 0u);
    bool ascending = true;
    if (in.single_leaf) { depth_of[0] = 1; level_count[0] = 1; }
    else depth_of[0] = 0xFFu;
    while (!pending.empty()) {
        const Pending p = pending.back();
        pending.pop_back();
        if (p.ref < 0) {      // a leaf, met where the host's walk meets it
            const uint32_t code = uint32_t(~p.ref), first = code >> 3, count = (code & 7u) + 1u;
            if (uint64_t(first) + count > triangle_count) { snprintf(message, message_size, "a leaf on level %u holds the triangles [%u, %u) of %u", p.depth, first, first + count, triangle_count); return W8_INPUT_INVALID; }
            if (first < expected_first) ascending = false;
            expected_first = uint64_t(first) + count;
            continue;
        }
        if (p.depth > W8_MAX_LEVELS) { snprintf(message, message_size, "node %d lies on level %u, a walk of %u entries does not reach it", p.ref, p.depth, W8_MAX_LEVELS); return W8_INPUT_INVALID; }
        depth_of[p.ref] = uint8_t(p.depth);
        level_count[p.depth - 1] += 1;
        levels = std::max(levels, p.depth);
        const int32_t* child = nodes[p.ref].child;
        for (int c = 1; c >= 0; --c) {      // right first, so that the left subtree is walked first
            if (child[c] >= 0) {
                if (uint32_t(child[c]) >= node_count) { snprintf(message, message_size, "child %d of node %d is %d of %u nodes", c, p.ref, child[c], node_count); return W8_INPUT_INVALID; }
                if (depth_of[child[c]]) { snprintf(message, message_size, "node %d is referenced twice (child %d of node %d)", child[c], c, p.ref); return W8_INPUT_INVALID; }
                depth_of[child[c]] = 0xFFu;
            }
            pending.push_back({child[c], p.depth + 1u});
        }
    }
    in.level_first.assign(levels + 1, 0u);
    for (uint32_t l = 0; l < levels; ++l) in.level_first[l + 1] = in.level_first[l] + level_count[l];
    in.level_nodes.assign(in.level_first[levels], 0u);
    std::vector<uint32_t> cursor(in.level_first.begin(), in.level_first.end() - 1);
    for (uint32_t i = 0; i < node_count; ++i)
        if (depth_of[i]) in.level_nodes[cursor[depth_of[i] - 1u]++] = i;
    // The level lists are made either way: the 4-wide collapse (wide4_build.h), which counts no records, goes by them whatever the order of the leaves.
    if (!ascending) { snprintf(message, message_size, "the leaves are not met in ascending order of their first triangle; collapse on the host"); return W8_INPUT_DECLINED; }
    return W8_INPUT_OK;
}

#if defined(__HIPCC__) && !defined(HIPR_COLLAPSE_HOST_ONLY)      // the kernels; a host build of the routines (tests/native/DeviceCollapseHost.hip) leaves them out

constexpr int W8_BLOCK = 256;
static_assert(W8_BLOCK == BUILD_BLOCK && W8_BLOCK == REFIT_BLOCK, "the scan and the bounds reduction are shared");

__global__ __launch_bounds__(W8_BLOCK) void k_w8_bounds(const HiprTriangle* __restrict__ triangles, uint32_t triangle_count, RefitBound* __restrict__ partial, uint32_t* __restrict__ status) {
    const uint32_t t = blockIdx.x * uint32_t(W8_BLOCK) + threadIdx.x;
    RefitBound bound[6];
    for (int k = 0; k < 6; ++k) bound[k] = {k < 3 ? FLT_MAX : -FLT_MAX, 0xFFFFFFFFu};
    if (t < triangle_count) {
        const HiprTriangle& tri = triangles[t];
        if (!w8_triangle_finite(tri)) status[W8_STATUS_NOT_FINITE] = 1u;
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
__global__ __launch_bounds__(W8_BLOCK) void k_w8_count_leaf(W8State S) {
    const uint32_t t = blockIdx.x * uint32_t(W8_BLOCK) + threadIdx.x;
    if (t < 2u * S.reachable) w8_count_leaf(S, t);
}
// The counts of a block's positions scanned in place, the block's sum kept.
__global__ __launch_bounds__(W8_BLOCK) void k_w8_scan_local(W8State S) {
    const uint32_t i = blockIdx.x * uint32_t(W8_BLOCK) + threadIdx.x;
    const uint32_t value = i < S.triangle_count ? S.counts[i] : 0u;
    uint32_t total;
    const uint32_t before = build_block_scan(value, total);
    if (i < S.triangle_count) S.counts[i] = before;
    if (threadIdx.x == 0) S.block_sums[blockIdx.x] = total;
}
__global__ __launch_bounds__(W8_BLOCK) void k_w8_leaf(W8State S) {
    const uint32_t t = blockIdx.x * uint32_t(W8_BLOCK) + threadIdx.x;
    uint32_t paired = t < 2u * S.reachable ? w8_build_leaf(S, t, uint32_t(W8_BLOCK)) : 0u;
    for (int mask = 32; mask >= 1; mask >>= 1) paired += uint32_t(__shfl_xor(int(paired), mask, 64));
    if ((threadIdx.x & 63u) == 0u && paired) atomicAdd(S.status + W8_STATUS_PAIRED, paired);
}
__global__ __launch_bounds__(W8_BLOCK) void k_w8_optimise(W8State S, uint32_t first, uint32_t count) {
    const uint32_t k = blockIdx.x * uint32_t(W8_BLOCK) + threadIdx.x;
    if (k < count) w8_optimise(S, int32_t(S.level_nodes[first + k]));
}
__global__ __launch_bounds__(W8_BLOCK) void k_w8_prepare(W8State S, uint32_t first, uint32_t count, uint32_t level) {
    const uint32_t k = blockIdx.x * uint32_t(W8_BLOCK) + threadIdx.x;
    if (k < count) w8_prepare(S, first + k, level, first + count);
}
__global__ __launch_bounds__(W8_BLOCK) void k_w8_size(W8State S, uint32_t first, uint32_t count) {
    const uint32_t k = blockIdx.x * uint32_t(W8_BLOCK) + threadIdx.x;
    if (k < count) w8_size(S, first + k);
}
__global__ __launch_bounds__(W8_BLOCK) void k_w8_place(W8State S, uint32_t first, uint32_t count) {
    const uint32_t k = blockIdx.x * uint32_t(W8_BLOCK) + threadIdx.x;
    if (k < count) w8_place(S, first + k);
}
__global__ __launch_bounds__(W8_BLOCK) void k_w8_emit_nodes(W8State S, uint32_t count) {
    const uint32_t k = blockIdx.x * uint32_t(W8_BLOCK) + threadIdx.x;
    if (k < count) w8_emit_node(S, k);
}
__global__ __launch_bounds__(W8_BLOCK) void k_w8_emit_leaves(W8State S) {
    const uint32_t k = blockIdx.x * uint32_t(W8_BLOCK) + threadIdx.x;
    if (k < S.record_total) w8_emit_leaf(S, k);
}

#endif // the kernels

} // namespace hipr
