// TraceHintStartHost.hip -- the start of a hinted ray and the next-item step of the 8-wide trace kernel (csrc/wide8_kernels.h hint_start, next_item_of_group),
// compiled for the HOST by hipcc's host pass (tests/native/libtrace_hint_start_host.so).
//
// Test infrastructure (tests/test_trace_hint_start_cpu.py); nothing here is linked into or loaded by the product, which has no CPU path.
//
// Both are __host__ __device__ routines of integer arithmetic; next_item_of_group is the text the kernel's loop expands in place (WIDE8_NEXT_ITEM). The CPU suite uses
// them for the two claims the hints of k_trace_wide8 rest on: from the hinted start state the next-item step yields the root and then the item sequence of an unhinted
// ray, and an entry of another generation, or of a slot outside the tree, is refused.
#define HIPR_HOST_DEVICE 1
#define HIPR_SHADE_TU 1      // none of the kernels of the other translation units: this build holds host code only
#define HIPR_FAST_MATH 0
#ifndef HIPR_VERIFY_MATH
#define HIPR_VERIFY_MATH 1
#endif
#include "../../bifrost3d_amd/csrc/wide8_kernels.h"

using namespace hipr;

extern "C" {

// hint_start on (hint, tag, slot_count, octant) from the unhinted start state: out3 = {accepted, item, gy}.
void trace_hint_start_host_start(uint32_t hint, uint32_t hint_tag, uint32_t slot_count, uint32_t octant, uint32_t* out3) {
    uint32_t item = slot_count == 0 ? ITEM_FINISHED : 0u, gy = 1u << 8;      // as the kernel sets a new ray up
    out3[0] = hint_start(hint, hint_tag, slot_count, octant, item, gy) ? 1u : 0u;
    out3[1] = item;
    out3[2] = gy;
}

// The items a ray takes from the group (gx, gy) and what the step leaves of it: next_item_of_group until the group is empty, at most `capacity` items.
// items[k] = the k-th item, groups[k] = gy after it. Returns the number of items, ITEM_FINISHED included.
uint32_t trace_hint_start_host_items(uint32_t gx, uint32_t gy, uint32_t octant, uint32_t capacity, uint32_t* items, uint32_t* groups) {
    uint32_t count = 0;
    while (count < capacity) {
        const uint32_t item = next_item_of_group(gx, gy, octant);
        items[count] = item;
        groups[count] = gy;
        ++count;
        if (item == ITEM_FINISHED) break;
    }
    return count;
}

}
