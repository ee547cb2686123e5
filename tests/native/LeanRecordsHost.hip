// LeanRecordsHost.hip -- the triangle test of the trace kernels (csrc/kernels.h triangle_inside) and the two-step analytic light test of the 8-wide kernel's
// retire (csrc/wide8_kernels.h analytic_light_reachable, analytic_light_distance_of), compiled for the HOST by hipcc's host pass
// (tests/native/liblean_records_host.so).
//
// Test infrastructure (tests/test_record_without_second_triangle_cpu.py); nothing here is linked into or loaded by the product, which has no CPU path.
//
// Both are __host__ __device__ functions of IEEE f32 arithmetic in a fixed order; `hipcc --cuda-host-only -ffp-contract=off` yields an x86 build of exactly the
// statements the kernels run. The CPU suite uses it for the two claims the lean record block and the lean retire of k_trace_wide8 rest on: a leaf record of one
// triangle (e3 = +0) cannot be hit through its absent B whatever the ray, and the two-step light test returns analytic_light_distance's value, NaN for NaN.
#define HIPR_HOST_DEVICE 1
#define HIPR_SHADE_TU 1      // none of the kernels of the other translation units: this build holds host code only
#define HIPR_FAST_MATH 0
#ifndef HIPR_VERIFY_MATH
#define HIPR_VERIFY_MATH 1
#endif
#include "../../bifrost3d_amd/csrc/wide8_kernels.h"

using namespace hipr;

namespace {

f3 words3(const uint32_t* w) { return mk3(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2])); }

}

extern "C" {

// Ray i (origin and direction, 3 floats each) against triangle `which` (0: A = (a; e1, e2), 1: B = (a; e2, e3)) of record record_of[i] (16 words each, HiprLeaf8):
// inside[i] = triangle_inside's answer, det_bits[i] = the bits of the determinant it found. Returns how many rays are inside.
uint32_t lean_records_host_inside(const uint32_t* records, const uint32_t* record_of, const float* origins, const float* directions, uint32_t n, int which, uint8_t* inside,
                                  uint32_t* det_bits) {
    uint32_t count = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t* r = records + 16 * size_t(record_of[i]);
        const f3 a = words3(r), first = words3(r + (which == 0 ? 3 : 6)), second = words3(r + (which == 0 ? 6 : 9));
        TriangleTest test;
        const bool hit = triangle_inside(a, first, second, mk3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]), mk3(directions[3 * i], directions[3 * i + 1], directions[3 * i + 2]), test);
        inside[i] = hit ? 1 : 0;
        det_bits[i] = __float_as_uint(test.det);
        count += hit ? 1u : 0u;
    }
    return count;
}

// Ray i against one light (HiprLight): whole[i] = analytic_light_distance, two_step[i] = analytic_light_distance_of where analytic_light_reachable says yes and
// NaN where it says no, reachable[i] its answer.
void lean_records_host_light(const HiprLight* light, const float* origins, const float* directions, uint32_t n, float* whole, float* two_step, uint8_t* reachable) {
    for (uint32_t i = 0; i < n; ++i) {
        const f3 o = mk3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]), d = mk3(directions[3 * i], directions[3 * i + 1], directions[3 * i + 2]);
        whole[i] = analytic_light_distance(*light, o, d);
        float along, disc;
        const bool can = analytic_light_reachable(*light, o, d, along, disc);
        reachable[i] = can ? 1 : 0;
        two_step[i] = can ? analytic_light_distance_of(*light, along, disc) : __builtin_nanf("");
    }
}

}
