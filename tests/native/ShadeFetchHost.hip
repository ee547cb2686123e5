// ShadeFetchHost.hip -- the two fetch stages of the shade kernel (csrc/shade_kernel.h shade_entry, shade_fetch_inputs, shade_fetch_by_kind), compiled for the
// HOST by hipcc's host pass (tests/native/libshade_fetch_host.so).
//
// Test infrastructure (tests/test_shade_fetch_kinds_cpu.py); nothing here is linked into or loaded by the product, which has no CPU path.
//
// The routines are __host__ __device__ functions of loads and integer compares: the x86 build runs exactly the statements k_shade runs for a place of its
// shading order, so the CPU suite can say field by field what an entry of each kind holds once both stages have run -- and that a kind reads no array it has
// no use for (the arrays handed in hold distinct patterns; a field that was not loaded keeps what it held before the stage).
#define HIPR_HOST_DEVICE 1
#define HIPR_SHADE_TU 1      // none of the kernels of the other translation unit: this build holds host code only
#define HIPR_FAST_MATH 0
#ifndef HIPR_VERIFY_MATH
#define HIPR_VERIFY_MATH 1
#endif
#include "../../bifrost3d_amd/csrc/shade_kernel.h"

using namespace hipr;

namespace {

void write_record(const ShadeInputs& r, float* o) {
    o[0] = __uint_as_float(r.entry); o[1] = __uint_as_float(r.meta.x); o[2] = __uint_as_float(r.meta.y);
    const float4 fields[4] = {r.o, r.d, r.t, r.hit};
    for (int k = 0; k < 4; ++k) { o[3 + 4 * k] = fields[k].x; o[4 + 4 * k] = fields[k].y; o[5 + 4 * k] = fields[k].z; o[6 + 4 * k] = fields[k].w; }
}

}

extern "C" {

uint32_t shade_fetch_host_record_words() { return 19u; }
uint32_t shade_fetch_host_dead_slot() { return HIPR_DEAD_SLOT; }

// Places 0 .. places - 1 of the shading order of a queue of n entries (`order`: the listing, or null for the queue's own order; places from n on hold no entry),
// each taken through both stages as k_shade takes it. Records of 19 words: bits(entry), bits(slot), bits(last triangle), origin field (4), direction field (4),
// throughput + bounces (4), hit (4): `after_inputs` as shade_fetch_inputs leaves them, `after_kind` as shade_fetch_by_kind leaves them, its word 0 holding shade_holds_radiance (1: k_shade adds to the origin field) in place of the entry. With
// `prefill` the origin and direction fields are set to it (8 floats) between the stages, so that a field the second stage does not load shows the prefill and not the zero of the first.
void shade_fetch_host(uint32_t n, uint32_t places, const uint32_t* order, int aov, int environment_lookup, float* o_tmin, float* d_pdf, float* thr_bounces, uint32_t* meta,
                      const float* hits, const float* radiance, const float* prefill, float* after_inputs, float* after_kind) {
    PathState in;
    in.o_tmin = reinterpret_cast<float4*>(o_tmin); in.d_pdf = reinterpret_cast<float4*>(d_pdf); in.thr_bounces = reinterpret_cast<float4*>(thr_bounces);
    in.meta = reinterpret_cast<uint2*>(meta);
    for (uint32_t j = 0; j < places; ++j) {
        ShadeInputs r = shade_fetch_inputs(in, reinterpret_cast<const float4*>(hits), shade_entry(order, j, n));
        write_record(r, after_inputs + 19 * size_t(j));
        if (prefill) { r.o = make_float4(prefill[0], prefill[1], prefill[2], prefill[3]); r.d = make_float4(prefill[4], prefill[5], prefill[6], prefill[7]); }
        if (aov) shade_fetch_by_kind<true>(in, reinterpret_cast<const float4*>(radiance), environment_lookup != 0, r);
        else shade_fetch_by_kind<false>(in, reinterpret_cast<const float4*>(radiance), environment_lookup != 0, r);
        // what k_shade asks before it adds to the path's radiance: does the origin field hold radiance[slot]?
        const bool holds = aov ? shade_holds_radiance<true>(r) : shade_holds_radiance<false>(r);
        write_record(r, after_kind + 19 * size_t(j));
        after_kind[19 * size_t(j)] = __uint_as_float(holds ? 1u : 0u);
    }
}

}
