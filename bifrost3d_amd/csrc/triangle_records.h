// triangle_records.h -- the two kernels that derive the per-triangle records of the resident scene from its pools and triangles: launched by
// ResidentScene::queue_triangle_records (scene.hip) and compiled in that unit alone. The records' layouts are kernels.h's ("Shading records", DeviceScene).
#pragma once

#include "kernels.h"

namespace hipr {

// What the trace kernels read per triangle: the vertex and the two edges the test works on (the edges rounded once, here, as
// the oracle rounds them), ids and flags where the uploaded triangle has them.
__global__ __launch_bounds__(256) void k_build_trace_triangles(const float4* __restrict__ triangles, uint32_t triangle_count, float4* __restrict__ out) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= triangle_count) return;
    const float4 a = triangles[3 * size_t(t)], b = triangles[3 * size_t(t) + 1], c = triangles[3 * size_t(t) + 2];
    const f3 v0 = mk3(a.x, a.y, a.z), e1 = mk3(a.w, b.x, b.y) - v0, e2 = mk3(b.z, b.w, c.x) - v0;
    out[3 * size_t(t)] = make_float4(v0.x, v0.y, v0.z, e1.x);
    out[3 * size_t(t) + 1] = make_float4(e1.y, e1.z, e2.x, e2.y);
    out[3 * size_t(t) + 2] = make_float4(e2.z, c.y, c.z, c.w);
}

__global__ __launch_bounds__(256) void k_build_shade_triangles(DeviceScene sc, float4* out) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= sc.triangle_count) return;
    build_shade_triangle_record(sc, t, out);
}

} // namespace hipr
