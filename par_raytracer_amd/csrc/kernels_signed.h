// kernels_signed.h - the pseudonormal accumulators of prt_signed_distance (dev_signed.h), filled on the device from the triangle
// records as they lie there now.
//
//   k_signed_normals   phase 0 zeroes the (position_count + edge_count) x 3 accumulators; phase 1, one lane per leaf slot, reads the
//                      slot's record, forms its unit normal and its three angles (signed_triangle_terms) and adds the 9 vertex
//                      integers and 3 x 3 edge integers with 64-bit integer atomics: the sums are the same bits for every launch
//                      shape and arrival order.  The two phases are two launches on one stream.
// Launched by the first signed query after an upload or after a prt_update_geometry (prt_api.hip: ensure_signed_tables).
#pragma once

#include "dev_signed.h"

namespace prt {

PRT_D void signed_add3(long long * acc, size_t at, const long long * q) {
    for (int k = 0; k < 3; ++k)
        __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(acc + 3u * at + k), (unsigned long long)q[k], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_signed_normals(const float4 * tris, unsigned int n_tris, SignedTables T, int phase) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (phase == 0) {
        const size_t words = 3u * ((size_t)T.position_count + T.edge_count);
        for (size_t i = gid; i < words; i += stride) T.acc[i] = 0;
        return;
    }
    for (size_t slot = gid; slot < n_tris; slot += stride) {
        const float4 * tp = tris + 3u * slot;
        const float4 r0 = tp[0], r1 = tp[1], r2 = tp[2];
        f3 n;
        float alpha[3];
        if (!signed_triangle_terms(mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), n, alpha)) continue;
        long long vq[9], eq[3];
        signed_triangle_fixed(n, alpha, vq, eq);
        const unsigned int * row = T.adj + 6u * slot;
        for (int k = 0; k < 3; ++k) {
            signed_add3(T.acc, (size_t)row[k], vq + 3 * k);
            signed_add3(T.acc, (size_t)T.position_count + row[3 + k], eq);
        }
    }
}

}  // namespace prt
