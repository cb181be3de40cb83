// The LDS staging loop of the toolbox kernels that stage a window with batched loads (caf_fir.hip, caf_slices.hip, caf_reduce.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace caf {

// LDS staging loops: element t = tid, tid + 256, ... of `count`, value load(t), stored by store(t, value).  STG loads per
// thread are issued before the first of them is stored: written element by element (load, wait, store) the round trips of
// a thread's share stand one after the other in front of the workgroup's barrier.  Worth 7-10 % on the decimating filters
// (128 taps / 4 on 2^24 samples: 72 -> 65 us), nothing on the others -- several workgroups per CU cover one another -- and
// -4 % on k_upfirdn_poly, which keeps its plain loops (profiles/r04/ab_staging_loops.log).
template <int STG, typename Load, typename Store>
__device__ __forceinline__ void stage_batched(int count, Load&& load, Store&& store) {
    for (int t0 = threadIdx.x; t0 < count; t0 += 256 * STG) {
        decltype(load(0)) v[STG];
#pragma unroll
        for (int u = 0; u < STG; ++u)
            if (t0 + 256 * u < count) v[u] = load(t0 + 256 * u);
#pragma unroll
        for (int u = 0; u < STG; ++u)
            if (t0 + 256 * u < count) store(t0 + 256 * u, v[u]);
    }
}

}  // namespace caf
