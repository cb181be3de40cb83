// Cross-lane reductions and scans of one wave (wave64), shared by the ahead-of-time kernels.  Two contracts of the
// library live here and nowhere else:
//
//  * Tie rule: of equal maxima the LOWER INDEX wins, so every arg max reports the first index of the maximum however the
//    elements were dealt to lanes, waves and workgroups -- what np.argmax and the reference's kernels report, and what lets
//    engines that cut the same data differently agree bit for bit.  (A lane visits its own indices in increasing order and
//    keeps the first maximum with a strict `>`; across lanes the rule is wave_argmax; where a workgroup folds its waves'
//    results through LDS, the fold spells the same comparison.)
//  * Summation order: the offsets of a sum and of a scan are compile-time constants applied in one fixed order (xor
//    butterfly WIDTH/2 ... 1; scan 1 ... 32), so a floating-point sum is a function of the data and the launch geometry
//    alone, never of scheduling: no atomics, no order of arrival.  Changing an order here changes result bits everywhere.
//
// Not for the run-time-compiled kernels (caf_perdelay_jit.h has its own DPP group_max) and not to be included from the
// headers embedded for them (caf_fft_dev.h, caf_mr_dev.h, caf_energy.h, caf_perdelay_jit.h).
#pragma once
#include <hip/hip_runtime.h>

namespace caf {

// sum over each aligned group of WIDTH lanes, left in every lane of the group
template <int WIDTH = 64, typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = WIDTH / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// maximum over each aligned group of WIDTH lanes, left in every lane of the group (the packed (value << 32 | ~index)
// keys carry the tie rule in their low half)
template <int WIDTH = 64, typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int o = WIDTH / 2; o > 0; o >>= 1) {
        const T u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

// inclusive scan over the wave: lane l gets op(v[0], ..., v[l]); `lane` is the caller's threadIdx.x & 63
template <typename T, typename Op>
__device__ __forceinline__ T wave_scan_inclusive(T v, int lane, Op op) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o, 64);
        if (lane >= o) v = op(v, u);
    }
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_scan_inclusive(T v, int lane) {
    return wave_scan_inclusive(v, lane, [](T a, T b) { return a + b; });
}

// (value, index) arg max over xor offsets HI ... LO (the full wave by default; HI = 32, LO = 16 folds only the four
// 16-lane groups together, HI = 8 reduces within groups of 16); `payload` fields travel with the winner.  In place, the
// result in every participating lane.
template <int HI = 32, int LO = 1, typename V, typename I, typename... P>
__device__ __forceinline__ void wave_argmax(V& v, I& i, P&... payload) {
#pragma unroll
    for (int o = HI; o >= LO; o >>= 1) {
        const V ov = __shfl_xor(v, o, 64);
        const I oi = __shfl_xor(i, o, 64);
        // (the payloads are shuffled by every lane, before the divergent update)
        [&](auto... op) {
            if (ov > v || (ov == v && oi < i)) {
                v = ov;
                i = oi;
                ((payload = op), ...);
            }
        }(__shfl_xor(payload, o, 64)...);
    }
}

}  // namespace caf
