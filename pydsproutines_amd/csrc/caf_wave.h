// Cross-lane reductions and scans of one wave (wave64) and the folds of a workgroup's waves through LDS, shared by the
// ahead-of-time kernels.  Two contracts of the library live here and nowhere else:
//
//  * Tie rule: of equal maxima the LOWER INDEX wins, so every arg max reports the first index of the maximum however the
//    elements were dealt to lanes, waves and workgroups -- what np.argmax and the reference's kernels report, and what lets
//    engines that cut the same data differently agree bit for bit.  (A lane visits its own indices in increasing order and
//    keeps the first maximum with a strict `>`; everywhere else the rule is first_max: in wave_argmax across lanes, in
//    block_argmax across the waves of a workgroup, and by name in the loops that compare (value, index) pairs.)
//  * Summation order: the offsets of a sum and of a scan are compile-time constants applied in one fixed order (xor
//    butterfly WIDTH/2 ... 1; scan 1 ... 32; wave totals in increasing wave order from wave 0), so a floating-point sum
//    is a function of the data and the launch geometry alone, never of scheduling: no atomics, no order of arrival.
//    Changing an order here changes result bits everywhere.
//
// What lives here: first_max / first_min; wave_sum, wave_max, wave_scan_inclusive, wave_argmax; block_sum (one value
// through an array, or several through a WaveSlots record and one barrier), block_sum_totals, block_max, block_argmax,
// block_argmin -- one barrier, the LDS in use until the caller's next one -- and the _all forms, whose trailing barrier
// frees the LDS; block_exclusive, the carry of a workgroup scan of sums, over block_carry, which takes the operator (k_scan_exclusive
// of caf_rows.hip is the whole scan by one workgroup).  The block helpers take their LDS from the caller (a WaveSlots
// or an array of WAVES entries), so a kernel's LDS is all declared in the kernel, and index lanes and waves by threadIdx.x.
//
// Hand-written on purpose, with the same rule: caf_fused.hip, caf_perdelay.hip and caf_perdelay_mr.hip (double-buffered
// LDS slots that these helpers do not model; the launches the published figures rest on), k_prefix_tiles (its own
// summation orders, and one more VGPR through a helper), k_cutout_sumsq (a pairwise order of the wave totals), the
// 16-thread tile fold of caf_cancel.hip, the carry of k_wm_level (15 more VGPRs through block_exclusive: a wave per SIMD
// fewer), the two carries of k_above's write pass and the carry-and-total of k_cancel_subtract (each from ONE store and
// barrier) and wave_best of k_magsq_norm_argmax (at 256 VGPRs; docs/LAB_NOTEBOOK.md).
//
// Not for the run-time-compiled kernels (caf_perdelay_jit.h has its own DPP group_max) and not to be included from the
// headers embedded for them (caf_fft_dev.h, caf_mr_dev.h, caf_energy.h, caf_perdelay_jit.h).
#pragma once
#include <hip/hip_runtime.h>

namespace caf {

// the tie rule: does (ov, oi) take over from (v, i)?  The larger value, and of equal values the lower index.
template <typename V, typename I>
__device__ __forceinline__ bool first_max(V v, I i, V ov, I oi) {
    return ov > v || (ov == v && oi < i);
}
// its twin for an arg min: the smaller value, and of equal values the lower index
template <typename V, typename I>
__device__ __forceinline__ bool first_min(V v, I i, V ov, I oi) {
    return ov < v || (ov == v && oi < i);
}

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
            if (first_max(v, i, ov, oi)) {
                v = ov;
                i = oi;
                ((payload = op), ...);
            }
        }(__shfl_xor(payload, o, 64)...);
    }
}

// ---- a workgroup of WAVES waves: its waves' results folded through the caller's LDS ------------------------------------

// the wave totals added in increasing wave order from wave 0: THE order of a workgroup's sum
template <int WAVES, typename T>
__device__ __forceinline__ T slot_sum(const T (&a)[WAVES]) {
    T t = a[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) t += a[w];
    return t;
}

// one LDS slot per wave for each field of a record (value, index, payloads ...), field by field
template <int WAVES, typename T, typename... R>
struct WaveSlots {
    T a[WAVES];
    WaveSlots<WAVES, R...> rest;
    __device__ __forceinline__ void put(int w, T v, R... r) { a[w] = v, rest.put(w, r...); }
    __device__ __forceinline__ void get(int w, T& v, R&... r) const { v = a[w], rest.get(w, r...); }
    __device__ __forceinline__ void sum(T& v, R&... r) const { v = slot_sum(a), rest.sum(r...); }
};
template <int WAVES, typename T>
struct WaveSlots<WAVES, T> {
    T a[WAVES];
    __device__ __forceinline__ void put(int w, T v) { a[w] = v; }
    __device__ __forceinline__ void get(int w, T& v) const { v = a[w]; }
    __device__ __forceinline__ void sum(T& v) const { v = slot_sum(a); }
};

// sum over the workgroup (slot_sum's order), returned in every thread; `lds` stays in use until the caller's next barrier.
// block_sum_totals: from wave totals the caller already has, such as a ballot's popcount.
template <int WAVES, typename T>
__device__ __forceinline__ T block_sum_totals(T total, T (&lds)[WAVES]) {
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = total;
    __syncthreads();
    return slot_sum(lds);
}
template <int WAVES, typename T>
__device__ __forceinline__ T block_sum(T v, T (&lds)[WAVES]) {
    return block_sum_totals(wave_sum(v), lds);
}
// ... `lds` free again on return
template <int WAVES, typename T>
__device__ __forceinline__ T block_sum_all(T v, T (&lds)[WAVES]) {
    const T t = block_sum(v, lds);
    __syncthreads();
    return t;
}
// several sums through one barrier, in place: the same three forms on a WaveSlots record with one field per sum
template <int WAVES, typename... T>
__device__ __forceinline__ void block_sum_totals(WaveSlots<WAVES, T...>& lds, T&... total) {
    if ((threadIdx.x & 63) == 0) lds.put(threadIdx.x >> 6, total...);
    __syncthreads();
    lds.sum(total...);
}
template <int WAVES, typename... T>
__device__ __forceinline__ void block_sum(WaveSlots<WAVES, T...>& lds, T&... v) {
    ((v = wave_sum(v)), ...);
    block_sum_totals(lds, v...);
}
template <int WAVES, typename... T>
__device__ __forceinline__ void block_sum_all(WaveSlots<WAVES, T...>& lds, T&... v) {
    block_sum(lds, v...);
    __syncthreads();
}

// maximum over the workgroup (packed keys: see wave_max), in thread 0
template <int WAVES, typename T>
__device__ __forceinline__ T block_max(T v, T (&lds)[WAVES]) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < WAVES; ++w) v = lds[w] > v ? lds[w] : v;
    }
    return v;
}

// (value, index) arg max over the workgroup, the waves' records folded with first_max in wave order; `payload` fields
// travel with the winner.  In place, the result in thread 0.
template <int WAVES, typename V, typename I, typename... P>
__device__ __forceinline__ void block_argmax(WaveSlots<WAVES, V, I, P...>& lds, V& v, I& i, P&... payload) {
    wave_argmax(v, i, payload...);
    if ((threadIdx.x & 63) == 0) lds.put(threadIdx.x >> 6, v, i, payload...);
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < WAVES; ++w)
            if (first_max(v, i, lds.a[w], lds.rest.a[w])) lds.get(w, v, i, payload...);
    }
}
// ... result in every thread, `lds` free again on return
template <int WAVES, typename V, typename I, typename... P>
__device__ __forceinline__ void block_argmax_all(WaveSlots<WAVES, V, I, P...>& lds, V& v, I& i, P&... payload) {
    wave_argmax(v, i, payload...);
    if ((threadIdx.x & 63) == 0) lds.put(threadIdx.x >> 6, v, i, payload...);
    __syncthreads();
    lds.get(0, v, i, payload...);
#pragma unroll
    for (int w = 1; w < WAVES; ++w)
        if (first_max(v, i, lds.a[w], lds.rest.a[w])) lds.get(w, v, i, payload...);
    __syncthreads();
}
// (value, index) arg min over the workgroup: the arg max of the negated values (first_min and first_max agree on them, signed
// zeros included, and a NaN wins neither).  In place, the result in thread 0.
template <int WAVES, typename V, typename I>
__device__ __forceinline__ void block_argmin(WaveSlots<WAVES, V, I>& lds, V& v, I& i) {
    v = -v;
    block_argmax(lds, v, i);
    v = -v;
}

// the carry of a workgroup scan under `op`: lane 63 leaves the wave's inclusive total `incl`, and after the barrier `first`
// (what the thread starts from: its own value within the wave, with whatever the caller carries in) takes up the totals
// of the waves before this one in wave order.  `lane`, `wave`: the caller's threadIdx.x & 63 and threadIdx.x >> 6.
template <int WAVES, typename T, typename Op>
__device__ __forceinline__ T block_carry(T first, T incl, int lane, int wave, T (&lds)[WAVES], Op op) {
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    for (int w = 0; w < wave; ++w) first = op(first, lds[w]);
    return first;
}
// the sum: from the inclusive scan `incl` of `v` over the wave to the exclusive scan over the workgroup, (incl - v) plus
// the totals of the waves before (a wave-uniform total is its own inclusive value: block_exclusive(c, c, ...) is what the
// waves before this one add up to)
template <int WAVES, typename T>
__device__ __forceinline__ T block_exclusive(T incl, T v, int lane, int wave, T (&lds)[WAVES]) {
    return block_carry(incl - v, incl, lane, wave, lds, [](T a, T b) { return a + b; });
}

}  // namespace caf
