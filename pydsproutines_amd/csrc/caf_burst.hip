// Burst detection (filterRoutines.BurstDetector and its helpers, filterRoutines.py:701-1088, thresholding.cu:27-225):
//   * |x| and |x|^2 in one pass (BurstDetector.medfilt :805-819: d_absx = |x| (a hypot), d_ampSq = d_absx * d_absx);
//   * the exact sliding median == scipy.signal.medfilt(x, W) (zeros outside [0, n)), over order-preserving unsigned keys:
//       - small W (<= MED_SMALL_MAX): every thread holds its window's keys in registers and selects the rank-W/2 key by
//         counting (W^2 compares, no memory traffic beyond the tile);
//       - any W: a wavelet matrix over the keys (one level per key bit, built with a stable partition per level) answers
//         each window as a range-quantile query, 2 rank lookups per level whatever W is.  The padding zeros are never
//         materialised: the rank of +0.0 inside the clipped window decides whether the answer is a zero or which
//         order statistic of the real samples it is.  CAF_MEDFILT_GENERAL=1 forces this path;
//   * threshold edges in the reference's (rows, edgesMaxPerBlock) layout, one wave per row with 64-bit ballots;
//   * the pairing of the edges (gatherThresholdEdgesResults): compaction of the stored edges, then one workgroup runs the
//     state machine 1024 edges at a time as a segmented scan;
//   * above-threshold indices and their runs, a histogram over float64 edges, column means in float64.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "caf_internal.h"
#include "caf_wave.h"

namespace caf {

namespace {

unsigned grid_for(int64_t items, int64_t per_block, int64_t cap = 1 << 20) {
    const int64_t g = (items + per_block - 1) / per_block;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(g, cap));
}

// ---- order-preserving keys: a < b (IEEE, -0 < +0, NaN past +inf / before -inf by sign) <=> key(a) < key(b) ------------
template <typename T>
struct KeyOf;
template <>
struct KeyOf<float> {
    using K = uint32_t;
    static constexpr int BITS = 32;
    __device__ static K key(float v) {
        const uint32_t u = __float_as_uint(v);
        return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    __device__ static float val(K k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
};
template <>
struct KeyOf<double> {
    using K = uint64_t;
    static constexpr int BITS = 64;
    __device__ static K key(double v) {
        const uint64_t u = (uint64_t)__double_as_longlong(v);
        return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
    }
    __device__ static double val(K k) {
        return __longlong_as_double((long long)((k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k));
    }
};

__device__ __forceinline__ uint64_t lanemask_lt() { return (1ull << (threadIdx.x & 63)) - 1ull; }
__device__ __forceinline__ int64_t imin64(int64_t a, int64_t b) { return a < b ? a : b; }

// ---- |x|, |x|^2 -------------------------------------------------------------------------------------------------------
template <typename C, typename R>
__global__ __launch_bounds__(256) void k_abs_ampsq(const C* __restrict__ x, int64_t n, R* __restrict__ a, R* __restrict__ a2) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        R v;
        if constexpr (sizeof(C) == 2 * sizeof(R)) {
            const C z = x[i];
            // numpy's complex absolute: larger * sqrt(fma(r, r, 1)), r = smaller / larger (bit-identical to np.abs on a
            // host with FMA; the device hypot differs from it by an ulp or two on a third of the inputs)
            const R ax = fabs(z.x), ay = fabs(z.y);
            const R hi = ax > ay ? ax : ay, lo = ax > ay ? ay : ax;
            if (isinf(ax) || isinf(ay)) v = (R)INFINITY;
            else if (isnan(ax) || isnan(ay)) v = ax + ay;
            else if (hi == (R)0) v = (R)0;
            else {
                const R r = lo / hi;
                v = hi * sqrt(fma(r, r, (R)1));
            }
        } else {
            if constexpr (sizeof(R) == 4) v = fabsf(x[i]);
            else v = ::fabs(x[i]);
        }
        a[i] = v;
        a2[i] = v * v;
    }
}

// ---- median, small W: window keys in registers ------------------------------------------------------------------------
constexpr int MED_SMALL_MAX = 31;
constexpr int MED_TILE = 256;

template <typename T, int W>
__global__ __launch_bounds__(MED_TILE) void k_med_small(const T* __restrict__ x, int64_t n, T* __restrict__ out) {
    using KO = KeyOf<T>;
    using K = typename KO::K;
    constexpr int H = W / 2;
    __shared__ K s[MED_TILE + W - 1];
    const K k0 = KO::key((T)0);
    const int64_t ntiles = (n + MED_TILE - 1) / MED_TILE;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t base = t * MED_TILE - H;  // the key of sample base + j sits at s[j]
        for (int j = threadIdx.x; j < MED_TILE + W - 1; j += MED_TILE) {
            const int64_t i = base + j;
            s[j] = (i >= 0 && i < n) ? KO::key(x[i]) : k0;
        }
        __syncthreads();
        K w[W];
#pragma unroll
        for (int j = 0; j < W; ++j) w[j] = s[threadIdx.x + j];
        K r = w[0];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            int lt = 0, le = 0;
#pragma unroll
            for (int m = 0; m < W; ++m) {
                lt += w[m] < w[j];
                le += w[m] <= w[j];
            }
            if (lt <= H && H < le) r = w[j];
        }
        const int64_t i = t * MED_TILE + threadIdx.x;
        if (i < n) out[i] = KO::val(r);
        __syncthreads();
    }
}

// ---- median, any W: wavelet matrix -------------------------------------------------------------------------------------
// Level l (bit BITS-1-l, most significant first) holds the keys in the order the levels above left them: the bit vector
// of that level in words of 64 (bit set = 1) with the number of zeros before each word, and Z[l], its zero count.  The
// next level's order is the stable partition zeros-then-ones.  Tiles of WM_TILE keys: 4 waves x 16 chunks of 64.
constexpr int WM_TILE = 4096;
struct WmWord {
    uint64_t bits;
    uint64_t rank0;  // zeros before this word
};

// zeros of bit `bit` per tile (positions past n count as ones)
template <typename K>
__global__ __launch_bounds__(256) void k_wm_count(const K* __restrict__ a, int64_t n, int bit, int64_t ntiles,
                                                  int64_t* __restrict__ tile_cnt) {
    __shared__ int64_t s_w[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int64_t c = 0;
        const int64_t b0 = t * WM_TILE + (int64_t)wave * 1024;
#pragma unroll 4
        for (int ch = 0; ch < 16; ++ch) {
            const int64_t i = b0 + ch * 64 + lane;
            const bool zero = i < n && !((a[i] >> bit) & 1);
            c += __popcll(__ballot(zero));
        }
        const int64_t z = block_sum_totals(c, s_w);
        if (threadIdx.x == 0) tile_cnt[t] = z;
        __syncthreads();
    }
}

// the words of one level and (unless it is the last) the next level's order.  tile_off: scanned zero counts,
// tile_off[ntiles] = Z of the level
template <typename K>
__global__ __launch_bounds__(256) void k_wm_level(const K* __restrict__ a, int64_t n, int bit, int64_t ntiles,
                                                  const int64_t* __restrict__ tile_off, WmWord* __restrict__ words,
                                                  K* __restrict__ next, int64_t* __restrict__ zlevel) {
    __shared__ int64_t s_w[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t Z = tile_off[ntiles];
    if (blockIdx.x == 0 && threadIdx.x == 0) *zlevel = Z;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t b0 = t * WM_TILE + (int64_t)wave * 1024;
        K v[16];
        uint64_t ones[16];
        int64_t c = 0;
#pragma unroll
        for (int ch = 0; ch < 16; ++ch) {
            const int64_t i = b0 + ch * 64 + lane;
            v[ch] = i < n ? a[i] : (K)0;
            ones[ch] = __ballot(i >= n || ((v[ch] >> bit) & 1));
            c += 64 - __popcll(ones[ch]);
        }
        // (the carry of block_exclusive of caf_wave.h, spelled out: through the helper the uint32 form takes 97 VGPRs for 82,
        // one wave per SIMD fewer)
        if (lane == 0) s_w[wave] = c;
        __syncthreads();
        int64_t z = tile_off[t];
        for (int w = 0; w < wave; ++w) z += s_w[w];
#pragma unroll
        for (int ch = 0; ch < 16; ++ch) {
            const int64_t i = b0 + ch * 64 + lane;
            if (lane == 0) words[(b0 >> 6) + ch] = WmWord{ones[ch], (uint64_t)z};
            if (next != nullptr && i < n) {
                const bool one = (ones[ch] >> lane) & 1;
                const int64_t z_before = z + __popcll(~ones[ch] & lanemask_lt());
                next[one ? Z + (i - z_before) : z_before] = v[ch];
            }
            z += 64 - __popcll(ones[ch]);
        }
        __syncthreads();
    }
}

// zeros before position i (0 <= i <= n) of one level
__device__ __forceinline__ int64_t wm_rank0(const WmWord* __restrict__ w, int64_t i) {
    const WmWord q = w[i >> 6];
    const int off = (int)(i & 63);
    const uint64_t below = off ? (~q.bits & (~0ull >> (64 - off))) : 0ull;
    return (int64_t)q.rank0 + __popcll(below);
}

// the k-th smallest (0-based) key of the original positions [lo, hi)
template <typename K, int BITS>
__device__ K wm_quantile(const WmWord* __restrict__ words, int64_t nwl, const int64_t* __restrict__ Zs, int64_t lo, int64_t hi,
                         int64_t k) {
    K r = 0;
    for (int l = 0; l < BITS; ++l) {
        const WmWord* w = words + (int64_t)l * nwl;
        const int64_t zl = wm_rank0(w, lo), zh = wm_rank0(w, hi);
        const int64_t zeros = zh - zl;
        if (k < zeros) {
            lo = zl, hi = zh;
        } else {
            k -= zeros;
            r |= (K)1 << (BITS - 1 - l);
            const int64_t Z = Zs[l];
            lo = Z + (lo - zl), hi = Z + (hi - zh);
        }
    }
    return r;
}

// how many keys of the original positions [lo, hi) are < key
template <typename K, int BITS>
__device__ int64_t wm_count_less(const WmWord* __restrict__ words, int64_t nwl, const int64_t* __restrict__ Zs, int64_t lo,
                                 int64_t hi, K key) {
    int64_t c = 0;
    for (int l = 0; l < BITS && lo < hi; ++l) {
        const WmWord* w = words + (int64_t)l * nwl;
        const int64_t zl = wm_rank0(w, lo), zh = wm_rank0(w, hi);
        if ((key >> (BITS - 1 - l)) & 1) {
            c += zh - zl;
            const int64_t Z = Zs[l];
            lo = Z + (lo - zl), hi = Z + (hi - zh);
        } else {
            lo = zl, hi = zh;
        }
    }
    return c;
}

template <typename T>
__global__ __launch_bounds__(256) void k_to_keys(const T* __restrict__ x, int64_t n, typename KeyOf<T>::K* __restrict__ a) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) a[i] = KeyOf<T>::key(x[i]);
}

template <typename T>
__global__ __launch_bounds__(256) void k_wm_median(const WmWord* __restrict__ words, int64_t nwl, const int64_t* __restrict__ Zs,
                                                   int64_t n, int64_t W, T* __restrict__ out) {
    using KO = KeyOf<T>;
    using K = typename KO::K;
    const int64_t h = W / 2;
    const K k0 = KO::key((T)0);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t lo = i - h > 0 ? i - h : 0;
        const int64_t hi = (n - i - 1 > h) ? i + h + 1 : n;
        const int64_t pad = W - (hi - lo);  // the zeros outside [0, n)
        T r;
        if (pad > 0) {
            const int64_t below = wm_count_less<K, KO::BITS>(words, nwl, Zs, lo, hi, k0);
            if (h < below) r = KO::val(wm_quantile<K, KO::BITS>(words, nwl, Zs, lo, hi, h));
            else if (h < below + pad) r = (T)0;
            else r = KO::val(wm_quantile<K, KO::BITS>(words, nwl, Zs, lo, hi, h - pad));
        } else {
            r = KO::val(wm_quantile<K, KO::BITS>(words, nwl, Zs, lo, hi, h));
        }
        out[i] = r;
    }
}

template <typename T>
int medfilt_small(const T* x, int64_t n, int64_t W, T* out, hipStream_t st) {
    const unsigned g = grid_for(n, MED_TILE);
#define CAF_MED_CASE(w) \
    case w: hipLaunchKernelGGL((k_med_small<T, w>), dim3(g), dim3(MED_TILE), 0, st, x, n, out); break;
    switch ((int)W) {
        CAF_MED_CASE(1) CAF_MED_CASE(3) CAF_MED_CASE(5) CAF_MED_CASE(7) CAF_MED_CASE(9) CAF_MED_CASE(11) CAF_MED_CASE(13)
        CAF_MED_CASE(15) CAF_MED_CASE(17) CAF_MED_CASE(19) CAF_MED_CASE(21) CAF_MED_CASE(23) CAF_MED_CASE(25) CAF_MED_CASE(27)
        CAF_MED_CASE(29) CAF_MED_CASE(31)
        default: set_error("caf_medfilt: no small-window kernel for this size"); return CAF_ERR_INVALID;
    }
#undef CAF_MED_CASE
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

template <typename T>
int medfilt_wavelet(const T* x, int64_t n, int64_t W, T* out, hipStream_t st) {
    using K = typename KeyOf<T>::K;
    constexpr int BITS = KeyOf<T>::BITS;
    const int64_t ntiles = n / WM_TILE + 1;  // rank queries reach position n
    const int64_t nwl = ntiles * (WM_TILE / 64);
    Scratch sc(st);
    K *a = nullptr, *b = nullptr;
    WmWord* words = nullptr;
    int64_t *tiles = nullptr, *Zs = nullptr;
    int rc;
    if ((rc = sc.get(&a, n)) || (rc = sc.get(&b, n)) || (rc = sc.get(&words, nwl * BITS)) || (rc = sc.get(&tiles, ntiles + 1)) ||
        (rc = sc.get(&Zs, BITS)))
        return rc;
    hipLaunchKernelGGL(k_to_keys<T>, dim3(grid_for(n, 256)), dim3(256), 0, st, x, n, a);
    const unsigned gt = grid_for(ntiles, 1, 1 << 16);
    for (int l = 0; l < BITS; ++l) {
        const int bit = BITS - 1 - l;
        hipLaunchKernelGGL(k_wm_count<K>, dim3(gt), dim3(256), 0, st, a, n, bit, ntiles, tiles);
        launch_scan_exclusive(tiles, ntiles, st);
        hipLaunchKernelGGL(k_wm_level<K>, dim3(gt), dim3(256), 0, st, a, n, bit, ntiles, tiles, words + (int64_t)l * nwl,
                           l + 1 < BITS ? b : nullptr, Zs + l);
        std::swap(a, b);
    }
    hipLaunchKernelGGL(k_wm_median<T>, dim3(grid_for(n, 256)), dim3(256), 0, st, words, nwl, Zs, n, W, out);
    return sc.finish();
}

// ---- threshold edges: one wave per row ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_threshold_edges(const float* __restrict__ x, int64_t n, float thr, int32_t B,
                                                         int64_t rows, int32_t emax, int32_t* __restrict__ edges,
                                                         int32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += nwaves) {
        const int64_t first = r * B + 1;  // the row classifies [first, last]
        const int64_t last = imin64(r * B + B, n - 1);
        int32_t cnt = 0;
        int32_t* e = edges + r * emax;
        for (int64_t c0 = first; c0 <= last; c0 += 64) {
            const int64_t i = c0 + lane;
            const bool m = i < n && x[i] > thr;  // m[n] = 0
            bool ml = __shfl_up(m ? 1 : 0, 1, 64);
            bool mr = __shfl_down(m ? 1 : 0, 1, 64);
            if (lane == 0) ml = x[i - 1] > thr;  // 0 <= i - 1 < n - 1
            if (lane == 63) mr = i + 1 < n && x[i + 1] > thr;
            const bool ok = i <= last && m;
            const bool left = ok && !ml && mr, right = ok && ml && !mr;
            const uint64_t mask = __ballot(left || right);
            const int32_t pos = cnt + __popcll(mask & lanemask_lt());
            if ((left || right) && pos < emax) e[pos] = left ? (int32_t)i : -(int32_t)i;
            cnt += __popcll(mask);
        }
        for (int32_t j = (cnt < emax ? cnt : emax) + lane; j < emax; j += 64) e[j] = 0;
        if (lane == 0) counts[r] = cnt;
    }
}

// ---- gather: compaction of the stored edges, then the pairing state machine --------------------------------------------
constexpr int GE_TILE = 1024;  // rows per tile

__device__ __forceinline__ int32_t ge_stored(const int32_t* __restrict__ counts, int64_t r, int32_t emax) {
    const int32_t c = counts[r];
    return c <= 0 ? 0 : (c < emax ? c : emax);
}

// per tile of rows: the number of non-zero stored edges
__global__ __launch_bounds__(GE_TILE) void k_ge_count(const int32_t* __restrict__ edges, const int32_t* __restrict__ counts,
                                                      int64_t rows, int32_t emax, int64_t* __restrict__ tile_cnt) {
    __shared__ int64_t s_w[GE_TILE / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * GE_TILE + threadIdx.x;
    int64_t c = 0;
    if (r < rows) {
        const int32_t k = ge_stored(counts, r, emax);
        for (int32_t j = 0; j < k; ++j) c += edges[r * emax + j] != 0;
    }
    c = block_sum(c, s_w);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = c;
}

__global__ __launch_bounds__(GE_TILE) void k_ge_compact(const int32_t* __restrict__ edges, const int32_t* __restrict__ counts,
                                                        int64_t rows, int32_t emax, const int64_t* __restrict__ tile_off,
                                                        int32_t* __restrict__ flat) {
    __shared__ int64_t s_w[GE_TILE / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * GE_TILE + threadIdx.x;
    int32_t k = 0;
    int64_t c = 0;
    if (r < rows) {
        k = ge_stored(counts, r, emax);
        for (int32_t j = 0; j < k; ++j) c += edges[r * emax + j] != 0;
    }
    const int64_t incl = wave_scan_inclusive(c, lane);
    int64_t off = tile_off[blockIdx.x] + block_exclusive(incl, c, lane, wave, s_w);
    for (int32_t j = 0; j < k; ++j) {
        const int32_t v = edges[r * emax + j];
        if (v != 0) flat[off++] = v;
    }
}

// The state is `left` alone (0 after a pair, as at the start).  Within a segment that starts at a left edge L (or at the
// carried-in state), the first right edge R with min <= R - L <= max emits (L, R); every later R of the segment meets
// left = 0 and emits (0, R) when min <= R <= max.  So per chunk of 1024 edges: the segment of each edge (max-scan of the
// left-edge positions), the first passing R of each segment (a minimum in LDS), the emit flags and their scan.
__global__ __launch_bounds__(1024) void k_ge_pair(const int32_t* __restrict__ flat, const int64_t* __restrict__ total,
                                                  int32_t mn, int32_t mx, int32_t* __restrict__ pairs, int64_t cap,
                                                  int64_t* __restrict__ num_pairs) {
    __shared__ int32_t s_lval[1025];   // [p + 1]: the left edge at chunk position p (0 elsewhere); [0]: the carried-in state
    __shared__ int32_t s_first[1025];  // the first passing R of the segment that starts there
    __shared__ int32_t s_wave[16];
    __shared__ int32_t s_state;
    __shared__ int64_t s_out;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int me = (int)threadIdx.x;
    const int64_t T = *total;
    if (me == 0) s_state = 0, s_out = 0;
    __syncthreads();
    for (int64_t c0 = 0; c0 < T; c0 += 1024) {
        const int64_t j = c0 + me;
        const int32_t e = j < T ? flat[j] : 0;
        int32_t seg = wave_scan_inclusive(e > 0 ? me + 1 : 0, lane, [](int32_t a, int32_t b) { return max(a, b); });
        s_lval[me + 1] = e > 0 ? e : 0;
        s_first[me + 1] = 0x7fffffff;
        if (me == 0) s_lval[0] = s_state, s_first[0] = 0x7fffffff;
        seg = block_carry(seg, seg, lane, wave, s_wave, [](int32_t a, int32_t b) { return max(a, b); });
        const int32_t L = s_lval[seg];
        const int64_t R = e < 0 ? -(int64_t)e : 0;
        const int64_t d = R - L;
        if (e < 0 && d >= mn && d <= mx) atomicMin(&s_first[seg], me);
        __syncthreads();
        const int32_t f = s_first[seg];
        const bool emit = e < 0 && (me == f || (me > f && R >= mn && R <= mx));
        const uint64_t bal = __ballot(emit);
        const int32_t cnt = __popcll(bal);
        const int32_t before = block_exclusive(cnt, cnt, lane, wave, s_wave);  // emitted by the waves before this one
        const int64_t pos = s_out + before + __popcll(bal & lanemask_lt());
        if (emit && pos < cap) {
            pairs[2 * pos] = me == f ? L : 0;
            pairs[2 * pos + 1] = (int32_t)R;
        }
        __syncthreads();
        if (me == 1023) {
            s_out += before + cnt;
            // the chunk's last segment hands its state on: 0 once it has paired, else its left value
            s_state = s_first[seg] != 0x7fffffff ? 0 : s_lval[seg];
        }
        __syncthreads();
    }
    if (me == 0) *num_pairs = s_out;
}

// ---- above-threshold indices and runs --------------------------------------------------------------------------------
template <typename T, bool WRITE>
__global__ __launch_bounds__(256) void k_above(const T* __restrict__ x, int64_t n, T thr, int64_t ntiles,
                                               int64_t* __restrict__ tile_a, int64_t* __restrict__ tile_s,
                                               int64_t* __restrict__ idx, int64_t* __restrict__ starts) {
    __shared__ WaveSlots<4, int64_t, int64_t> s_as;  // (above, run starts)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t b0 = t * WM_TILE + (int64_t)wave * 1024;
        uint64_t ma[16], ms[16];
        int64_t ca = 0, cs = 0;
#pragma unroll
        for (int ch = 0; ch < 16; ++ch) {
            const int64_t i = b0 + ch * 64 + lane;
            const bool m = i < n && x[i] > thr;
            bool ml = __shfl_up(m ? 1 : 0, 1, 64);
            if (lane == 0) ml = i > 0 && i - 1 < n && x[i - 1] > thr;
            ma[ch] = __ballot(m);
            ms[ch] = __ballot(m && !ml);  // a run starts here
            ca += __popcll(ma[ch]);
            cs += __popcll(ms[ch]);
        }
        if (!WRITE) {
            block_sum_totals(s_as, ca, cs);
            if (threadIdx.x == 0) tile_a[t] = ca, tile_s[t] = cs;
        } else {
            // (two carries from ONE store and barrier: block_exclusive of caf_wave.h, spelled out for the pair)
            if (lane == 0) s_as.put(wave, ca, cs);
            __syncthreads();
            int64_t oa = tile_a[t], os = tile_s[t];
            for (int w = 0; w < wave; ++w) oa += s_as.a[w], os += s_as.rest.a[w];
#pragma unroll
            for (int ch = 0; ch < 16; ++ch) {
                const int64_t i = b0 + ch * 64 + lane;
                const int64_t ra = oa + __popcll(ma[ch] & lanemask_lt());
                if ((ma[ch] >> lane) & 1) idx[ra] = i;
                if ((ms[ch] >> lane) & 1) starts[os + __popcll(ms[ch] & lanemask_lt())] = ra;
                oa += __popcll(ma[ch]);
                os += __popcll(ms[ch]);
            }
        }
        __syncthreads();
    }
}

// ---- histogram over increasing float64 edges (np.histogram): LDS counts, one global add per bin per workgroup ----------
constexpr int HIST_LDS_BINS = 8192;

// v in [e[0], e[ne-1]]: the last edge <= v, the closed last bin taking v == e[ne-1]
__device__ __forceinline__ int64_t hist_bin(const double* __restrict__ e, int64_t ne, double v) {
    int64_t lo = 0, hi = ne - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (e[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo < ne - 1 ? lo : ne - 2;
}

template <typename T, bool LDS>
__global__ __launch_bounds__(256) void k_histogram(const T* __restrict__ x, int64_t n, const double* __restrict__ e, int64_t ne,
                                                   unsigned long long* __restrict__ counts) {
    __shared__ uint32_t s_c[LDS ? HIST_LDS_BINS : 1];
    const int64_t nb = ne - 1;
    if (LDS) {
        for (int64_t b = threadIdx.x; b < nb; b += 256) s_c[b] = 0;
        __syncthreads();
    }
    const double e0 = e[0], e1 = e[ne - 1];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double v = (double)x[i];
        if (v >= e0 && v <= e1) {  // (NaN fails both)
            const int64_t b = hist_bin(e, ne, v);
            if (LDS) atomicAdd(&s_c[b], 1u);
            else atomicAdd(&counts[b], 1ull);
        }
    }
    if (LDS) {
        __syncthreads();
        for (int64_t b = threadIdx.x; b < nb; b += 256)
            if (s_c[b]) atomicAdd(&counts[b], (unsigned long long)s_c[b]);
    }
}

// ---- column means of a (rows, cols) matrix in float64: partial sums per chunk of rows, then the chunks in order -------
constexpr int CM_CHUNKS = 64;

template <typename T>
__global__ __launch_bounds__(256) void k_colsum_part(const T* __restrict__ x, int64_t rows, int64_t cols, int32_t absolute,
                                                     int64_t rows_per, double* __restrict__ part) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per, r1 = imin64(rows, r0 + rows_per);
    double s = 0.0;
    for (int64_t r = r0; r < r1; ++r) {
        const double v = (double)x[r * cols + c];
        s += absolute ? ::fabs(v) : v;
    }
    part[(int64_t)blockIdx.y * cols + c] = s;
}

__global__ __launch_bounds__(256) void k_colsum_final(const double* __restrict__ part, int32_t nchunks, int64_t rows, int64_t cols,
                                                      double* __restrict__ out) {
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < cols; c += (int64_t)gridDim.x * 256) {
        double s = 0.0;
        for (int k = 0; k < nchunks; ++k) s += part[(int64_t)k * cols + c];
        out[c] = s / (double)rows;
    }
}

template <typename T>
int column_means(const T* x, int64_t rows, int64_t cols, int32_t absolute, double* out, hipStream_t st) {
    const int64_t nchunks = std::min<int64_t>(CM_CHUNKS, rows);
    const int64_t rows_per = (rows + nchunks - 1) / nchunks;
    const int64_t gx = (cols + 255) / 256;
    CAF_REQUIRE(gx <= 0x7fffffff, "caf_column_means: too many columns");
    Scratch sc(st);
    double* part = nullptr;
    const int rc = sc.get(&part, nchunks * cols);
    if (rc) return rc;
    hipLaunchKernelGGL(k_colsum_part<T>, dim3((unsigned)gx, (unsigned)nchunks), dim3(256), 0, st, x, rows, cols, absolute,
                       rows_per, part);
    hipLaunchKernelGGL(k_colsum_final, dim3(grid_for(cols, 256)), dim3(256), 0, st, part, (int32_t)nchunks, rows, cols, out);
    return sc.finish();
}

template <typename T>
int above_threshold(const T* x, int64_t n, T thr, int64_t* idx, int64_t idx_cap, int64_t* starts, int64_t starts_cap,
                    int64_t* h_counts, hipStream_t st) {
    const int64_t ntiles = (n + WM_TILE - 1) / WM_TILE;
    Scratch sc(st);
    int64_t *ta = nullptr, *ts = nullptr;
    int rc;
    if ((rc = sc.get(&ta, ntiles + 1)) || (rc = sc.get(&ts, ntiles + 1))) return rc;
    const unsigned g = grid_for(ntiles, 1, 1 << 16);
    hipLaunchKernelGGL((k_above<T, false>), dim3(g), dim3(256), 0, st, x, n, thr, ntiles, ta, ts, nullptr, nullptr);
    launch_scan_exclusive(ta, ntiles, st);
    launch_scan_exclusive(ts, ntiles, st);
    int64_t tot[2] = {0, 0};
    CAF_HIP_TRY(hipMemcpyAsync(&tot[0], ta + ntiles, 8, hipMemcpyDeviceToHost, st));
    CAF_HIP_TRY(hipMemcpyAsync(&tot[1], ts + ntiles, 8, hipMemcpyDeviceToHost, st));
    CAF_HIP_TRY(hipStreamSynchronize(st));
    h_counts[0] = tot[0], h_counts[1] = tot[1];
    if (idx != nullptr) {
        CAF_REQUIRE(idx_cap >= tot[0] && starts != nullptr && starts_cap >= tot[1], "caf_threshold_indices: outputs too small");
        hipLaunchKernelGGL((k_above<T, true>), dim3(g), dim3(256), 0, st, x, n, thr, ntiles, ta, ts, idx, starts);
    }
    return sc.finish();
}

template <typename T>
int histogram(const T* x, int64_t n, const double* e, int64_t ne, int64_t* counts, hipStream_t st) {
    CAF_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)(ne - 1) * 8, st));
    if (n == 0) return CAF_OK;
    const unsigned g = grid_for(n, 256 * 16, 4096);
    if (ne - 1 <= HIST_LDS_BINS)
        hipLaunchKernelGGL((k_histogram<T, true>), dim3(g), dim3(256), 0, st, x, n, e, ne, (unsigned long long*)counts);
    else
        hipLaunchKernelGGL((k_histogram<T, false>), dim3(g), dim3(256), 0, st, x, n, e, ne, (unsigned long long*)counts);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

}  // namespace

}  // namespace caf

using namespace caf;

int32_t caf_abs_ampsq(const void* d_x, int64_t n, int32_t dtype, void* d_abs, void* d_ampsq, void* stream) {
    CAF_REQUIRE(dtype >= 0 && dtype <= 3, "caf_abs_ampsq: dtype must be 0 (complex64), 1 (complex128), 2 (float32), 3 (float64)");
    CAF_REQUIRE(n >= 0, "caf_abs_ampsq: n < 0");
    if (n == 0) return CAF_OK;
    CAF_REQUIRE(d_x && d_abs && d_ampsq, "caf_abs_ampsq: NULL buffer");
    hipStream_t st = (hipStream_t)stream;
    const unsigned g = grid_for(n, 256, 1 << 16);
    switch (dtype) {
        case 0:
            hipLaunchKernelGGL((k_abs_ampsq<float2, float>), dim3(g), dim3(256), 0, st, (const float2*)d_x, n, (float*)d_abs,
                               (float*)d_ampsq);
            break;
        case 1:
            hipLaunchKernelGGL((k_abs_ampsq<double2, double>), dim3(g), dim3(256), 0, st, (const double2*)d_x, n,
                               (double*)d_abs, (double*)d_ampsq);
            break;
        case 2:
            hipLaunchKernelGGL((k_abs_ampsq<float, float>), dim3(g), dim3(256), 0, st, (const float*)d_x, n, (float*)d_abs,
                               (float*)d_ampsq);
            break;
        default:
            hipLaunchKernelGGL((k_abs_ampsq<double, double>), dim3(g), dim3(256), 0, st, (const double*)d_x, n, (double*)d_abs,
                               (double*)d_ampsq);
            break;
    }
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_medfilt(const void* d_x, int64_t n, int32_t is_f64, int64_t kernel_size, void* d_out, void* stream) {
    CAF_REQUIRE(kernel_size >= 1 && (kernel_size & 1), "caf_medfilt: kernel_size must be odd and >= 1");
    CAF_REQUIRE(n >= 0, "caf_medfilt: n < 0");
    if (n == 0) return CAF_OK;
    CAF_REQUIRE(d_x && d_out, "caf_medfilt: NULL buffer");
    hipStream_t st = (hipStream_t)stream;
    // CAF_MEDFILT_GENERAL=1 forces the wavelet path (cross-checks, A/B); read per call like CAF_WOLA_FUSED
    const char* eg = std::getenv("CAF_MEDFILT_GENERAL");
    const bool small = kernel_size <= MED_SMALL_MAX && !(eg && eg[0] == '1');
    if (const char* ed = std::getenv("CAF_MEDFILT_DEBUG"))
        if (ed[0] == '1')
            std::fprintf(stderr, "[caf medfilt] path=%s n=%lld W=%lld f64=%d\n", small ? "small" : "wavelet", (long long)n,
                         (long long)kernel_size, (int)is_f64);
    if (is_f64)
        return small ? medfilt_small((const double*)d_x, n, kernel_size, (double*)d_out, st)
                     : medfilt_wavelet((const double*)d_x, n, kernel_size, (double*)d_out, st);
    return small ? medfilt_small((const float*)d_x, n, kernel_size, (float*)d_out, st)
                 : medfilt_wavelet((const float*)d_x, n, kernel_size, (float*)d_out, st);
}

int32_t caf_threshold_edges(const float* d_x, int64_t n, float threshold, int32_t threads_per_block, int32_t edges_max,
                            int32_t* d_edges, int32_t* d_counts, void* stream) {
    CAF_REQUIRE(threads_per_block >= 3 && threads_per_block <= 1024, "caf_threshold_edges: threads_per_block must be in [3, 1024]");
    CAF_REQUIRE(edges_max >= 1, "caf_threshold_edges: edges_max must be >= 1");
    CAF_REQUIRE(n >= 0 && n <= 0x7fffffff, "caf_threshold_edges: n must be < 2^31 (edges are int32)");
    const int32_t B = threads_per_block - 2;
    const int64_t rows = (n + B - 1) / B;
    if (rows == 0) return CAF_OK;
    CAF_REQUIRE(d_x && d_edges && d_counts, "caf_threshold_edges: NULL buffer");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_threshold_edges, dim3(grid_for(rows, 4, 1 << 18)), dim3(256), 0, st, d_x, n, threshold, B, rows,
                       edges_max, d_edges, d_counts);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_gather_edges(const int32_t* d_edges, int64_t rows, int32_t edges_max, const int32_t* d_counts, int32_t min_len,
                         int32_t max_len, int32_t* d_pairs, int64_t capacity, int64_t* h_num_pairs, void* stream) {
    CAF_REQUIRE(rows >= 0 && edges_max >= 1 && capacity >= 0 && h_num_pairs, "caf_gather_edges: bad arguments");
    *h_num_pairs = 0;
    if (rows == 0) return CAF_OK;
    CAF_REQUIRE(d_edges && d_counts && (capacity == 0 || d_pairs), "caf_gather_edges: NULL buffer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t ntiles = (rows + GE_TILE - 1) / GE_TILE;
    CAF_REQUIRE(ntiles <= 0x7fffffff, "caf_gather_edges: too many rows");
    Scratch sc(st);
    int64_t *tiles = nullptr, *np = nullptr;
    int32_t* flat = nullptr;
    int rc;
    if ((rc = sc.get(&tiles, ntiles + 1)) || (rc = sc.get(&np, 1))) return rc;
    hipLaunchKernelGGL(k_ge_count, dim3((unsigned)ntiles), dim3(GE_TILE), 0, st, d_edges, d_counts, rows, edges_max, tiles);
    launch_scan_exclusive(tiles, ntiles, st);
    int64_t T = 0;
    CAF_HIP_TRY(hipMemcpyAsync(&T, tiles + ntiles, 8, hipMemcpyDeviceToHost, st));
    CAF_HIP_TRY(hipStreamSynchronize(st));
    if (T == 0) return sc.finish();
    if ((rc = sc.get(&flat, T))) return rc;
    hipLaunchKernelGGL(k_ge_compact, dim3((unsigned)ntiles), dim3(GE_TILE), 0, st, d_edges, d_counts, rows, edges_max, tiles, flat);
    hipLaunchKernelGGL(k_ge_pair, dim3(1), dim3(1024), 0, st, flat, tiles + ntiles, min_len, max_len, d_pairs, capacity, np);
    CAF_HIP_TRY(hipGetLastError());
    int64_t K = 0;
    CAF_HIP_TRY(hipMemcpyAsync(&K, np, 8, hipMemcpyDeviceToHost, st));
    CAF_HIP_TRY(hipStreamSynchronize(st));
    *h_num_pairs = K;
    return sc.finish();
}

int32_t caf_threshold_indices(const void* d_x, int64_t n, int32_t is_f64, double threshold, int64_t* d_idx, int64_t idx_cap,
                              int64_t* d_run_starts, int64_t runs_cap, int64_t* h_counts, void* stream) {
    CAF_REQUIRE(n >= 0 && h_counts, "caf_threshold_indices: bad arguments");
    h_counts[0] = h_counts[1] = 0;
    if (n == 0) return CAF_OK;
    CAF_REQUIRE(d_x, "caf_threshold_indices: NULL buffer");
    hipStream_t st = (hipStream_t)stream;
    if (is_f64) return above_threshold((const double*)d_x, n, threshold, d_idx, idx_cap, d_run_starts, runs_cap, h_counts, st);
    return above_threshold((const float*)d_x, n, (float)threshold, d_idx, idx_cap, d_run_starts, runs_cap, h_counts, st);
}

int32_t caf_histogram(const void* d_x, int64_t n, int32_t is_f64, const double* d_edges, int64_t num_edges, int64_t* d_counts,
                      void* stream) {
    CAF_REQUIRE(n >= 0 && num_edges >= 2 && d_edges && d_counts, "caf_histogram: bad arguments");
    CAF_REQUIRE(n == 0 || d_x, "caf_histogram: NULL buffer");
    hipStream_t st = (hipStream_t)stream;
    if (is_f64) return histogram((const double*)d_x, n, d_edges, num_edges, d_counts, st);
    return histogram((const float*)d_x, n, d_edges, num_edges, d_counts, st);
}

int32_t caf_column_means(const void* d_x, int64_t rows, int64_t cols, int32_t is_f64, int32_t absolute, double* d_out,
                         void* stream) {
    CAF_REQUIRE(rows >= 1 && cols >= 1 && d_x && d_out, "caf_column_means: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (is_f64) return column_means((const double*)d_x, rows, cols, absolute, d_out, st);
    return column_means((const float*)d_x, rows, cols, absolute, d_out, st);
}
