// gfx950 reduction kernels of the stand-alone toolbox with their entry points: |x|^2, moving sums and means, and the
// maxima over items and columns.  CDNA4 counterparts -- by semantics, not by code -- of the reference's
//   custom_kernels/complex_magn.cu:8-19       complex_magnSq_kernel<T,U>
//   custom_kernels/filter.cu:196-347,374-438  movingAverage / multiMovingAverage / movingComplexSum
//   custom_kernels/argmax.cu:11-81            multiArgmax3d_uint32
// All are HBM-bound elementwise / sliding-window work.
#include <algorithm>

#include "caf_internal.h"
#include "caf_stage.h"
#include "caf_wave.h"

namespace caf {

// multiArgmax3d_uint32 (argmax.cu:11-81): per item, argmax over the last three dimensions of a
// (items, d1, d2, d3) uint32 array -> the three indices (+ the maximum).  First flat index on ties;
// an all-zero item reports (0, 0, 0) like the reference's zero-initialised workspace.
__global__ __launch_bounds__(256) void k_argmax3d_u32(const uint32_t* __restrict__ x, int32_t d1, int32_t d2, int32_t d3,
                                                      uint32_t* __restrict__ argmax, uint32_t* __restrict__ maxv) {
    __shared__ WaveSlots<4, uint32_t, uint32_t> s_best;
    const int64_t n = (int64_t)d1 * d2 * d3;
    const uint32_t* xi = x + (int64_t)blockIdx.x * n;
    uint32_t bv = 0, bi = 0;
    for (int64_t t = threadIdx.x; t < n; t += 256) {
        const uint32_t v = xi[t];
        if (v > bv) {
            bv = v;
            bi = (uint32_t)t;
        }
    }
    block_argmax(s_best, bv, bi);
    if (threadIdx.x == 0) {
        argmax[blockIdx.x * 3 + 0] = bi / (uint32_t)(d2 * d3);
        argmax[blockIdx.x * 3 + 1] = (bi / (uint32_t)d3) % (uint32_t)d2;
        argmax[blockIdx.x * 3 + 2] = bi % (uint32_t)d3;
        if (maxv) maxv[blockIdx.x] = bv;
    }
}

// |x|^2, elementwise.  IN: 0 complex64, 1 complex128.  OUT: 0 float32, 1 float64.
template <typename TIn, typename TOut>
__global__ __launch_bounds__(256) void k_magnsq(const TIn* __restrict__ x, int64_t n, TOut* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const TIn v = x[i];
        out[i] = (TOut)(v.x * v.x + v.y * v.y);
    }
}

// ---------------------------------------------------------------------------------------
// Causal moving sum / mean of float32 (zeros in front), double accumulation (filter.cu:324-339).
// Two forms: float64 prefixes per MA_TILE-sample tile in global memory (any window), and k_moving_tile below
// (windows up to MAT_MAXL, one launch).
// ---------------------------------------------------------------------------------------
constexpr int MA_THREADS = 256;
constexpr int MA_PER_THREAD = 16;
constexpr int MA_TILE = MA_THREADS * MA_PER_THREAD;

// The long-window form (L > MAT_MAXL, or more rows than one launch of k_moving_tile takes) keeps no prefix of the whole
// record: a difference of two entries of such a prefix is off by 2^-53 of everything in front of the window, which is
// the whole window where the record is far louder somewhere before it.  local[i] = the sum of x over [tile start, i) of
// the MA_TILE-sample tile that holds index i (i in [0, n]) and tile_sums[t] = the total of tile t; a window is then
//   the tail of its first tile (total - local: a difference within ONE tile) + the whole tiles between + the head of its last,
// so that nothing is subtracted across more than MA_TILE samples -- what the upstream kernel's per-thread re-anchoring
// achieves (filter.cu:324-339).  The tile form's reach was not raised instead: its LDS prefix holds span = window + outputs
// doubles, so the outputs per workgroup shrink as the window grows and no span serves every window length.
__global__ __launch_bounds__(MA_THREADS) void k_moving_prefix_write(const float* __restrict__ x, int64_t n,
                                                                    double* __restrict__ tile_sums,
                                                                    double* __restrict__ local) {
    __shared__ double s_wave[MA_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * MA_TILE + (int64_t)threadIdx.x * MA_PER_THREAD;
    double p[MA_PER_THREAD];
    double tot = 0.0;
#pragma unroll
    for (int j = 0; j < MA_PER_THREAD; ++j) {
        p[j] = tot;
        if (base + j < n) tot += (double)x[base + j];
    }
    const double incl = wave_scan_inclusive(tot, lane);
    const double off = block_exclusive(incl, tot, lane, wave, s_wave);
#pragma unroll
    for (int j = 0; j < MA_PER_THREAD; ++j)
        if (base + j <= n) local[base + j] = off + p[j];
    if (threadIdx.x == MA_THREADS - 1) tile_sums[blockIdx.x] = off + tot;  // (the same additions as an entry one past the tile)
}

// out[i] = sum x[max(0, i+1-L) .. i] [/ L] from the tile-local prefixes and the tile totals
__global__ __launch_bounds__(256) void k_moving_from_prefix(const double* __restrict__ local, const double* __restrict__ tile_sums,
                                                            int64_t n, int32_t L, int32_t sum_instead, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t hi = i + 1, lo = hi > L ? hi - L : 0;
    const int64_t ta = lo / MA_TILE, tb = hi / MA_TILE;
    double s;
    if (ta == tb) {
        s = local[hi] - local[lo];
    } else {
        s = tile_sums[ta] - local[lo];
        for (int64_t t = ta + 1; t < tb; ++t) s += tile_sums[t];
        s += local[hi];
    }
    out[i] = sum_instead ? (float)s : (float)(s / (double)L);
}

// Causal moving sum / mean in ONE launch for windows up to MAT_MAXL: a workgroup covers MAT_SPAN consecutive samples
// (its outputs preceded by a halo of the window, zeros before the start), each thread 8 of them straight from two
// 16-byte loads; their float64 inclusive prefix is built in registers (thread, wave shuffle, wave totals) and only the
// prefix goes through LDS, once: out[i] = P[i] - P[i - L].  No global prefix array, no scratch; 4 B read + 4 B written
// per sample plus the halo.  (The form this replaces staged the samples in LDS as well and read them twice: six LDS
// operations per sample against three, 47 us against the time in profiles/ for 2^24 samples.)
constexpr int MAT_NT = 256, MAT_PER = 8;
constexpr int MAT_SPAN = MAT_NT * MAT_PER;
constexpr int MAT_MAXL = 1024;
// prefix through slot t lives at s_p[mat_slot(t + 1)]: one pad per 8 entries, so that the 8-consecutive writes of a
// thread (stride 9 doubles across lanes) and the consecutive reads of the output loop both spread over the banks
__device__ __forceinline__ int mat_slot(int t) { return t + (t >> 3); }
__host__ __device__ inline int mat_halo(int L) { return (L - 1 + 3) & ~3; }       // slots before the first output
__host__ __device__ inline int mat_outputs(int L) { return MAT_SPAN - mat_halo(L); }  // outputs per workgroup (multiple of 4)

__global__ __launch_bounds__(MAT_NT) void k_moving_tile(const float* __restrict__ x, int64_t n, int32_t L, int32_t sum_instead,
                                                        float* __restrict__ out) {
    __shared__ double s_p[MAT_SPAN + MAT_SPAN / 8 + 2];
    __shared__ double s_wave[MAT_NT / 64];
    const float* xr = x + (int64_t)blockIdx.y * n;
    float* outr = out + (int64_t)blockIdx.y * n;
    const int H = mat_halo(L), T = MAT_SPAN - H;
    const int64_t i0 = (int64_t)blockIdx.x * T;  // first output of the workgroup; slot t <-> sample i0 - H + t
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t0 = threadIdx.x * MAT_PER;
    const int64_t j0 = i0 - H + t0;
    float v[MAT_PER];
    if (j0 >= 0 && j0 + MAT_PER <= n && (reinterpret_cast<uintptr_t>(xr + j0) & 15) == 0) {
        const float4 a = *reinterpret_cast<const float4*>(xr + j0), b = *reinterpret_cast<const float4*>(xr + j0 + 4);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
    } else {
#pragma unroll
        for (int k = 0; k < MAT_PER; ++k) v[k] = (j0 + k >= 0 && j0 + k < n) ? xr[j0 + k] : 0.f;
    }
    double pl[MAT_PER];
    double tot = 0.0;
#pragma unroll
    for (int k = 0; k < MAT_PER; ++k) pl[k] = (tot += (double)v[k]);
    const double incl = wave_scan_inclusive(tot, lane);
    if (threadIdx.x == 0) s_p[0] = 0.0;
    const double off = block_exclusive(incl, tot, lane, wave, s_wave);
#pragma unroll
    for (int k = 0; k < MAT_PER; ++k) s_p[mat_slot(t0 + k + 1)] = off + pl[k];
    __syncthreads();
    for (int l = threadIdx.x; l < T; l += MAT_NT) {
        const int64_t i = i0 + l;
        if (i >= n) break;
        const int t = H + l;  // window of output i: slots t - L + 1 .. t
        const double s = s_p[mat_slot(t + 1)] - s_p[mat_slot(t + 1 - L)];
        outr[i] = sum_instead ? (float)s : (float)(s / (double)L);
    }
}

// valid-only forward moving complex sum -> |sum|^2 (filter.cu:374-438): direct O(L) per output in f64
// staged through LDS (L is small in the reference's use: symbol-length sums).
__global__ __launch_bounds__(256) void k_complex_moving_sum(const float2* __restrict__ x, int64_t n, int32_t L,
                                                            float* __restrict__ out) {
    extern __shared__ float2 s_x[];  // 256*CMS_PER + L - 1 samples
    constexpr int PER = 8;
    const int64_t o0 = (int64_t)blockIdx.x * 256 * PER;
    const int64_t nout = n - L + 1;
    const int span = 256 * PER + L - 1;
    stage_batched<8>(span, [&](int t) { const int64_t j = o0 + t; return (j < n) ? x[j] : make_float2(0.f, 0.f); },
                     [&](int t, float2 v) { s_x[t] = v; });
    __syncthreads();
    const int l0 = threadIdx.x * PER;
    double sr = 0.0, si = 0.0;
    for (int k = 0; k < L; ++k) {
        sr += (double)s_x[l0 + k].x;
        si += (double)s_x[l0 + k].y;
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int64_t o = o0 + l0 + j;
        if (o < nout) out[o] = (float)(sr * sr + si * si);
        sr += (double)s_x[l0 + j + L].x - (double)s_x[l0 + j].x;
        si += (double)s_x[l0 + j + L].y - (double)s_x[l0 + j].y;
    }
}

// per column i of complex (rows, n): max_r |z[r][i]| and its first row index (int32, or int64 = cp.argmax's dtype)
template <typename TArg>
__global__ __launch_bounds__(256) void k_colmax_abs(const float2* __restrict__ z, int32_t rows, int64_t n,
                                                    float* __restrict__ maxv, TArg* __restrict__ arg) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float bv = -1.f;
    TArg bi = 0;
    for (int r = 0; r < rows; ++r) {
        const float2 a = z[(int64_t)r * n + i];
        // |z| via float64 so that the float32 result is the correctly rounded one (== numpy/hypotf)
        const float v = (float)sqrt((double)a.x * (double)a.x + (double)a.y * (double)a.y);
        if (v > bv) {
            bv = v;
            bi = r;
        }
    }
    maxv[i] = bv;
    arg[i] = bi;
}

// per column i of a real (rows, n) matrix of QF^2 values: max_r sqrt(q[r][i]) and its first row (int64, the dtype
// of cp.argmax) -- TemplateCrossCorrelator.correlate(returnMax=True) on per-template QF^2 traces; the comparison
// is made on the float32 square roots, like the reference's on |QF| (xcorrRoutines.py:361-371)
__global__ __launch_bounds__(256) void k_colmax_sqrt(const float* __restrict__ q, int32_t rows, int64_t n,
                                                     float* __restrict__ maxv, int64_t* __restrict__ arg) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float bv = -1.f;
    int64_t bi = 0;
    for (int r = 0; r < rows; ++r) {
        const float v = sqrtf(q[(int64_t)r * n + i]);
        if (v > bv) {
            bv = v;
            bi = r;
        }
    }
    maxv[i] = bv;
    arg[i] = bi;
}

static int64_t moving_num_tiles(int64_t n) { return (n + 1 + MA_TILE - 1) / MA_TILE; }

static void launch_moving_average(const float* x, int64_t n, int32_t L, int32_t sum_instead, double* tile_sums,
                           double* prefix, float* out, hipStream_t st) {
    const int64_t nt = moving_num_tiles(n);
    hipLaunchKernelGGL(k_moving_prefix_write, dim3((unsigned)nt), dim3(MA_THREADS), 0, st, x, n, tile_sums, prefix);
    hipLaunchKernelGGL(k_moving_from_prefix, dim3(cdiv(n, 256)), dim3(256), 0, st, prefix, tile_sums, n, L, sum_instead, out);
}

static int moving_tile_max_window() { return MAT_MAXL; }

}  // namespace caf

using namespace caf;

int32_t caf_complex_magnsq(const void* d_x, int64_t n, int32_t in_c128, void* d_out, int32_t out_f64, void* stream) {
    CAF_REQUIRE(d_x && d_out && n >= 0, "caf_complex_magnsq: bad arguments");
    CAF_REQUIRE(!(in_c128 && !out_f64), "complex128 input needs float64 output");
    if (n) {
        hipStream_t st = (hipStream_t)stream;
        const unsigned g = std::min<unsigned>(cdiv(n, 256), 256 * 16);
        if (!in_c128 && !out_f64)
            hipLaunchKernelGGL((k_magnsq<float2, float>), dim3(g), dim3(256), 0, st, (const float2*)d_x, n, (float*)d_out);
        else if (!in_c128 && out_f64)
            hipLaunchKernelGGL((k_magnsq<float2, double>), dim3(g), dim3(256), 0, st, (const float2*)d_x, n, (double*)d_out);
        else
            hipLaunchKernelGGL((k_magnsq<double2, double>), dim3(g), dim3(256), 0, st, (const double2*)d_x, n, (double*)d_out);
    }
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_moving_average(const float* d_x, int64_t rows, int64_t n, int32_t avg_length, int32_t sum_instead,
                           float* d_out, void* stream) {
    CAF_REQUIRE(d_x && d_out && rows >= 1 && n >= 1 && avg_length >= 1, "caf_moving_average: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (avg_length <= moving_tile_max_window() && rows <= 65535) {  // one launch, no scratch, asynchronous
        hipLaunchKernelGGL(k_moving_tile, dim3(cdiv(n, mat_outputs(avg_length)), (unsigned)rows), dim3(MAT_NT), 0, st, d_x, n,
                           avg_length, sum_instead, d_out);
        CAF_HIP_TRY(hipGetLastError());
        return CAF_OK;
    }
    Scratch sc(st, true);
    double *tiles = nullptr, *prefix = nullptr;
    int rc = sc.get(&tiles, moving_num_tiles(n) + 1024);
    if (rc) return rc;
    if ((rc = sc.get(&prefix, n + 1))) return rc;
    for (int64_t r = 0; r < rows; ++r)
        launch_moving_average(d_x + r * n, n, avg_length, sum_instead, tiles, prefix, d_out + r * n, st);
    return sc.finish();
}

int32_t caf_complex_moving_sum(const float* d_x, int64_t n, int32_t sum_length, float* d_out, void* stream) {
    CAF_REQUIRE(d_x && d_out && sum_length >= 1 && n >= sum_length, "caf_complex_moving_sum: bad arguments");
    CAF_REQUIRE(sum_length <= 4096, "sum_length too long for the LDS-resident kernel");
    const int64_t nout = n - sum_length + 1;
    const size_t sm = (size_t)(256 * 8 + sum_length - 1 + 8) * sizeof(float2);
    hipLaunchKernelGGL(k_complex_moving_sum, dim3(cdiv(nout, 256 * 8)), dim3(256), sm, (hipStream_t)stream, (const float2*)d_x, n,
                       sum_length, d_out);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_argmax3d_u32(const uint32_t* d_x, int64_t num_items, int32_t dim1, int32_t dim2, int32_t dim3,
                         uint32_t* d_argmax, uint32_t* d_max, void* stream) {
    CAF_REQUIRE(d_x && d_argmax && num_items >= 0 && dim1 >= 1 && dim2 >= 1 && dim3 >= 1, "caf_argmax3d_u32: bad arguments");
    CAF_REQUIRE((int64_t)dim1 * dim2 * dim3 < ((int64_t)1 << 32) && num_items < ((int64_t)1 << 31),
                "caf_argmax3d_u32: item too large");
    if (num_items > 0)  // (::dim3: the type, not the argument)
        hipLaunchKernelGGL(k_argmax3d_u32, ::dim3((unsigned)num_items), ::dim3(256), 0, (hipStream_t)stream, d_x, dim1, dim2, dim3,
                           d_argmax, d_max);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_colmax_abs(const float* d_z, int32_t rows, int64_t n, float* d_max, void* d_arg, int32_t arg_int64,
                       void* stream) {
    CAF_REQUIRE(d_z && d_max && d_arg && rows >= 1 && n >= 1, "caf_colmax_abs: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (arg_int64)
        hipLaunchKernelGGL(k_colmax_abs<int64_t>, dim3(cdiv(n, 256)), dim3(256), 0, st, (const float2*)d_z, rows, n, d_max,
                           (int64_t*)d_arg);
    else
        hipLaunchKernelGGL(k_colmax_abs<int32_t>, dim3(cdiv(n, 256)), dim3(256), 0, st, (const float2*)d_z, rows, n, d_max,
                           (int32_t*)d_arg);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_colmax_sqrt(const float* d_q2, int32_t rows, int64_t n, float* d_max, int64_t* d_arg, void* stream) {
    CAF_REQUIRE(d_q2 && d_max && d_arg && rows >= 1 && n >= 1, "caf_colmax_sqrt: bad arguments");
    hipLaunchKernelGGL(k_colmax_sqrt, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, d_q2, rows, n, d_max, d_arg);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}
