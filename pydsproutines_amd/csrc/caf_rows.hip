// gfx950 kernels of the per-delay (time-domain product) path and the toolbox kernels that more than one translation unit
// launches, with their launchers (caf_internal.h) and the entry points that are nothing but these kernels.
// CDNA4 counterparts -- by semantics, not by code -- of the reference's
//   custom_kernels/multiplySlices.cu:113-216  slidingMultiplyNormalised
//   custom_kernels/argmax.cu:93-153           multiArgmaxAbsRows_complex64
//   custom_kernels/peakfinding.cu:14-58       findLocalMaxima
// All are HBM-bound elementwise / sliding-window work.
#include <algorithm>

#include "caf_internal.h"
#include "caf_energy.h"
#include "caf_wave.h"

namespace caf {

// sum |x|^2 of a complex64 vector in float64 as NORM_PARTS partial sums (fixed assignment of elements to workgroups
// and a fixed summation order: the result does not depend on scheduling); the consumer adds the partials up.
// Replaces a blocking device-to-host copy + host loop in front of the per-delay path.
constexpr int NORM_PARTS = 128;
__global__ __launch_bounds__(256) void k_cutout_sumsq(const float2* __restrict__ x, int64_t n, double* __restrict__ parts) {
    __shared__ double s[4];
    double e = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)NORM_PARTS * 256) {
        const float2 a = x[i];
        e += (double)a.x * a.x + (double)a.y * a.y;
    }
    e = wave_sum(e);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = e;
    __syncthreads();
    // (PAIRWISE over the wave totals: block_sum of caf_wave.h adds them in sequence and would change the float64 bits)
    if (threadIdx.x == 0) parts[blockIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
}
__global__ void k_cutout_final(double* __restrict__ parts) {  // parts[NORM_PARTS] = sqrt(sum of the partials), fixed order
    double t = 0.0;
    for (int i = 0; i < NORM_PARTS; ++i) t += parts[i];
    parts[NORM_PARTS] = sqrt(t);
}
int cutout_norm_scratch_doubles() { return NORM_PARTS + 1; }
// returns the device address of ||x|| (valid once the two kernels have run on `st`)
const double* launch_cutout_norm(const float2* x, int64_t n, double* parts, hipStream_t st) {
    hipLaunchKernelGGL(k_cutout_sumsq, dim3(NORM_PARTS), dim3(256), 0, st, x, n, parts);
    hipLaunchKernelGGL(k_cutout_final, dim3(1), dim3(1), 0, st, parts);
    return parts + NORM_PARTS;
}

// ---------------------------------------------------------------------------------------
// z[i][t] = x[t] * y[s_i + t] / (sqrt(E_i) * coef),  s_i = start + i*step,
// E_i = sum_t |y[s_i + t]|^2 from the f64 prefix array (samples past the end of y read as 0).
// Rows whose window does not lie inside [0, ylen) are written as zeros when zero_oor != 0
// (IppXcorrFFT.cpp:125-130 semantics), otherwise they are computed with zero padding
// (multiplySlices.cu:147-163 semantics).
// ---------------------------------------------------------------------------------------
// A workgroup handles `rpw` consecutive rows (short rows: one 1/sqrt(E) in float64 per LANE instead of one per wave --
// for 1000-sample rows the float64 square root and division were three quarters of the instructions) and the
// blockIdx.x-th chunk of their samples.
constexpr int SM_MAX_RPW = 64;
__global__ __launch_bounds__(256) void k_sliding_multiply(const float2* __restrict__ x, int32_t xlen,
                                                          const float2* __restrict__ y, int64_t ylen,
                                                          const double* __restrict__ prefix, int64_t start,
                                                          int64_t step, double coef, int32_t zero_oor,
                                                          float2* __restrict__ z, const double* __restrict__ d_coef,
                                                          int64_t rows, int32_t rpw, int32_t rows_fastest) {
    __shared__ float s_inv[SM_MAX_RPW];
    // rows_fastest (long rows): the row groups are the fast grid dimension, so the workgroups in flight work on the SAME chunk of
    // x and of the (overlapping) windows of y for different rows and find it in the L2 / Infinity Cache -- with the chunks fastest
    // every row group streamed both arrays from HBM again (128 rows of 10^7 samples: 5.6 GB fetched for 0.16 GB of inputs)
    const uint32_t bx = rows_fastest ? blockIdx.y : blockIdx.x, by = rows_fastest ? blockIdx.x : blockIdx.y;
    const uint32_t gdx = rows_fastest ? gridDim.y : gridDim.x;
    const int64_t row0 = (int64_t)by * rpw;
    if ((int)threadIdx.x < rpw && row0 + threadIdx.x < rows) {
        const int64_t s = start + (row0 + threadIdx.x) * step;
        const bool oor = (s < 0) || (s + xlen > ylen);
        float inv = 0.f;
        if (!(oor && zero_oor)) {
            int64_t a = s < 0 ? 0 : (s > ylen ? ylen : s);
            int64_t b = s + xlen;
            b = b < 0 ? 0 : (b > ylen ? ylen : b);
            const double e = window_energy(prefix, y, ylen, a, b);  // (exact where the difference is not: caf_energy.h)
            inv = (float)(1.0 / (sqrt(e) * (d_coef ? coef * *d_coef : coef)));
        }
        s_inv[threadIdx.x] = inv;
    }
    __syncthreads();
    // four rows at a time: x[t] is loaded once for them, and with consecutive delays (step 1) the four y loads of a thread
    // are the neighbouring threads' lines -- per output 8 + 8 bytes came from L2 / the Infinity Cache, now about a quarter of
    // that (long rows, 128 x 10^7 outputs: 715 -> 665 us per batch; non-temporal stores and one contiguous chunk of t per
    // workgroup instead of the grid stride were measured too: no change / 10 % slower; round 4: two outputs per lane with 16-byte
    // stores: no change on 1430-sample rows, 10 % slower on 10^7-sample ones.  A write-only stream reaches 4.4 .. 6.1 TB/s on this
    // chip, scripts/ubench/stream_rw.hip: the 4.3 TB/s of the short rows are at that ceiling)
    for (int r = 0; r < rpw && row0 + r < rows; r += 4) {
        int64_t sq[4];
        bool zq[4], live[4];
        float iq[4];
        float2* zrow[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            live[q] = r + q < rpw && row0 + r + q < rows;
            sq[q] = start + (row0 + r + q) * step;
            zq[q] = ((sq[q] < 0) || (sq[q] + xlen > ylen)) && zero_oor;
            iq[q] = live[q] ? s_inv[r + q] : 0.f;
            zrow[q] = z + (row0 + r + q) * (int64_t)xlen;
        }
        for (int t = bx * 256 + threadIdx.x; t < xlen; t += gdx * 256) {
            const float2 a = x[t];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (!live[q]) continue;
                float2 o = make_float2(0.f, 0.f);
                const int64_t j = sq[q] + t;
                if (!zq[q] && j >= 0 && j < ylen) {
                    const float2 b = y[j];
                    o.x = (a.x * b.x - a.y * b.y) * iq[q];
                    o.y = (a.x * b.y + a.y * b.x) * iq[q];
                }
                zrow[q][t] = o;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// Row post-processing after the row FFT: per row r of (rows, len) complex64
//   argmax[r] (first index of the maximum of |z|^2), max[r] (|z|^2 or |z|),
//   optional |z|^2 plane (float32), all scaled by `scale`.
// One workgroup per row.
// ---------------------------------------------------------------------------------------
// nan_empty: an all-NaN row reports (NaN, 0) -- the per-delay path's zero-energy window, the reference's pmax / norm / 0
// (xcorrRoutines.py:527-528) -- instead of the (0, 0) of the CUDA kernel's zero-initialised workspace
__global__ __launch_bounds__(256) void k_rows_argmax(const float2* __restrict__ z, int64_t len, int32_t use_normsq,
                                                     float scale, uint32_t* __restrict__ argmax,
                                                     float* __restrict__ maxv, float* __restrict__ plane, int32_t nan_empty) {
    __shared__ WaveSlots<4, float, uint32_t> s_best;
    const int64_t row = blockIdx.x;
    const float2* zr = z + row * len;
    float bv = -1.f;
    uint32_t bi = 0;
    for (int64_t t = threadIdx.x; t < len; t += 256) {
        const float2 a = zr[t];
        const float v = (a.x * a.x + a.y * a.y) * scale;
        if (plane) plane[row * len + t] = v;
        if (v > bv) {
            bv = v;
            bi = (uint32_t)t;
        }
    }
    block_argmax(s_best, bv, bi);
    if (threadIdx.x == 0) {
        if (bv < 0.f) {  // empty or all-NaN row: the reference's zero-initialised workspace (argmax.cu:108-109)
            bv = (nan_empty && len > 0) ? __builtin_nanf("") : 0.f;
            bi = 0;
        }
        if (argmax) argmax[row] = bi;
        if (maxv) maxv[row] = use_normsq ? bv : sqrtf(bv);
    }
}

// Many short rows (the per-delay path's product rows: 10^5 rows of ~10^3 elements): one WAVE per row, four rows per
// workgroup -- no barrier, no LDS --, 16-byte loads (two elements per lane and instruction, four instructions in flight).
// A row that starts 8 bytes off a 16-byte boundary gives its first element to lane 0.  Per lane the indices are visited in
// increasing order, so the strict comparison keeps the first maximum; across lanes the lower index wins ties.
__global__ __launch_bounds__(256) void k_rows_argmax_wave(const float2* __restrict__ z, int64_t rows, int64_t len, int32_t use_normsq,
                                                          float scale, uint32_t* __restrict__ argmax, float* __restrict__ maxv,
                                                          float* __restrict__ plane, int32_t nan_empty) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;  // (wave-uniform)
    const float2* zr = z + row * len;
    float* pr = plane ? plane + row * len : nullptr;
    float bv = -1.f;
    uint32_t bi = 0;
    auto offer = [&](float2 a, int64_t t) {
        const float v = (a.x * a.x + a.y * a.y) * scale;
        if (pr) pr[t] = v;
        if (v > bv) {
            bv = v;
            bi = (uint32_t)t;
        }
    };
    const int head = (int)((reinterpret_cast<uintptr_t>(zr) >> 3) & 1);
    if (head && lane == 0 && len > 0) offer(zr[0], 0);
    const int64_t nv = len > head ? (len - head) >> 1 : 0;
    const float4* zv = reinterpret_cast<const float4*>(zr + head);
#pragma unroll 4
    for (int64_t p = lane; p < nv; p += 64) {
        const float4 q = zv[p];
        offer(make_float2(q.x, q.y), head + 2 * p);
        offer(make_float2(q.z, q.w), head + 2 * p + 1);
    }
    if (len > head && ((len - head) & 1) && lane == 0) offer(zr[len - 1], len - 1);
    wave_argmax(bv, bi);
    if (lane == 0) {
        if (bv < 0.f) {  // empty or all-NaN row: see k_rows_argmax
            bv = (nan_empty && len > 0) ? __builtin_nanf("") : 0.f;
            bi = 0;
        }
        if (argmax) argmax[row] = bi;
        if (maxv) maxv[row] = use_normsq ? bv : sqrtf(bv);
    }
}

// Rows too long for one workgroup each (cp_fastXcorr at N = 1e7: three workgroups scanning 1e7 elements took 17 ms per
// launch): the row is cut into chunks, one workgroup per (chunk, row) leaves a packed key
//   (float bits of the maximum) << 32 | (0xFFFFFFFF - index)      (values >= 0: the bits order like the floats; 0 = none)
// and a second small kernel takes the largest key per row: same result as k_rows_argmax (first index on ties).
__global__ __launch_bounds__(256) void k_rows_argmax_part(const float2* __restrict__ z, int64_t len, int64_t chunk, float scale,
                                                          unsigned long long* __restrict__ part, float* __restrict__ plane) {
    __shared__ unsigned long long s_k[4];
    const int64_t row = blockIdx.y, c = blockIdx.x;
    const float2* zr = z + row * len;
    const int64_t lo = c * chunk, hi = min(len, lo + chunk);
    float bv = -1.f;
    uint32_t bi = 0;
    for (int64_t t = lo + threadIdx.x; t < hi; t += 256) {
        const float2 a = zr[t];
        const float v = (a.x * a.x + a.y * a.y) * scale;
        if (plane) plane[row * len + t] = v;
        if (v > bv) {
            bv = v;
            bi = (uint32_t)t;
        }
    }
    unsigned long long key = bv < 0.f ? 0ull : (((unsigned long long)__float_as_uint(bv)) << 32) | (0xFFFFFFFFu - bi);
    key = block_max(key, s_k);
    if (threadIdx.x == 0) part[row * gridDim.x + c] = key;
}
__global__ __launch_bounds__(64) void k_rows_argmax_fin(const unsigned long long* __restrict__ part, int32_t chunks,
                                                        int64_t rows, int32_t use_normsq, uint32_t* __restrict__ argmax,
                                                        float* __restrict__ maxv, int32_t nan_empty) {
    const int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (row >= rows) return;
    unsigned long long key = 0ull;
    for (int c = 0; c < chunks; ++c) {
        const unsigned long long k = part[row * chunks + c];
        key = k > key ? k : key;
    }
    const float bv = key ? __uint_as_float((uint32_t)(key >> 32)) : nan_empty ? __builtin_nanf("") : 0.f;  // empty / all-NaN row: (0, 0) or (NaN, 0)
    if (argmax) argmax[row] = key ? 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull) : 0u;
    if (maxv) maxv[row] = use_normsq ? bv : sqrtf(bv);
}

// findLocalMaxima (peakfinding.cu:14-58 predicate: above min_height and above both neighbours, zeros beyond the ends):
// ordered (ascending index) compaction that reads x ONCE.  Launch 1: a thread owns LM_PER consecutive samples
// (neighbours from the adjacent lanes), keeps its flags as a bit mask (n / 8 bytes of scratch) and the workgroup adds up
// the tile's count.  Launch 2 never touches x: a workgroup sums the counts of the tiles before its own (or reads the
// scanned counts when there are many tiles), ranks its masks with a workgroup scan and writes the indices; tiles
// without a maximum leave at once.  (A single-launch form with a ticketed look-back, scripts/ubench/tilescan_model.hip,
// costs more than this second launch: same-address tickets are served at ~10 ns each.)
constexpr int LM_NT = 1024, LM_PER = 16;
constexpr int LM_TILE = LM_NT * LM_PER;
constexpr int LM_DIRECT_TILES = 4096;  // up to here launch 2 adds the preceding counts itself (<= 16 KB per workgroup)

template <bool ALIGNED>
__global__ __launch_bounds__(LM_NT) void k_local_max_flags(const float* __restrict__ x, int64_t n, float min_height,
                                                           uint16_t* __restrict__ masks, int32_t* __restrict__ tile_count) {
    __shared__ int32_t s_w[LM_NT / 64];
    const int lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * LM_TILE + (int64_t)threadIdx.x * LM_PER;
    float v[LM_PER];
    if (ALIGNED && base + LM_PER <= n) {
#pragma unroll
        for (int j = 0; j < LM_PER; j += 4) {
            const float4 q = *reinterpret_cast<const float4*>(x + base + j);
            v[j] = q.x, v[j + 1] = q.y, v[j + 2] = q.z, v[j + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < LM_PER; ++j) v[j] = base + j < n ? x[base + j] : 0.f;
    }
    float left = __shfl_up(v[LM_PER - 1], 1, 64), right = __shfl_down(v[0], 1, 64);
    if (lane == 0) left = base > 0 && base - 1 < n ? x[base - 1] : 0.f;
    if (lane == 63) right = base + LM_PER < n ? x[base + LM_PER] : 0.f;
    uint32_t mask = 0;
#pragma unroll
    for (int j = 0; j < LM_PER; ++j) {
        const float l = j ? v[j - 1] : left, r = j + 1 < LM_PER ? v[j + 1] : right;
        if (base + j < n && v[j] > min_height && v[j] > l && v[j] > r) mask |= 1u << j;
    }
    masks[(int64_t)blockIdx.x * LM_NT + threadIdx.x] = (uint16_t)mask;
    const int t = block_sum((int32_t)__popc(mask), s_w);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = t;
}

// In place exclusive scan by one workgroup of 1024, a[n] = the total: the tile counts of the compactions (the local
// maxima here, the edges, the wavelet-matrix levels and the runs of caf_burst.hip).
template <typename T>
__global__ __launch_bounds__(1024) void k_scan_exclusive(T* __restrict__ a, int64_t n) {
    __shared__ T s_wave[16];
    __shared__ T s_base;
    if (threadIdx.x == 0) s_base = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t c0 = 0; c0 < n; c0 += 1024) {
        const int64_t t = c0 + threadIdx.x;
        const T v = t < n ? a[t] : 0;
        const T incl = wave_scan_inclusive(v, lane);
        const T off = s_base + block_exclusive(incl, v, lane, wave, s_wave);
        if (t < n) a[t] = off;
        __syncthreads();
        if (threadIdx.x == 1023) s_base = off + v;
        __syncthreads();
    }
    if (threadIdx.x == 0) a[n] = s_base;
}
template <typename T>
void launch_scan_exclusive(T* a, int64_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_scan_exclusive<T>, dim3(1), dim3(1024), 0, st, a, n);
}
template void launch_scan_exclusive<int32_t>(int32_t*, int64_t, hipStream_t);
template void launch_scan_exclusive<int64_t>(int64_t*, int64_t, hipStream_t);

__global__ __launch_bounds__(LM_NT) void k_local_max_write(const uint16_t* __restrict__ masks, const int32_t* __restrict__ tile_count,
                                                           int32_t scanned, int32_t max_out, int32_t* __restrict__ idx,
                                                           int32_t* __restrict__ count) {
    __shared__ int32_t s_w[LM_NT / 64];
    __shared__ int32_t s_before;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool last = blockIdx.x == gridDim.x - 1;
    int mine, before;
    if (scanned) {
        before = tile_count[blockIdx.x];
        mine = tile_count[blockIdx.x + 1] - before;
        if (last && threadIdx.x == 0) *count = before + mine;
        if (mine == 0) return;  // (uniform)
    } else {
        mine = tile_count[blockIdx.x];
        if (mine == 0 && !last) return;  // (uniform)
        int c = 0;
        for (int t = threadIdx.x; t < (int)blockIdx.x; t += LM_NT) c += tile_count[t];
        const int t = block_sum(c, s_w);
        if (threadIdx.x == 0) {
            s_before = t;
            if (last) *count = t + mine;
        }
        __syncthreads();
        before = s_before;
        if (mine == 0) return;
        __syncthreads();  // (s_w is reused below)
    }
    uint32_t mask = masks[(int64_t)blockIdx.x * LM_NT + threadIdx.x];
    const int c = __popc(mask);
    const int incl = wave_scan_inclusive(c, lane);
    int off = before + block_exclusive(incl, c, lane, wave, s_w);
    const int64_t base = (int64_t)blockIdx.x * LM_TILE + (int64_t)threadIdx.x * LM_PER;
    while (mask) {
        const int j = __ffs(mask) - 1;
        mask &= mask - 1;
        if (off < max_out) idx[off] = (int32_t)(base + j);
        ++off;
    }
}

// elementwise complex row-broadcast multiply: y[r][i] = x[r][i] * v[i]  (CZT pre/post chirps, spectra)
__global__ __launch_bounds__(256) void k_rows_mul_vec(const float2* __restrict__ x, int64_t in_pitch, int64_t in_off,
                                                      const float2* __restrict__ v, int64_t len,
                                                      float2* __restrict__ y, int64_t out_pitch, int64_t pad_to,
                                                      float scale) {
    const int64_t r = blockIdx.y;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pad_to; i += (int64_t)gridDim.x * 256) {
        float2 o = make_float2(0.f, 0.f);
        if (i < len) {
            const float2 a = x[r * in_pitch + in_off + i], b = v[i];
            o = make_float2((a.x * b.x - a.y * b.y) * scale, (a.x * b.y + a.y * b.x) * scale);
        }
        y[r * out_pitch + i] = o;
    }
}

__global__ __launch_bounds__(256) void k_scale(float2* __restrict__ y, int64_t n, float scale) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        float2 v = y[i];
        y[i] = make_float2(v.x * scale, v.y * scale);
    }
}

// ---- engine add-on: complex QF output (the across-template maximum: caf_reduce.hip) -------
// cqf[h][i] = P[h][i] * sqrt(tscale[t] * inv_e[i])   (TemplateCrossCorrelator layout, xcorrRoutines.py:352-357)
__global__ __launch_bounds__(256) void k_complex_norm(const float2* __restrict__ pbuf, int32_t pitch, int32_t nfreq,
                                                      const float* __restrict__ tscale,
                                                      const float* __restrict__ inv_e, int64_t num_shifts,
                                                      int32_t step, int32_t blk0, int32_t nhyp,
                                                      float2* __restrict__ cqf) {
    const int z = blockIdx.z, h = blockIdx.y;
    const int blk = blk0 + z;
    const int sl = blockIdx.x * 256 + threadIdx.x;
    const int64_t rel = (int64_t)blk * step + sl;
    if (sl >= step || rel >= num_shifts) return;
    const float2 p = pbuf[((int64_t)z * nhyp + h) * pitch + sl];
    const float g = sqrtf(tscale[h / nfreq]) * sqrtf(inv_e[rel]);
    cqf[(int64_t)h * num_shifts + rel] = make_float2(p.x * g, p.y * g);
}

// ---------------------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------------------
void launch_sliding_multiply(const float2* x, int32_t xlen, const float2* y, int64_t ylen, const double* prefix,
                             int64_t start, int64_t step, int64_t rows, double coef, int32_t zero_oor, float2* z,
                             hipStream_t st, const double* d_coef) {
    // rows of up to 8192 samples: ~64K elements per workgroup (up to 64 rows), one chunk; longer rows: one row per
    // workgroup row, up to 64 chunks
    int rpw = 1;
    int rows_fastest = 0;
    unsigned gx = std::min<unsigned>(cdiv(xlen, 256), 64);
    if (xlen > 8192 && rows >= 4) {
        rows_fastest = 1;
        // long rows: four rows per workgroup (one x load for the four), enough chunks to fill the chip
        rpw = 4;
        const int64_t groups = (rows + 3) / 4;
        gx = (unsigned)std::min<int64_t>(cdiv(xlen, 1024), std::max<int64_t>(64, 4096 / groups));
    }
    if (xlen <= 8192) {
        rpw = (int)std::max<int64_t>(1, std::min<int64_t>(SM_MAX_RPW, 65536 / std::max(xlen, 1)));
        // keep at least ~2048 workgroups in flight when there are that many rows
        while (rpw > 1 && (rows + rpw - 1) / rpw < 2048) rpw >>= 1;
        if (rpw > 1) gx = 1;
    }
    const int64_t rows_per_launch = (int64_t)65535 * rpw;
    for (int64_t r0 = 0; r0 < rows; r0 += rows_per_launch) {
        const int64_t nr = std::min<int64_t>(rows_per_launch, rows - r0);
        const unsigned gy = (unsigned)((nr + rpw - 1) / rpw);
        hipLaunchKernelGGL(k_sliding_multiply, rows_fastest ? dim3(gy, gx) : dim3(gx, gy), dim3(256), 0, st, x, xlen, y, ylen,
                           prefix, start + r0 * step, step, coef, zero_oor, z + r0 * (int64_t)xlen, d_coef, nr, rpw, rows_fastest);
    }
}

int rows_argmax_chunks(int64_t rows, int64_t len) {
    // one workgroup per row is fine while there are enough rows to fill the chip or the rows are short
    if (len <= 131072 || rows >= 2048) return 0;
    return (int)std::min<int64_t>(1024, (len + 32767) / 32768);
}

void launch_rows_argmax(const float2* z, int64_t rows, int64_t len, int32_t use_normsq, float scale, uint32_t* argmax,
                        float* maxv, float* plane, hipStream_t st, unsigned long long* part, int32_t nan_empty) {
    if (rows <= 0) return;
    const int chunks = part ? rows_argmax_chunks(rows, len) : 0;
    if (chunks > 1) {
        const int64_t chunk = ((len + chunks - 1) / chunks + 255) / 256 * 256;
        hipLaunchKernelGGL(k_rows_argmax_part, dim3((unsigned)chunks, (unsigned)rows), dim3(256), 0, st, z, len, chunk, scale, part,
                           plane);
        hipLaunchKernelGGL(k_rows_argmax_fin, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, st, part, chunks, rows, use_normsq,
                           argmax, maxv, nan_empty);
        return;
    }
    if (rows >= 1024 && len <= 32768) {
        hipLaunchKernelGGL(k_rows_argmax_wave, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, z, rows, len, use_normsq, scale,
                           argmax, maxv, plane, nan_empty);
        return;
    }
    hipLaunchKernelGGL(k_rows_argmax, dim3((unsigned)rows), dim3(256), 0, st, z, len, use_normsq, scale, argmax, maxv,
                       plane, nan_empty);
}

// scratch: the tile counts (+ the total) followed by one 16-bit mask per thread of launch 1
int64_t local_maxima_scratch_ints(int64_t n) {
    const int64_t ntiles = (n + LM_TILE - 1) / LM_TILE;
    return ((ntiles + 1 + 3) & ~(int64_t)3) + ntiles * LM_NT / 2;
}

void launch_find_local_maxima(const float* x, int64_t n, float min_height, int32_t* tile_scratch, int32_t max_out,
                              int32_t* idx, int32_t* count, hipStream_t st) {
    const int64_t ntiles = (n + LM_TILE - 1) / LM_TILE;
    uint16_t* masks = reinterpret_cast<uint16_t*>(tile_scratch + ((ntiles + 1 + 3) & ~(int64_t)3));
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0)
        hipLaunchKernelGGL(k_local_max_flags<true>, dim3((unsigned)ntiles), dim3(LM_NT), 0, st, x, n, min_height, masks, tile_scratch);
    else
        hipLaunchKernelGGL(k_local_max_flags<false>, dim3((unsigned)ntiles), dim3(LM_NT), 0, st, x, n, min_height, masks,
                           tile_scratch);
    const int scanned = ntiles > LM_DIRECT_TILES;
    if (scanned) launch_scan_exclusive(tile_scratch, ntiles, st);
    hipLaunchKernelGGL(k_local_max_write, dim3((unsigned)ntiles), dim3(LM_NT), 0, st, masks, tile_scratch, scanned, max_out, idx,
                       count);
}

void launch_rows_mul_vec(const float2* x, int64_t in_pitch, int64_t in_off, const float2* v, int64_t len, float2* y,
                         int64_t out_pitch, int64_t pad_to, int64_t rows, float scale, hipStream_t st) {
    const unsigned gx = std::min<unsigned>(cdiv(pad_to, 256), 256);
    for (int64_t r0 = 0; r0 < rows; r0 += 65535) {
        const int64_t nr = std::min<int64_t>(65535, rows - r0);
        hipLaunchKernelGGL(k_rows_mul_vec, dim3(gx, (unsigned)nr), dim3(256), 0, st, x + r0 * in_pitch, in_pitch, in_off, v,
                           len, y + r0 * out_pitch, out_pitch, pad_to, scale);
    }
}

void launch_complex_norm(const float2* pbuf, int32_t pitch, int32_t nfreq, const float* tscale, const float* inv_e,
                         int64_t num_shifts, int32_t step, int32_t blk0, int32_t nblk, int32_t nhyp, float2* cqf,
                         hipStream_t st) {
    hipLaunchKernelGGL(k_complex_norm, dim3(cdiv(step, 256), nhyp, nblk), dim3(256), 0, st, pbuf, pitch, nfreq, tscale,
                       inv_e, num_shifts, step, blk0, nhyp, cqf);
}

void launch_scale(float2* y, int64_t n, float scale, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_scale, dim3(std::min<unsigned>(cdiv(n, 256), 4096)), dim3(256), 0, st, y, n, scale);
}

}  // namespace caf

using namespace caf;

int32_t caf_sliding_multiply_normalised(const float* d_x, int32_t xlen, const float* d_y, int64_t ylen,
                                        int64_t start_idx, int64_t idxlen, double coefficient, float* d_z,
                                        void* stream) {
    CAF_REQUIRE(d_x && d_y && d_z && xlen >= 1 && ylen >= 1, "caf_sliding_multiply_normalised: bad arguments");
    CAF_REQUIRE(start_idx >= 0 && idxlen >= 0 && start_idx + idxlen <= ylen,
                "startIdx and idxlen should be within the bounds of d_y.");
    if (idxlen == 0) return CAF_OK;
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st, true);
    double* prefix = nullptr;
    int rc = energy_prefix((const float2*)d_y, ylen, sc, &prefix, st);
    if (rc) return rc;
    launch_sliding_multiply((const float2*)d_x, xlen, (const float2*)d_y, ylen, prefix, start_idx, 1, idxlen, coefficient,
                            0, (float2*)d_z, st);
    return sc.finish();
}

int32_t caf_argmax_abs_rows(const float* d_x, int64_t rows, int64_t len, uint32_t* d_argmax, float* d_max,
                            int32_t use_normsq, void* stream) {
    CAF_REQUIRE(d_x && d_argmax && rows >= 0 && len >= 1, "caf_argmax_abs_rows: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    unsigned long long* part = nullptr;
    const int ch = rows > 0 ? rows_argmax_chunks(rows, len) : 0;
    if (ch) {
        const int rc = sc.get(&part, rows * ch);
        if (rc) return rc;
    }
    for (int64_t r0 = 0; r0 < rows; r0 += ((int64_t)1 << 30))
        launch_rows_argmax((const float2*)d_x + r0 * len, std::min<int64_t>(rows - r0, (int64_t)1 << 30), len, use_normsq,
                           1.0f, d_argmax + r0, d_max ? d_max + r0 : nullptr, nullptr, st, part ? part + r0 * ch : nullptr);
    return sc.finish();
}

int32_t caf_find_local_maxima(const float* d_x, int64_t n, float min_height, int32_t max_peaks, int32_t* d_peak_index,
                              int32_t* d_count, void* stream) {
    CAF_REQUIRE(d_x && d_peak_index && d_count && n >= 1 && max_peaks >= 1, "caf_find_local_maxima: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st, true);
    int32_t* tiles = nullptr;
    int rc = sc.get(&tiles, local_maxima_scratch_ints(n));
    if (rc) return rc;
    launch_find_local_maxima(d_x, n, min_height, tiles, max_peaks, d_peak_index, d_count, st);
    return sc.finish();
}
