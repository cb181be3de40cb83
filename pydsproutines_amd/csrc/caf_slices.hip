// gfx950 slice kernels of the stand-alone toolbox with their entry points: sliding dot products against several templates,
// products and copies of slices, gathers.  CDNA4 counterparts -- by semantics, not by code -- of the reference's
//   custom_kernels/multiplySlices.cu:251-399  multiTemplateSlidingDotProduct
//   custom_kernels/multiplySlices.cu:25-84    multiplySlicesWithIndexedRowsOptimistic
//   custom_kernels/copying.cu:8-138, cupyExtensions.py:17-38   slice/group copies
// All are HBM-bound elementwise / sliding-window work.
#include <algorithm>

#include "caf_internal.h"
#include "caf_energy.h"
#include "caf_stage.h"
#include "caf_wave.h"

namespace caf {

// ---------------------------------------------------------------------------------------
// multiTemplateSlidingDotProduct: per slide k, best template i of
//   |sum_t T_i[t] x[k+t]|^2 / E_i / ||x[k:k+L]||^2   (first template wins ties; all-zero -> (0, 0)).
// One workgroup owns MT_SLIDES consecutive slides; the x section and one template at a time live in
// LDS; each wave computes whole dot products (lanes stride over t, shuffle reduce), so no block-wide
// barrier per slide as in the reference.
// ---------------------------------------------------------------------------------------
constexpr int MT_SLIDES = 64;

// 1 / ||x[s : s+L]||^2 of a slide: the energy from window_energy (caf_energy.h: the prefix difference where it is resolved,
// the direct sum where it is not -- a window behind a louder stretch of the record), float64 up to and including the one
// division.  A window without energy gives 0, so that every template scores 0 and the slide reports (0, 0.0): the
// reference's all-zero column.
__device__ __forceinline__ float mt_inv_energy(const double* __restrict__ prefix, const float2* __restrict__ x, int64_t xlen,
                                               int64_t s, int32_t L) {
    int64_t e1 = s + L;
    if (e1 > xlen) e1 = xlen;
    const double e = window_energy(prefix, x, xlen, s, e1);
    return e > 0.0 ? (float)(1.0 / e) : 0.f;
}

__global__ __launch_bounds__(256) void k_multi_template_dot(const float2* __restrict__ tm, const float* __restrict__ te,
                                                            int32_t ntm, int32_t L, const float2* __restrict__ x,
                                                            int64_t xlen, const double* __restrict__ prefix,
                                                            int64_t start, int64_t nslides, int32_t* __restrict__ tidx,
                                                            float* __restrict__ qf2) {
    extern __shared__ float2 s_mem[];
    float2* s_t = s_mem;          // L
    float2* s_xs = s_mem + L;     // MT_SLIDES + L - 1
    const int64_t k0 = (int64_t)blockIdx.x * MT_SLIDES;
    const int span = MT_SLIDES + L - 1;
    stage_batched<8>(span, [&](int t) { const int64_t j = start + k0 + t; return (j < xlen) ? x[j] : make_float2(0.f, 0.f); },
                     [&](int t, float2 v) { s_xs[t] = v; });
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int PER_WAVE = MT_SLIDES / 4;
    float bv[PER_WAVE], ie[PER_WAVE];  // ie: 1 / ||x[k:k+L]||^2 per slide (mt_inv_energy)
    int32_t bi[PER_WAVE];
#pragma unroll
    for (int r = 0; r < PER_WAVE; ++r) {
        const int64_t k = k0 + wave * PER_WAVE + r;
        ie[r] = k < nslides ? mt_inv_energy(prefix, x, xlen, start + k, L) : 0.f;
        bv[r] = 0.f;
        bi[r] = 0;
    }
    for (int i = 0; i < ntm; ++i) {
        __syncthreads();
        for (int t = threadIdx.x; t < L; t += 256) s_t[t] = tm[(int64_t)i * L + t];
        __syncthreads();
        const float inv_te = 1.0f / te[i];
#pragma unroll
        for (int r = 0; r < PER_WAVE; ++r) {
            const int k = wave * PER_WAVE + r;
            if (k0 + k >= nslides) break;
            float ar = 0.f, ai = 0.f;
            for (int t = lane; t < L; t += 64) {
                const float2 a = s_t[t], b = s_xs[k + t];
                ar += a.x * b.x - a.y * b.y;
                ai += a.x * b.y + a.y * b.x;
            }
            ar = wave_sum(ar);
            ai = wave_sum(ai);
            const float v = (ar * ar + ai * ai) * inv_te * ie[r];
            if (v > bv[r]) {
                bv[r] = v;
                bi[r] = i;
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < PER_WAVE; ++r) {
            const int64_t k = k0 + wave * PER_WAVE + r;
            if (k < nslides) {
                tidx[k] = bi[r];
                qf2[k] = bv[r];
            }
        }
    }
}

// Register-tiled form of the above for templates up to MTR_MAXL samples: a thread owns MTR_R consecutive slides and
// keeps their MTR_R-sample window of x in registers (it slides by one sample per template tap; the tap loop is
// unrolled by MTR_R so that the window rotates through fixed register names), so a tap costs one LDS sample read
// and one broadcast tap read for MTR_R complex MACs, where the kernel above reads both operands per MAC and
// shuffle-reduces every dot product.  x window stored transposed (e % MTR_R major) as in k_fir_fast; templates
// zero-padded to a multiple of MTR_R.
constexpr int MTR_R = 8;
constexpr int MTR_SLIDES = 256 * MTR_R;
constexpr int MTR_MAXL = 2048;

__global__ __launch_bounds__(256) void k_multi_template_dot_rt(const float2* __restrict__ tm, const float* __restrict__ te,
                                                               int32_t ntm, int32_t L, const float2* __restrict__ x,
                                                               int64_t xlen, const double* __restrict__ prefix,
                                                               int64_t start, int64_t nslides,
                                                               int32_t* __restrict__ tidx, float* __restrict__ qf2) {
    extern __shared__ float2 s_mtr[];
    const int Lp = (L + MTR_R - 1) / MTR_R * MTR_R;
    const int span = MTR_SLIDES + Lp;
    const int pitch = span / MTR_R + 1;
    float2* s_t = s_mtr;        // Lp
    float2* s_xs = s_mtr + Lp;  // MTR_R rows of `pitch`
    const int64_t k0 = (int64_t)blockIdx.x * MTR_SLIDES;
    stage_batched<8>(span, [&](int t) { const int64_t j = start + k0 + t; return (j < xlen) ? x[j] : make_float2(0.f, 0.f); },
                     [&](int t, float2 v) { s_xs[(t % MTR_R) * pitch + t / MTR_R] = v; });
    const int l0 = threadIdx.x * MTR_R;
    float ie[MTR_R], bv[MTR_R];  // ie: 1 / ||x[k:k+L]||^2 per slide (mt_inv_energy; 0 for slides past the end)
    int32_t bi[MTR_R];
#pragma unroll
    for (int r = 0; r < MTR_R; ++r) {
        ie[r] = k0 + l0 + r < nslides ? mt_inv_energy(prefix, x, xlen, start + k0 + l0 + r, L) : 0.f;
        bv[r] = 0.f;
        bi[r] = 0;
    }
    for (int i = 0; i < ntm; ++i) {
        __syncthreads();  // previous template consumed (and, first time, the x window written)
        for (int t = threadIdx.x; t < Lp; t += 256) s_t[t] = t < L ? tm[(int64_t)i * L + t] : make_float2(0.f, 0.f);
        __syncthreads();
        float2 acc[MTR_R], win[MTR_R];
#pragma unroll
        for (int r = 0; r < MTR_R; ++r) {
            acc[r] = make_float2(0.f, 0.f);
            win[r] = s_xs[r * pitch + threadIdx.x];  // e = l0 + r
        }
        for (int t0 = 0; t0 < Lp; t0 += MTR_R) {
#pragma unroll
            for (int tt = 0; tt < MTR_R; ++tt) {
                const float2 a = s_t[t0 + tt];
                // slide r at tap t reads sample l0 + r + t, held in slot (r + tt) mod R
#pragma unroll
                for (int r = 0; r < MTR_R; ++r) {
                    const float2 b = win[(r + tt) % MTR_R];
                    acc[r].x += a.x * b.x - a.y * b.y;
                    acc[r].y += a.x * b.y + a.y * b.x;
                }
                // sample l0 + t is done; slot tt takes l0 + t + R  (row tt, column tid + (t0 + R) / R)
                win[tt] = s_xs[tt * pitch + threadIdx.x + t0 / MTR_R + 1];
            }
        }
        const float inv_te = 1.0f / te[i];
#pragma unroll
        for (int r = 0; r < MTR_R; ++r) {
            const float v = (acc[r].x * acc[r].x + acc[r].y * acc[r].y) * inv_te * ie[r];
            if (v > bv[r]) {
                bv[r] = v;
                bi[r] = i;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < MTR_R; ++r) {
        const int64_t k = k0 + l0 + r;
        if (k < nslides) {
            tidx[k] = bi[r];
            qf2[k] = bv[r];
        }
    }
}

// out[i][t] = rows[row_idx[i]][t] * x[slice_start[i] + t] for t < slice_lens[i] (0 beyond), t < slice_len
__global__ __launch_bounds__(256) void k_multiply_indexed_rows(const float2* __restrict__ x, int64_t xlen,
                                                               const float2* __restrict__ rows, int32_t row_len,
                                                               const int32_t* __restrict__ slice_start,
                                                               const int32_t* __restrict__ slice_lens,
                                                               const int32_t* __restrict__ row_idx, int32_t slice_len,
                                                               float2* __restrict__ out) {
    const int64_t i = blockIdx.y;
    const float2* r = rows + (int64_t)row_idx[i] * row_len;
    const int64_t s0 = slice_start[i];
    const int li = slice_lens ? min(slice_lens[i], row_len) : min(slice_len, row_len);
    for (int t = blockIdx.x * 256 + threadIdx.x; t < slice_len; t += gridDim.x * 256) {
        const int64_t j = s0 + t;
        float2 v = make_float2(0.f, 0.f);
        if (t < li && j >= 0 && j < xlen) {
            const float2 a = r[t], b = x[j];
            v = make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
        }
        out[i * slice_len + t] = v;
    }
}

// generic gather of equal-length slices: out[i][t] = x[starts[i] + t]  (or start0 + i*inc when starts == NULL)
// starts_stride = 2 reads the start column of an (N, 2) [start, end) bounds array and limits row i to end-start.
__global__ __launch_bounds__(256) void k_copy_slices(const float2* __restrict__ x, int64_t xlen,
                                                     const int32_t* __restrict__ starts, int32_t starts_stride,
                                                     int64_t start0, int64_t inc, int32_t len,
                                                     float2* __restrict__ out) {
    const int64_t i = blockIdx.y;
    const int64_t s0 = starts ? (int64_t)starts[i * starts_stride] : start0 + i * inc;
    const int li = (starts && starts_stride == 2) ? min(len, starts[i * 2 + 1] - starts[i * 2]) : len;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < len; t += gridDim.x * 256) {
        const int64_t j = s0 + t;
        out[i * len + t] = (t < li && j >= 0 && j < xlen) ? x[j] : make_float2(0.f, 0.f);
    }
}

// copy groups: y[ys[b] + i] = x[xs[b] + i], i < len[b]   (cupyExtensions.py:17-38)
__global__ __launch_bounds__(256) void k_copy_groups(const float2* __restrict__ x, float2* __restrict__ y,
                                                     const int32_t* __restrict__ xs, const int32_t* __restrict__ ys,
                                                     const int32_t* __restrict__ lens) {
    const int b = blockIdx.x;
    const int64_t xo = xs[b], yo = ys[b];
    for (int i = threadIdx.x; i < lens[b]; i += 256) y[yo + i] = x[xo + i];
}

// out[i] = x[idx[i]] for 4-byte elements (values / arguments of the candidate peaks without copying whole traces)
__global__ __launch_bounds__(256) void k_gather_b32(const uint32_t* __restrict__ x, int64_t xlen,
                                                    const int32_t* __restrict__ idx, int64_t n,
                                                    uint32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t j = idx[i];
    out[i] = (j >= 0 && j < xlen) ? x[j] : 0u;
}

// out[i] = (double) x[idx ? idx[i] : i]: float32 traces into the float64 device arrays the reference's GPU entry
// points return (xc = cp.zeros(shifts.size), xcorrRoutines.py:1198-1203) without a host round trip
__global__ __launch_bounds__(256) void k_gather_f32_f64(const float* __restrict__ x, int64_t xlen,
                                                        const int32_t* __restrict__ idx, int64_t n,
                                                        double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t j = idx ? (int64_t)idx[i] : i;
    out[i] = (j >= 0 && j < xlen) ? (double)x[j] : 0.0;
}

static void launch_multi_template_dot(const float2* tm, const float* te, int32_t ntm, int32_t L, const float2* x, int64_t xlen,
                               const double* prefix, int64_t start, int64_t nslides, int32_t* tidx, float* qf2,
                               hipStream_t st) {
    const int Lp = (L + MTR_R - 1) / MTR_R * MTR_R;
    if (Lp <= MTR_MAXL) {
        const int span = MTR_SLIDES + Lp;
        const size_t smr = (size_t)(Lp + MTR_R * (span / MTR_R + 1)) * sizeof(float2);
        hipLaunchKernelGGL(k_multi_template_dot_rt, dim3(cdiv(nslides, MTR_SLIDES)), dim3(256), smr, st, tm, te, ntm, L, x,
                           xlen, prefix, start, nslides, tidx, qf2);
        return;
    }
    const size_t sm = (size_t)(2 * L + MT_SLIDES) * sizeof(float2);
    hipLaunchKernelGGL(k_multi_template_dot, dim3(cdiv(nslides, MT_SLIDES)), dim3(256), sm, st, tm, te, ntm, L, x, xlen,
                       prefix, start, nslides, tidx, qf2);
}

}  // namespace caf

using namespace caf;

int32_t caf_multi_template_sliding_dot(const float* d_templates, const float* d_energies, int32_t num_templates,
                                       int32_t template_len, const float* d_x, int64_t xlen, int64_t start_idx,
                                       int64_t idxlen, int32_t* d_template_idx, float* d_qf2, void* stream) {
    CAF_REQUIRE(d_templates && d_energies && d_x && d_template_idx && d_qf2, "caf_multi_template_sliding_dot: NULL");
    CAF_REQUIRE(num_templates >= 1 && template_len >= 1, "need >= 1 template");
    CAF_REQUIRE(template_len <= 8192, "template too long for the LDS-resident kernel (use the hypothesis engine)");
    CAF_REQUIRE(start_idx >= 0 && idxlen >= 0 && start_idx + idxlen - 1 + template_len - 1 < xlen,
                "final slide index should be within the bounds of d_x");
    if (idxlen == 0) return CAF_OK;
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st, true);
    double* prefix = nullptr;
    int rc = energy_prefix((const float2*)d_x, xlen, sc, &prefix, st);
    if (rc) return rc;
    launch_multi_template_dot((const float2*)d_templates, d_energies, num_templates, template_len, (const float2*)d_x,
                              xlen, prefix, start_idx, idxlen, d_template_idx, d_qf2, st);
    return sc.finish();
}

int32_t caf_multiply_slices_indexed_rows(const float* d_x, int64_t xlen, const float* d_rows, int32_t num_rows,
                                         int32_t row_len, const int32_t* d_slice_starts, const int32_t* d_slice_lens,
                                         const int32_t* d_row_idx, int32_t out_len, int64_t num_slices, float* d_out,
                                         void* stream) {
    CAF_REQUIRE(d_x && d_rows && d_slice_starts && d_row_idx && d_out, "caf_multiply_slices_indexed_rows: NULL");
    CAF_REQUIRE(out_len >= 1 && num_rows >= 1 && num_slices >= 0, "bad slice/row lengths");
    hipStream_t st = (hipStream_t)stream;
    const unsigned gx = std::min<unsigned>(cdiv(out_len, 256), 64);
    for (int64_t r0 = 0; r0 < num_slices; r0 += 65535) {
        const int64_t nr = std::min<int64_t>(65535, num_slices - r0);
        hipLaunchKernelGGL(k_multiply_indexed_rows, dim3(gx, (unsigned)nr), dim3(256), 0, st, (const float2*)d_x, xlen,
                           (const float2*)d_rows, row_len, d_slice_starts + r0, d_slice_lens ? d_slice_lens + r0 : nullptr,
                           d_row_idx + r0, out_len, (float2*)d_out + r0 * (int64_t)out_len);
    }
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_copy_slices_to_matrix(const float* d_x, int64_t xlen, const int32_t* d_starts, int32_t starts_stride,
                                  int64_t start0, int64_t increment, int32_t len, int64_t rows, float* d_out,
                                  void* stream) {
    CAF_REQUIRE(d_x && d_out && len >= 1 && rows >= 0, "caf_copy_slices_to_matrix: bad arguments");
    CAF_REQUIRE(!d_starts || starts_stride == 1 || starts_stride == 2, "starts_stride must be 1 or 2");
    hipStream_t st = (hipStream_t)stream;
    const unsigned gx = std::min<unsigned>(cdiv(len, 256), 64);
    for (int64_t r0 = 0; r0 < rows; r0 += 65535) {
        const int64_t nr = std::min<int64_t>(65535, rows - r0);
        hipLaunchKernelGGL(k_copy_slices, dim3(gx, (unsigned)nr), dim3(256), 0, st, (const float2*)d_x, xlen,
                           d_starts ? d_starts + r0 * starts_stride : nullptr, starts_stride, start0 + r0 * increment, increment,
                           len, (float2*)d_out + r0 * (int64_t)len);
    }
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_copy_groups(const float* d_x, float* d_y, const int32_t* d_x_starts, const int32_t* d_y_starts,
                        const int32_t* d_lengths, int32_t num_groups, void* stream) {
    CAF_REQUIRE(d_x && d_y && d_x_starts && d_y_starts && d_lengths && num_groups >= 0, "caf_copy_groups: bad arguments");
    if (num_groups > 0)
        hipLaunchKernelGGL(k_copy_groups, dim3(num_groups), dim3(256), 0, (hipStream_t)stream, (const float2*)d_x, (float2*)d_y,
                           d_x_starts, d_y_starts, d_lengths);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_gather_b32(const void* d_x, int64_t xlen, const int32_t* d_index, int64_t n, void* d_out, void* stream) {
    CAF_REQUIRE(d_x && d_index && d_out && xlen >= 1 && n >= 0, "caf_gather_b32: bad arguments");
    if (n > 0)
        hipLaunchKernelGGL(k_gather_b32, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)d_x, xlen, d_index,
                           n, (uint32_t*)d_out);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_gather_f32_f64(const float* d_x, int64_t xlen, const int32_t* d_index, int64_t n, double* d_out, void* stream) {
    CAF_REQUIRE(d_x && d_out && xlen >= 1 && n >= 0, "caf_gather_f32_f64: bad arguments");
    if (n > 0)
        hipLaunchKernelGGL(k_gather_f32_f64, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, d_x, xlen, d_index, n, d_out);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}
