// gfx950 kernels of the steps after the correlation peak, with their entry points: coherent sums of per-delay planes, the
// sub-sample refinement and the tone-dot zoom.  CDNA4 counterparts -- by semantics, not by code -- of the reference's
//   xcorrRoutines.py:1454-1484, 1549-1585     GroupXcorrCZT_Permutations.getCAF
//   xcorrRoutines.py:996-1039, GroupXcorrCZT.cpp:106-329   GroupXcorrCZT.xcorr
//   xcorrRoutines.py:583-719                  fineFreqTimeSearch / GenXcorr
//   custom_kernels/genTones.cu:165-283        dotTonesScaling_32f
#include <algorithm>

#include "caf_internal.h"
#include "caf_wave.h"

namespace caf {

// Combination step of GroupXcorrCZT_Permutations.getCAF (xcorrRoutines.py:1454-1484, 1549-1585):
// out[i][k] = | sum_j planes[idx[j]][i][k] |^2 / (row_norm[i] * ynormsq), complex64 planes of rows x cols
constexpr int SUMPL_MAX = 64;
struct SumPlanesIdx {
    int32_t v[SUMPL_MAX];
};
__global__ __launch_bounds__(256) void k_sum_planes_qf2(const float2* __restrict__ planes, int64_t plane_elems,
                                                        int32_t cols, SumPlanesIdx idx, int32_t nsel,
                                                        const double* __restrict__ row_norm, double ynormsq,
                                                        double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < plane_elems; e += stride) {
        float2 acc = make_float2(0.f, 0.f);
        for (int j = 0; j < nsel; ++j) {
            const float2 v = planes[(int64_t)idx.v[j] * plane_elems + e];
            acc.x += v.x;
            acc.y += v.y;
        }
        const float m = acc.x * acc.x + acc.y * acc.y;  // cp.abs(complex64)**2 is float32 upstream
        out[e] = (double)m / row_norm[e / cols] / ynormsq;
    }
}

// Coherent sum over the GROUPS of a composite template on the per-delay path (GroupXcorrCZT.xcorr, xcorrRoutines.py:996-1039;
// GroupXcorrCZT.cpp:106-329): planes[g][row][col] = the chirp-Z transform of group g's product row at delay `row`, evaluated
// as if the group began at sample 0; phase[g][col] = e^{-j 2 pi f_col start_g / fs} moves it to where the group lies.
//   out[row][col] = | sum_g phase[g][col] planes[g][row][col] |^2 / row_norm[row] / ynormsq
// (float32 products and sum like the upstream complex64 arithmetic, float64 normalisation).  Any number of groups.
__global__ __launch_bounds__(256) void k_sum_groups_qf2(const float2* __restrict__ planes, int32_t ngroups, int64_t plane_elems,
                                                        int32_t cols, const float2* __restrict__ phase,
                                                        const double* __restrict__ row_norm, double ynormsq,
                                                        double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < plane_elems; e += stride) {
        const int64_t row = e / cols;
        const int col = (int)(e - row * cols);
        float2 acc = make_float2(0.f, 0.f);
        for (int g = 0; g < ngroups; ++g) {
            const float2 v = planes[(int64_t)g * plane_elems + e];
            const float2 p = phase ? phase[(int64_t)g * cols + col] : make_float2(1.f, 0.f);
            acc.x += v.x * p.x - v.y * p.y;
            acc.y += v.x * p.y + v.y * p.x;
        }
        const float m = acc.x * acc.x + acc.y * acc.y;
        out[e] = (double)m / row_norm[row] / ynormsq;
    }
}

// Sub-sample refinement after the peak (fineFreqTimeSearch / GenXcorr, xcorrRoutines.py:583-719):
//   k_mul_conj : out[i] = a[i] * conj(b[i])                       (x_fft * y_fft.conj(), y.conj() * x, masks)
//   k_steer_dot: out[r] = scale * sum_k vec[k] * conj(steer[r][k]) (np.dot(rx_vec, steeringvec.conj().T), np.vdot)
// The steering matrix is complex128 as upstream (phases 2 pi f tau need the precision); products and the sum
// are float64, the vector is the complex64 the device FFT produced.
__global__ __launch_bounds__(256) void k_mul_conj(const float2* __restrict__ a, const float2* __restrict__ b, int64_t n,
                                                  float2* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float2 x = a[i], y = b[i];
        out[i] = make_float2(x.x * y.x + x.y * y.y, x.y * y.x - x.x * y.y);
    }
}

__global__ __launch_bounds__(256) void k_steer_dot(const float2* __restrict__ vec, const double2* __restrict__ steer,
                                                   int64_t n, double scale, double2* __restrict__ out) {
    __shared__ WaveSlots<4, double, double> s_sum;
    const double2* row = steer + (int64_t)blockIdx.x * n;
    double re = 0.0, im = 0.0;
    for (int64_t k = threadIdx.x; k < n; k += 256) {
        const float2 v = vec[k];
        const double2 s = row[k];
        re += (double)v.x * s.x + (double)v.y * s.y;  // v * conj(s)
        im += (double)v.y * s.x - (double)v.x * s.y;
    }
    block_sum(s_sum, re, im);
    if (threadIdx.x == 0) out[blockIdx.x] = make_double2(scale * re, scale * im);
}

// Tone-dot zoom (dotTonesScaling_32f, genTones.cu:165-283; cupyDotTonesScaling, spectralRoutines.py:580-630):
//   out[b][k] = sum_{i in 64-sample block b} src[i] * exp(j 2 pi (f0 + k fstep) i),  k < num_freqs
// One wave per block.  Every lane carries src[i] * tone and steps it by exp(j 2 pi fstep i) (complex64, as
// upstream), re-anchored with a float64 sincospi at every batch of 64 frequencies (upstream lets the float
// recurrence run over all frequencies); a 64 x 65 LDS patch turns 64 frequencies x 64 samples into row sums.
__global__ __launch_bounds__(64) void k_dot_tones(double f0, double fstep, int32_t num_freqs, int64_t len,
                                                  const float2* __restrict__ src, float2* __restrict__ out) {
    __shared__ float2 s_ws[64 * 65];
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 64 + lane;
    const float2 v = i < len ? src[i] : make_float2(0.f, 0.f);
    double sr, cr;
    {
        double t = fstep * (double)i;
        t -= floor(t);  // whole cycles do not matter; keeps the argument of sincospi small
        sincospi(2.0 * t, &sr, &cr);
    }
    const float2 alpha = make_float2((float)cr, (float)sr);
    for (int k0 = 0; k0 < num_freqs; k0 += 64) {
        double t = (f0 + (double)k0 * fstep) * (double)i;
        t -= floor(t);
        sincospi(2.0 * t, &sr, &cr);
        float2 cur = make_float2(v.x * (float)cr - v.y * (float)sr, v.x * (float)sr + v.y * (float)cr);
        const int nk = min(64, num_freqs - k0);
        for (int r = 0; r < nk; ++r) {
            s_ws[r * 65 + lane] = cur;
            cur = make_float2(cur.x * alpha.x - cur.y * alpha.y, cur.x * alpha.y + cur.y * alpha.x);
        }
        __builtin_amdgcn_wave_barrier();  // one wave: LDS operations execute in order
        if (lane < nk) {
            float2 acc = make_float2(0.f, 0.f);
#pragma unroll 8
            for (int c = 0; c < 64; ++c) {
                const float2 w = s_ws[lane * 65 + c];
                acc.x += w.x;
                acc.y += w.y;
            }
            out[(int64_t)blockIdx.x * num_freqs + k0 + lane] = acc;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace caf

using namespace caf;

int32_t caf_dot_tones(const float* d_src, int64_t len, double f0, double fstep, int32_t num_freqs, float* d_out,
                      void* stream) {
    CAF_REQUIRE(d_src && d_out && len >= 1 && num_freqs >= 1, "caf_dot_tones: bad arguments");
    CAF_REQUIRE((len + 63) / 64 < ((int64_t)1 << 31), "caf_dot_tones: source too long");
    hipLaunchKernelGGL(k_dot_tones, dim3((unsigned)((len + 63) / 64)), dim3(64), 0, (hipStream_t)stream, f0, fstep, num_freqs, len,
                       (const float2*)d_src, (float2*)d_out);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_mul_conj(const float* d_a, const float* d_b, int64_t n, float* d_out, void* stream) {
    CAF_REQUIRE(d_a && d_b && d_out && n >= 0, "caf_mul_conj: bad arguments");
    if (n)
        hipLaunchKernelGGL(k_mul_conj, dim3(std::min<unsigned>(cdiv(n, 256), 256 * 16)), dim3(256), 0, (hipStream_t)stream,
                           (const float2*)d_a, (const float2*)d_b, n, (float2*)d_out);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_steer_dot(const float* d_vec, const double* d_steer, int64_t rows, int64_t n, double scale, double* d_out,
                      void* stream) {
    CAF_REQUIRE(d_vec && d_steer && d_out && rows >= 1 && n >= 1, "caf_steer_dot: bad arguments");
    CAF_REQUIRE(rows < ((int64_t)1 << 31), "caf_steer_dot: too many rows");
    hipLaunchKernelGGL(k_steer_dot, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, (const float2*)d_vec,
                       (const double2*)d_steer, n, scale, (double2*)d_out);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_sum_planes_qf2(const float* d_planes, int32_t num_planes, int64_t rows, int32_t cols, const int32_t* h_sel,
                           int32_t num_sel, const double* d_row_norm, double ynormsq, double* d_out, void* stream) {
    CAF_REQUIRE(d_planes && h_sel && d_row_norm && d_out && num_planes >= 1 && rows >= 1 && cols >= 1,
                "caf_sum_planes_qf2: bad arguments");
    CAF_REQUIRE(num_sel >= 1 && num_sel <= 64, "caf_sum_planes_qf2: between 1 and 64 planes can be summed");
    for (int j = 0; j < num_sel; ++j)
        CAF_REQUIRE(h_sel[j] >= 0 && h_sel[j] < num_planes, "caf_sum_planes_qf2: plane number out of range");
    CAF_REQUIRE(ynormsq > 0.0, "caf_sum_planes_qf2: ynormsq must be positive");
    SumPlanesIdx idx;
    for (int j = 0; j < SUMPL_MAX; ++j) idx.v[j] = j < num_sel ? h_sel[j] : 0;
    const int64_t plane_elems = rows * cols;
    hipLaunchKernelGGL(k_sum_planes_qf2, dim3(std::min<unsigned>(cdiv(plane_elems, 256), 256 * 16)), dim3(256), 0, (hipStream_t)stream,
                       (const float2*)d_planes, plane_elems, cols, idx, num_sel, d_row_norm, ynormsq, d_out);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_sum_groups_qf2(const float* d_planes, int32_t num_groups, int64_t rows, int32_t cols, const float* d_phase,
                           const double* d_row_norm, double ynormsq, double* d_out, void* stream) {
    CAF_REQUIRE(d_planes && d_row_norm && d_out && num_groups >= 1 && rows >= 1 && cols >= 1, "caf_sum_groups_qf2: bad arguments");
    CAF_REQUIRE(ynormsq > 0.0, "caf_sum_groups_qf2: ynormsq must be positive");
    const int64_t plane_elems = rows * cols;
    hipLaunchKernelGGL(k_sum_groups_qf2, dim3(std::min<unsigned>(cdiv(plane_elems, 256), 256 * 16)), dim3(256), 0, (hipStream_t)stream,
                       (const float2*)d_planes, num_groups, plane_elems, cols, (const float2*)d_phase, d_row_norm, ynormsq, d_out);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}
