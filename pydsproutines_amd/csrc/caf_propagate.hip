// Signal propagation (signalCreationRoutines.py: propagateSignal, propagateSignalExact, freqshiftSignal, cupyAddTonePhase,
// cupyGenTonesDirect / cupyGenTonesScaling).  With N samples per row, X = FFT(sig), and k' the signed bin of makeFreq (k' = k
// for 2 k < N, k - N otherwise: for even N bin N / 2 is -fs / 2):
//
//   caf_propagate        out[r][n] = tone[n] IFFT_k( X[r or 0][k] exp(-j 2 pi k' (fs t_r) / N) )[n]
//   caf_propagate_exact  out[r][n] = exp(-j 2 pi f_c tau[r][n]) (1 / N) sum_k X[k] exp(j 2 pi k' u / N),  u = (n - fs tau[r][n]) mod N
//
// Phases.  Every phase is formed and reduced to a fraction of a turn in float64; only the sine and cosine of the reduced phase
// are float32 (unit_f32: the quadrant is taken out in float64 first, so the float32 argument is at most 1 / 8 turn and its
// rounding is below 2^-27 turn).  The products fs tau and f_c tau are taken exactly (product + fma residual, mul_split), so a
// delay of 1e5 samples or a carrier phase of 1e8 turns loses nothing before the reduction; the delay is reduced mod N in
// integers, which changes no phase because k' is an integer.
//
//   k_propagate_exact  N^2 terms per row.  A workgroup of 8 waves owns 64 consecutive outputs n (one per lane) of one row; the
//                      pairs (X[m], X[N - m]), m = 0 .. N / 2, packed by k_px_pairs (the missing partner of m = 0 and of
//                      m = N / 2 is zero, as is the padding to whole blocks) are cut into blocks of PX_L = 32 pairs and the blocks
//                      dealt to the waves in 8 contiguous runs.  Per block a lane seeds the rotor z = exp(j 2 pi frac(m0 u / N))
//                      from the float64 phase, then per pair: acc+ += X[m] z, acc- += X[N - m] conj(z), z *= w with
//                      w = exp(j 2 pi u / N) rounded once from float64: 12 float32 lane operations per pair, 6 per term.  One
//                      rotor serves +m and -m.  The pairs are the same for all lanes: the loads are wave-uniform.  A block's four
//                      float32 sums go into float64 sums per lane, the 8 waves' float64 sums are added in wave order through LDS,
//                      and wave 0 applies 1 / N and the carrier (float64 sincospi of the exactly reduced f_c tau) and rounds once.
//                      Nothing is atomic, the split depends on N alone and rows never meet: a row is bitwise the same whatever R.
//
// Floating-point contraction is off in this file (the tone kernels repeat upstream's float64 roundings); the fused
// multiply-adds of the hot loop are written out.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "caf_internal.h"
#include "caf_phase.h"  // mul_split, frac_turn, unit_f32, cmulf

#pragma clang fp contract(off)

namespace caf {

namespace {

constexpr int PX_WAVE = 64;                      // outputs per workgroup (one per lane)
constexpr int PX_WAVES = 8;                      // waves per workgroup: the k range is cut into this many runs
constexpr int PX_THREADS = PX_WAVE * PX_WAVES;
constexpr int PX_L = 32;                         // pairs per rotor seed (the bound of tests/propagate_ref.py grows with it)
constexpr int PX_MAXN = 1 << 20;
constexpr int EW_THREADS = 256;

// pairs[m] = (X[m] or 0, X[N - m] or 0), m < total (a multiple of PX_L, zero beyond N / 2)
__global__ __launch_bounds__(EW_THREADS) void k_px_pairs(const float2* __restrict__ X, int32_t N, int32_t total, float4* __restrict__ pairs) {
    const int32_t m = (int32_t)blockIdx.x * EW_THREADS + threadIdx.x;
    if (m >= total) return;
    const int32_t P = (N + 1) / 2, H = N / 2;
    float2 a = make_float2(0.f, 0.f), b = make_float2(0.f, 0.f);
    if (m < P) a = X[m];
    if (m >= 1 && m <= H) b = X[N - m];
    pairs[m] = make_float4(a.x, a.y, b.x, b.y);
}

__global__ __launch_bounds__(PX_THREADS) void k_propagate_exact(const float4* __restrict__ pairs, int32_t nblk, int32_t bpw,
                                                              const double* __restrict__ tau, int32_t N, int32_t tiles, double fs,
                                                              double fc, float2* __restrict__ out) {
    __shared__ double2 s_part[PX_WAVES][PX_WAVE];
    const int lane = threadIdx.x & (PX_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int32_t row = (int32_t)blockIdx.x / tiles;
    const int32_t tile = (int32_t)blockIdx.x - row * tiles;
    const int32_t n = tile * PX_WAVE + lane;
    const bool live = n < N;
    const int32_t nn = live ? n : N - 1;  // a lane past the row computes the last output again and stores nothing
    const int64_t at = (int64_t)row * N + nn;
    const double t = tau[at];

    // u = (n - fs tau) mod N in [0, N), v = u / N
    double whole, rest;
    mul_split(fs, t, &whole, &rest);
    double u = fmod((double)nn - whole, (double)N) - rest;
    if (u < 0.0) u += (double)N;
    if (u >= (double)N) u -= (double)N;
    const double v = u / (double)N;
    double ws, wc;
    sincospi(2.0 * frac_turn(v), &ws, &wc);
    const float2 w = make_float2((float)wc, (float)ws);

    double accr = 0.0, acci = 0.0;
    const int b0 = wave * bpw, b1 = std::min(b0 + bpw, nblk);
    for (int b = b0; b < b1; b++) {
        const int m0 = b * PX_L;
        float2 z = unit_f32(frac_turn((double)m0 * v));
        float pr = 0.f, pi = 0.f, qr = 0.f, qi = 0.f;
        const float4* __restrict__ xp = pairs + m0;
#pragma unroll
        for (int j = 0; j < PX_L; j++) {
            const float4 x = xp[j];  // the same address in every lane
            pr = fmaf(x.x, z.x, pr);
            pr = fmaf(-x.y, z.y, pr);
            pi = fmaf(x.x, z.y, pi);
            pi = fmaf(x.y, z.x, pi);
            qr = fmaf(x.z, z.x, qr);
            qr = fmaf(x.w, z.y, qr);
            qi = fmaf(x.w, z.x, qi);
            qi = fmaf(-x.z, z.y, qi);
            z = cmulf(z, w);
        }
        accr += (double)pr + (double)qr;
        acci += (double)pi + (double)qi;
    }
    s_part[wave][lane] = make_double2(accr, acci);
    __syncthreads();
    if (wave != 0) return;
    double sr = s_part[0][lane].x, si = s_part[0][lane].y;
#pragma unroll
    for (int k = 1; k < PX_WAVES; k++) {
        sr += s_part[k][lane].x;
        si += s_part[k][lane].y;
    }
    const double inv = 1.0 / (double)N;
    sr *= inv;
    si *= inv;
    mul_split(fc, t, &whole, &rest);
    double cs, cc;
    sincospi(-2.0 * frac_turn(rest), &cs, &cc);
    if (live) out[at] = make_float2((float)(sr * cc - si * cs), (float)(sr * cs + si * cc));
}

// out[k][i] = spec[k or 0][i] exp(-j 2 pi k'(i) d_k / len), d_k = fs t_k mod len
__global__ __launch_bounds__(EW_THREADS) void k_prop_ramp(const float2* __restrict__ spec, int32_t one_row, const double* __restrict__ time,
                                                         double fs, int64_t len, int64_t total, float2* __restrict__ out) {
    const int64_t at = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x;
    if (at >= total) return;
    const int64_t k = at / len, i = at - k * len;
    const int64_t kp = 2 * i < len ? i : i - len;
    double whole, rest;
    mul_split(fs, time[k], &whole, &rest);
    const double d = fmod(whole, (double)len) + rest;
    const float2 z = unit_f32(frac_turn(-(double)kp * (d / (double)len)));
    out[at] = cmulf(spec[(one_row ? 0 : k) * len + i], z);
}

// the inverse transform's 1 / len and the tone
__global__ __launch_bounds__(EW_THREADS) void k_prop_finish(float2* __restrict__ out, const float2* __restrict__ tone, int64_t len, int64_t total,
                                                           float inv) {
    const int64_t at = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x;
    if (at >= total) return;
    float2 x = out[at];
    x.x *= inv;
    x.y *= inv;
    if (tone) x = cmulf(x, tone[at % len]);
    out[at] = x;
}

// genTones*: upstream's float64 arithmetic to the letter (f = f0 + i fstep, sincospi(2 f n)), stored as complex64 or complex128
template <bool C128>
__global__ __launch_bounds__(EW_THREADS) void k_gen_tones(double f0, double fstep, int64_t length, int64_t total, void* __restrict__ out) {
    const int64_t at = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x;
    if (at >= total) return;
    const int64_t i = at / length, n = at - i * length;
    const double f = f0 + (double)i * fstep;
    double s, c;
    sincospi(2 * f * (double)n, &s, &c);
    if (C128) ((double2*)out)[at] = make_double2(c, s);
    else ((float2*)out)[at] = make_float2((float)c, (float)s);
}

// addPhase: upstream's expression to the letter
__global__ __launch_bounds__(EW_THREADS) void k_add_tone_phase(float* __restrict__ phase, int64_t len, double two_pi_f, double tstart, double tstep) {
    const int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x;
    if (i >= len) return;
    phase[i] = (float)fma(two_pi_f, fma((double)i, tstep, tstart), (double)phase[i]);
}

__global__ __launch_bounds__(EW_THREADS) void k_freq_shift(const float2* __restrict__ x, int64_t len, int64_t total, double fnorm,
                                                          float2* __restrict__ out) {
    const int64_t at = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x;
    if (at >= total) return;
    const int64_t i = at % len;
    out[at] = cmulf(x[at], unit_f32(frac_turn(fnorm * (double)i)));
}

inline bool grid_ok(int64_t total) { return (total + EW_THREADS - 1) / EW_THREADS <= 0x7fffffff; }

}  // namespace

}  // namespace caf

using namespace caf;

int32_t caf_propagate_geometry(int32_t* max_len, int32_t* reseed_interval, int32_t* outputs_per_workgroup, int32_t* waves_per_workgroup) {
    if (max_len) *max_len = PX_MAXN;
    if (reseed_interval) *reseed_interval = PX_L;
    if (outputs_per_workgroup) *outputs_per_workgroup = PX_WAVE;
    if (waves_per_workgroup) *waves_per_workgroup = PX_WAVES;
    return CAF_OK;
}

int32_t caf_propagate(const float* d_sig, int32_t rows_sig, int64_t len, const double* d_time, int32_t num_delays, double fs,
                      const float* d_tone, float* d_out, void* stream) {
    CAF_REQUIRE(len >= 1 && num_delays >= 1, "caf_propagate: len and the number of delays must be positive");
    CAF_REQUIRE(rows_sig == 1 || rows_sig == num_delays, "caf_propagate: one signal row, or one per delay");
    CAF_REQUIRE(len < ((int64_t)1 << 31), "caf_propagate: len < 2^31");
    CAF_REQUIRE(std::isfinite(fs) && fs > 0.0, "caf_propagate: fs must be positive and finite");
    const int64_t total = (int64_t)num_delays * len;
    CAF_REQUIRE(grid_ok(total), "caf_propagate: too many samples for one launch");
    CAF_REQUIRE(d_sig && d_time && d_out, "caf_propagate: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    float2* spec = nullptr;
    if (const int rc = sc.get(&spec, (int64_t)rows_sig * len)) return rc;
    if (const int rc = fft_rows((const float2*)d_sig, spec, rows_sig, len, false, st)) return rc;
    hipLaunchKernelGGL(k_prop_ramp, dim3(cdiv(total, EW_THREADS)), dim3(EW_THREADS), 0, st, (const float2*)spec, rows_sig == 1 ? 1 : 0, d_time,
                       fs, len, total, (float2*)d_out);
    if (const int rc = fft_rows((const float2*)d_out, (float2*)d_out, num_delays, len, true, st)) return rc;
    hipLaunchKernelGGL(k_prop_finish, dim3(cdiv(total, EW_THREADS)), dim3(EW_THREADS), 0, st, (float2*)d_out, (const float2*)d_tone, len, total,
                       (float)(1.0 / (double)len));
    CAF_HIP_TRY(hipGetLastError());
    return sc.finish();
}

int32_t caf_propagate_exact(const float* d_sig, const double* d_tau, int32_t rows, int32_t len, double fs, double f_c, float* d_out,
                            void* stream) {
    CAF_REQUIRE(len >= 1 && len <= PX_MAXN, "caf_propagate_exact: 1 <= len <= 2^20");
    CAF_REQUIRE(rows >= 1, "caf_propagate_exact: rows must be positive");
    CAF_REQUIRE(std::isfinite(fs) && fs > 0.0 && std::isfinite(f_c), "caf_propagate_exact: fs must be positive, fs and f_c finite");
    const int32_t tiles = (len + PX_WAVE - 1) / PX_WAVE;
    CAF_REQUIRE((int64_t)tiles * rows <= 0x7fffffff, "caf_propagate_exact: too many rows for one launch");
    CAF_REQUIRE(d_sig && d_tau && d_out, "caf_propagate_exact: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    const int32_t nblk = (len / 2 + 1 + PX_L - 1) / PX_L;  // blocks of pairs m = 0 .. len / 2
    const int32_t bpw = (nblk + PX_WAVES - 1) / PX_WAVES;
    const int32_t total = nblk * PX_L;
    float2* spec = nullptr;
    float4* pairs = nullptr;
    if (const int rc = sc.get(&spec, len)) return rc;
    if (const int rc = sc.get(&pairs, total)) return rc;
    if (const int rc = fft_rows((const float2*)d_sig, spec, 1, len, false, st)) return rc;
    hipLaunchKernelGGL(k_px_pairs, dim3(cdiv(total, EW_THREADS)), dim3(EW_THREADS), 0, st, (const float2*)spec, len, total, pairs);
    hipLaunchKernelGGL(k_propagate_exact, dim3((unsigned)(tiles * rows)), dim3(PX_THREADS), 0, st, (const float4*)pairs, nblk, bpw, d_tau, len,
                       tiles, fs, f_c, (float2*)d_out);
    CAF_HIP_TRY(hipGetLastError());
    return sc.finish();
}

int32_t caf_gen_tones(double f0, double fstep, int32_t num_freqs, int64_t length, int32_t c128, void* d_out, void* stream) {
    CAF_REQUIRE(num_freqs >= 1 && length >= 1, "caf_gen_tones: the number of frequencies and the length must be positive");
    CAF_REQUIRE(length < ((int64_t)1 << 31), "caf_gen_tones: length < 2^31");
    CAF_REQUIRE(c128 == 0 || c128 == 1, "caf_gen_tones: c128 must be 0 or 1");
    CAF_REQUIRE(std::isfinite(f0) && std::isfinite(fstep), "caf_gen_tones: f0 and fstep must be finite");
    const int64_t total = (int64_t)num_freqs * length;
    CAF_REQUIRE(grid_ok(total), "caf_gen_tones: too many samples for one launch");
    CAF_REQUIRE(d_out, "caf_gen_tones: NULL output");
    hipStream_t st = (hipStream_t)stream;
    if (c128) hipLaunchKernelGGL(k_gen_tones<true>, dim3(cdiv(total, EW_THREADS)), dim3(EW_THREADS), 0, st, f0, fstep, length, total, d_out);
    else hipLaunchKernelGGL(k_gen_tones<false>, dim3(cdiv(total, EW_THREADS)), dim3(EW_THREADS), 0, st, f0, fstep, length, total, d_out);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_add_tone_phase(float* d_phase, int64_t len, double freq, double tstart, double tstep, void* stream) {
    CAF_REQUIRE(len >= 0 && grid_ok(len), "caf_add_tone_phase: bad length");
    if (len == 0) return CAF_OK;
    CAF_REQUIRE(d_phase, "caf_add_tone_phase: NULL phase");
    hipLaunchKernelGGL(k_add_tone_phase, dim3(cdiv(len, EW_THREADS)), dim3(EW_THREADS), 0, (hipStream_t)stream, d_phase, len,
                       6.283185307179586 * freq, tstart, tstep);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_freq_shift(const float* d_x, int64_t rows, int64_t len, double fnorm, float* d_out, void* stream) {
    CAF_REQUIRE(rows >= 1 && len >= 1 && len < ((int64_t)1 << 31), "caf_freq_shift: rows and len must be positive, len < 2^31");
    CAF_REQUIRE(rows <= ((int64_t)1 << 40) / len && grid_ok(rows * len), "caf_freq_shift: too many samples for one launch");
    CAF_REQUIRE(std::isfinite(fnorm), "caf_freq_shift: the frequency must be finite");
    CAF_REQUIRE(d_x && d_out, "caf_freq_shift: NULL argument");
    hipLaunchKernelGGL(k_freq_shift, dim3(cdiv(rows * len, EW_THREADS)), dim3(EW_THREADS), 0, (hipStream_t)stream, (const float2*)d_x, len,
                       rows * len, fnorm, (float2*)d_out);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}
