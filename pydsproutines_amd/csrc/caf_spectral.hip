// The second half of spectralRoutines.py and burstyRoutines.py: tone spectra (toneSpectrum, toneSpec_kernel, toneSpecMulti_kernel
// :394-571, 663-679), the dense DFT at arbitrary frequencies (dft :637-659), IntegerMultipleFFT (:128-232) and burstFFT
// (burstyRoutines.py:14-36).  The float64 paths (tone spectra, DFT) do all arithmetic in float64; the two FFT paths are complex64
// through the rocFFT rows of caf_fft.hip, as the chirp-Z objects are.
//
//   k_tone_spectrum   one thread per (row, frequency), TS_THREADS per workgroup, rows of consecutive parameter sets packed together.
//                     The one body of caf_tone_spectrum (parameters from device lists) and caf_tone_spectrum_one (scalars): both
//                     call tone_value, so a row of the multi form holds the bits of the single form.  With d = f - f0, x = d / fs and
//                     t = x N = whole + r turns (mul_split, frac_turn: |r| <= 1/2),
//                        -j A (1 - e^{-j 2 pi t}) / (2 pi x) e^{j phi}  =  2 sin(pi r) A / (2 pi x) e^{j (phi - pi r)}
//                     ((-1)^whole enters the sine and the phasor alike and cancels).  No 1 - cos: nothing cancels near f0, where the
//                     value tends to A N e^{j phi}, which is what d == 0 returns (the reference returns NaN there).
//   k_dft             a workgroup owns DFT_T frequencies (DFT_F per lane) and a segment of the samples, walked in chunks of DFT_C
//                     samples staged in LDS as complex128 (a complex64 input is widened on the way in).  Per block of DFT_R samples a
//                     lane evaluates sum_i x[n0 + i] s^i by Horner's rule from the block's last sample down (s = e^{-j 2 pi nu},
//                     nu = f / fs: 4 fma per sample, the sample an LDS broadcast) and multiplies by the block's seed
//                     e^{-j 2 pi frac(nu n0)}, nu n0 reduced exactly by mul_split: the drift of s^i is bounded by DFT_R, not by len.
//                     A lane carries DFT_F frequencies, DFT_LANES apart: the steps of one chain wait for each other, the chains do
//                     not, and one LDS broadcast feeds them all.
//                     Few frequencies: len is cut into segments of whole chunks so that about DFT_SPLIT workgroups run, and
//   k_dft_fold        adds the segments' partial sums in segment order.  The cut depends on len and num_freqs alone, never on rows.
//   k_imfft_shift     y[r][i][n] = x[r][n] e^{-j 2 pi i n / (multiple N)}: i n < multiple N is an integer, the fraction of a turn is
//                     formed from it directly (no recurrence), quarter turns in float64, the rest in float32 (unit_f32).
//   k_imfft_transpose (multiple, N) -> (N, multiple) per row through a 32 x 33 LDS tile, coalesced on both sides.
//   k_burst_fold      column sums of the (alpha, length) reshape of a zero-padded row, float64 in row order, rounded once.
// No atomics and no cross-lane sums: a lane owns its output.  Floating-point contraction is off in this file (caf_phase.h needs
// it off): every product and sum is rounded where it is written, and each fma is spelled.
#include <cmath>
#include <cstdint>

#include "caf_internal.h"
#include "caf_phase.h"

#pragma clang fp contract(off)

namespace caf {

namespace {

constexpr int TS_THREADS = 256;   // threads, and outputs, per workgroup of k_tone_spectrum
constexpr int DFT_LANES = 256;    // threads per workgroup of k_dft
constexpr int DFT_F = 4;          // frequencies per lane: one LDS broadcast of a sample feeds 4 DFT_F fma
constexpr int DFT_T = DFT_LANES * DFT_F;  // frequencies per workgroup
constexpr int DFT_C = 1024;       // samples per LDS chunk (16 KiB of complex128)
constexpr int DFT_R = 128;        // samples per Horner block: the re-seed interval
constexpr int DFT_SPLIT = 512;    // workgroups per row that the cut of len aims for (two per compute unit)
constexpr int64_t DFT_MAX_LEN = ((int64_t)1 << 31) - 1;
constexpr int TR_TILE = 32;       // the transpose's tile edge; 32 x 8 threads
constexpr int64_t MAX_ELEMS = (int64_t)1 << 40;

static_assert(DFT_C % DFT_R == 0 && DFT_C % DFT_LANES == 0, "a chunk is whole blocks and whole staging rounds");

__device__ __forceinline__ double2 tone_value(double f, double f0, double phi, double A, double fs, double N) {
    double sphi, cphi;
    sincos(phi, &sphi, &cphi);
    const double d = f - f0;
    if (d == 0.0) {  // the limit
        const double g = A * N;
        return make_double2(g * cphi, g * sphi);
    }
    const double x = d / fs;
    double whole, rest;
    mul_split(x, N, &whole, &rest);
    const double r = frac_turn(rest);
    double sp, cp;
    sincospi(r, &sp, &cp);
    const double coef = A / ((2.0 * M_PI) * x);
    const double g = (2.0 * sp) * coef;
    return make_double2(g * fma(cp, cphi, sp * sphi), g * fma(cp, sphi, -(sp * cphi)));
}

// f0l != nullptr: row i takes (f0l[i], phil[i], Al[i]); otherwise every row (there is one) takes the scalars
__global__ __launch_bounds__(TS_THREADS) void k_tone_spectrum(const double* __restrict__ f0l, const double* __restrict__ phil,
                                                              const double* __restrict__ Al, double f0, double phi, double A, int64_t m,
                                                              const double* __restrict__ freqs, int64_t nf, double fs, double N,
                                                              double2* __restrict__ out) {
    const int64_t at = (int64_t)blockIdx.x * TS_THREADS + threadIdx.x;
    if (at >= m * nf) return;
    const int64_t row = at / nf, k = at - row * nf;
    if (f0l) f0 = f0l[row], phi = phil[row], A = Al[row];
    out[at] = tone_value(freqs[k], f0, phi, A, fs, N);
}

// workgroup = (tile of frequencies, segment, row), the tile fastest; dst is (rows, segs, nf): the output itself when segs == 1.
// Lane l of a tile owns the frequencies l, l + DFT_LANES, ... of it: DFT_F independent chains fed by one LDS broadcast.
template <bool C128>
__global__ __launch_bounds__(DFT_LANES) void k_dft(const void* __restrict__ xv, int64_t len, const double* __restrict__ freqs, int64_t nf,
                                                   double fs, int64_t tiles, int64_t segs, int64_t seg_chunks, double2* __restrict__ dst) {
    __shared__ __attribute__((aligned(16))) double2 xs[DFT_C];
    const int64_t tile = (int64_t)blockIdx.x % tiles, rs = (int64_t)blockIdx.x / tiles;
    const int64_t seg = rs % segs, row = rs / segs;
    const int64_t k0 = tile * DFT_T + threadIdx.x;
    double nu[DFT_F], ss[DFT_F], sc[DFT_F], ar[DFT_F], ai[DFT_F];
#pragma unroll
    for (int f = 0; f < DFT_F; f++) {
        const int64_t k = k0 + f * DFT_LANES;
        nu[f] = (k < nf ? freqs[k] : 0.0) / fs;  // (past the last frequency: nu = 0, nothing stored)
        sincospi(-2.0 * frac_turn(nu[f]), &ss[f], &sc[f]);  // s = e^{-j 2 pi nu}
        ar[f] = 0.0, ai[f] = 0.0;
    }
    const int64_t n_begin = seg * seg_chunks * DFT_C;
    const int64_t n_end = n_begin + seg_chunks * DFT_C < len ? n_begin + seg_chunks * DFT_C : len;
    for (int64_t c0 = n_begin; c0 < n_end; c0 += DFT_C) {
        const int cn = n_end - c0 < DFT_C ? (int)(n_end - c0) : DFT_C;
        __syncthreads();  // the chunk before has been read by every lane
        for (int i = threadIdx.x; i < cn; i += DFT_LANES) {
            if (C128) {
                xs[i] = ((const double2*)xv)[row * len + c0 + i];
            } else {
                const float2 v = ((const float2*)xv)[row * len + c0 + i];
                xs[i] = make_double2((double)v.x, (double)v.y);
            }
        }
        __syncthreads();
        for (int b0 = 0; b0 < cn; b0 += DFT_R) {
            const int bn = cn - b0 < DFT_R ? cn - b0 : DFT_R;
            double hr[DFT_F], hi[DFT_F];
#pragma unroll
            for (int f = 0; f < DFT_F; f++) hr[f] = 0.0, hi[f] = 0.0;
#pragma unroll 4
            for (int i = bn - 1; i >= 0; i--) {
                const double2 v = xs[b0 + i];
#pragma unroll
                for (int f = 0; f < DFT_F; f++) {  // h <- h s + x[b0 + i]
                    const double tr = fma(hr[f], sc[f], fma(-hi[f], ss[f], v.x));
                    const double ti = fma(hr[f], ss[f], fma(hi[f], sc[f], v.y));
                    hr[f] = tr, hi[f] = ti;
                }
            }
#pragma unroll
            for (int f = 0; f < DFT_F; f++) {
                double whole, rest, ws, wc;
                mul_split(nu[f], (double)(c0 + b0), &whole, &rest);
                sincospi(-2.0 * frac_turn(rest), &ws, &wc);  // the seed e^{-j 2 pi frac(nu n0)}
                ar[f] += fma(hr[f], wc, -(hi[f] * ws));
                ai[f] += fma(hr[f], ws, hi[f] * wc);
            }
        }
    }
#pragma unroll
    for (int f = 0; f < DFT_F; f++) {
        const int64_t k = k0 + f * DFT_LANES;
        if (k < nf) dst[rs * nf + k] = make_double2(ar[f], ai[f]);
    }
}

__global__ __launch_bounds__(256) void k_dft_fold(const double2* __restrict__ part, int64_t rows, int64_t segs, int64_t nf,
                                                  double2* __restrict__ out) {
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= rows * nf) return;
    const int64_t row = at / nf, k = at - row * nf;
    const double2* p = part + row * segs * nf + k;
    double re = p[0].x, im = p[0].y;
    for (int64_t s = 1; s < segs; s++) re += p[s * nf].x, im += p[s * nf].y;
    out[at] = make_double2(re, im);
}

__global__ __launch_bounds__(256) void k_imfft_shift(const float2* __restrict__ x, int64_t rows, int64_t len, int64_t mult,
                                                     float2* __restrict__ y) {
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= rows * mult * len) return;
    const int64_t n = at % len, ri = at / len;
    const int64_t i = ri % mult, row = ri / mult;
    const double t = (double)(i * n) / (double)(mult * len);  // i n < mult len: the integer is its own residue
    y[at] = cmulf(x[row * len + n], unit_f32(frac_turn(-t)));
}

// in: (batch, R, C) -> out: (batch, C, R); workgroup = (tile of C, tile of R, batch), the tile of C fastest
__global__ __launch_bounds__(TR_TILE * 8) void k_imfft_transpose(const float2* __restrict__ in, int64_t R, int64_t C, int64_t tiles_c,
                                                                 int64_t tiles_r, float2* __restrict__ out) {
    __shared__ float2 tile[TR_TILE][TR_TILE + 1];
    const int64_t tc = (int64_t)blockIdx.x % tiles_c, q = (int64_t)blockIdx.x / tiles_c;
    const int64_t tr = q % tiles_r, b = q / tiles_r;
    const int tx = threadIdx.x % TR_TILE, ty = threadIdx.x / TR_TILE;
    const float2* src = in + b * R * C;
    float2* dst = out + b * R * C;
#pragma unroll
    for (int j = ty; j < TR_TILE; j += 8) {
        const int64_t r = tr * TR_TILE + j, c = tc * TR_TILE + tx;
        if (r < R && c < C) tile[j][tx] = src[r * C + c];
    }
    __syncthreads();
#pragma unroll
    for (int j = ty; j < TR_TILE; j += 8) {
        const int64_t c = tc * TR_TILE + j, r = tr * TR_TILE + tx;
        if (r < R && c < C) dst[c * R + r] = tile[tx][j];
    }
}

__global__ __launch_bounds__(256) void k_burst_fold(const float2* __restrict__ x, int64_t rows, int64_t len, int64_t length,
                                                    int64_t alpha, float2* __restrict__ y) {
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= rows * length) return;
    const int64_t row = at / length, c = at - row * length;
    const float2* xr = x + row * len;
    double re = 0.0, im = 0.0;
    const int64_t whole = len / length;  // pieces that hold this column whatever it is; the last piece may not (alpha - whole <= 1)
    const float2* p = xr + c;
#pragma unroll 16
    for (int64_t a = 0; a < whole; a++) {  // (no test inside: the loads of an unrolled round are issued together, the sums stay in order)
        const float2 v = p[a * length];
        re += (double)v.x, im += (double)v.y;
    }
    if (whole < alpha && whole * length + c < len) {
        const float2 v = p[whole * length];
        re += (double)v.x, im += (double)v.y;
    }
    y[at] = make_float2((float)re, (float)im);
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool finite_nonzero(double v) { return v != 0.0 && v > -INFINITY && v < INFINITY; }

int check_tone(const char* who, const double* d_freqs, int64_t m, int64_t num_freqs, double fs, int64_t N, const double* d_out,
               int64_t* blocks) {
    const std::string w(who);
    CAF_REQUIRE(d_freqs != nullptr && d_out != nullptr, w + ": NULL pointer");
    CAF_REQUIRE(m >= 1 && num_freqs >= 1, w + ": needs at least one parameter set and one frequency");
    CAF_REQUIRE(N >= 1 && N <= ((int64_t)1 << 53), w + ": N must be in 1 .. 2^53");
    CAF_REQUIRE(finite_nonzero(fs), w + ": fs must be finite and not zero");
    CAF_REQUIRE(aligned(d_freqs, 8) && aligned(d_out, 16), w + ": d_freqs must be 8-byte and d_out 16-byte aligned");
    CAF_REQUIRE(m <= MAX_ELEMS / num_freqs, w + ": too many outputs for one launch");
    *blocks = (m * num_freqs + TS_THREADS - 1) / TS_THREADS;
    CAF_REQUIRE(*blocks <= 0x7fffffff, w + ": too many outputs for one launch");
    return CAF_OK;
}

// the cut of len: segments of seg_chunks whole chunks; a function of len and num_freqs alone
void dft_cut(int64_t len, int64_t num_freqs, int64_t* tiles, int64_t* segs, int64_t* seg_chunks) {
    *tiles = (num_freqs + DFT_T - 1) / DFT_T;
    const int64_t nchunks = (len + DFT_C - 1) / DFT_C;
    int64_t want = (DFT_SPLIT + *tiles - 1) / *tiles;
    if (want > nchunks) want = nchunks;
    if (want < 1) want = 1;
    *seg_chunks = (nchunks + want - 1) / want;
    *segs = (nchunks + *seg_chunks - 1) / *seg_chunks;
}

}  // namespace

}  // namespace caf

using namespace caf;

int32_t caf_tone_spectrum(const double* d_f0, const double* d_phi, const double* d_A, int64_t m, const double* d_freqs, int64_t num_freqs,
                          double fs, int64_t N, double* d_out, void* stream) {
    int64_t blocks = 0;
    if (int rc = check_tone("caf_tone_spectrum", d_freqs, m, num_freqs, fs, N, d_out, &blocks)) return rc;
    CAF_REQUIRE(d_f0 != nullptr && d_phi != nullptr && d_A != nullptr, "caf_tone_spectrum: NULL parameter list");
    CAF_REQUIRE(aligned(d_f0, 8) && aligned(d_phi, 8) && aligned(d_A, 8), "caf_tone_spectrum: the parameter lists must be 8-byte aligned");
    hipLaunchKernelGGL(k_tone_spectrum, dim3((unsigned)blocks), dim3(TS_THREADS), 0, (hipStream_t)stream, d_f0, d_phi, d_A, 0.0, 0.0, 0.0, m,
                       d_freqs, num_freqs, fs, (double)N, (double2*)d_out);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_tone_spectrum_one(double f0, double phi, double A, const double* d_freqs, int64_t num_freqs, double fs, int64_t N, double* d_out,
                              void* stream) {
    int64_t blocks = 0;
    if (int rc = check_tone("caf_tone_spectrum_one", d_freqs, 1, num_freqs, fs, N, d_out, &blocks)) return rc;
    hipLaunchKernelGGL(k_tone_spectrum, dim3((unsigned)blocks), dim3(TS_THREADS), 0, (hipStream_t)stream, (const double*)nullptr,
                       (const double*)nullptr, (const double*)nullptr, f0, phi, A, (int64_t)1, d_freqs, num_freqs, fs, (double)N,
                       (double2*)d_out);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_dft_geometry(int32_t* freqs_per_workgroup, int32_t* samples_per_chunk, int32_t* reseed_interval, int64_t* max_len,
                         int32_t* split_workgroups) {
    if (freqs_per_workgroup) *freqs_per_workgroup = DFT_T;
    if (samples_per_chunk) *samples_per_chunk = DFT_C;
    if (reseed_interval) *reseed_interval = DFT_R;
    if (max_len) *max_len = DFT_MAX_LEN;
    if (split_workgroups) *split_workgroups = DFT_SPLIT;
    return CAF_OK;
}

int32_t caf_dft_rows(const void* d_x, int32_t c128, int64_t rows, int64_t len, const double* d_freqs, int64_t num_freqs, double fs,
                     double* d_out, void* stream) {
    CAF_REQUIRE(d_x != nullptr && d_freqs != nullptr && d_out != nullptr, "caf_dft_rows: NULL pointer");
    CAF_REQUIRE(c128 == 0 || c128 == 1, "caf_dft_rows: c128 must be 0 (complex64 input) or 1 (complex128 input)");
    CAF_REQUIRE(rows >= 1 && num_freqs >= 1, "caf_dft_rows: needs at least one row and one frequency");
    CAF_REQUIRE(num_freqs <= MAX_ELEMS / DFT_SPLIT, "caf_dft_rows: too many frequencies for one launch");
    CAF_REQUIRE(len >= 1 && len <= DFT_MAX_LEN, "caf_dft_rows: len must be in 1 .. 2^31 - 1");
    CAF_REQUIRE(finite_nonzero(fs), "caf_dft_rows: fs must be finite and not zero");
    CAF_REQUIRE(aligned(d_x, c128 ? 16 : 8), "caf_dft_rows: d_x must be aligned to its element (8 bytes complex64, 16 bytes complex128)");
    CAF_REQUIRE(aligned(d_freqs, 8) && aligned(d_out, 16), "caf_dft_rows: d_freqs must be 8-byte and d_out 16-byte aligned");
    int64_t tiles, segs, seg_chunks;
    dft_cut(len, num_freqs, &tiles, &segs, &seg_chunks);
    CAF_REQUIRE(rows <= MAX_ELEMS / len && rows <= MAX_ELEMS / (num_freqs * segs) && tiles * segs <= 0x7fffffff / rows,
                "caf_dft_rows: too many rows for one launch");
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    double2* dst = (double2*)d_out;
    if (segs > 1)
        if (int rc = sc.get(&dst, rows * segs * num_freqs)) return rc;
    const dim3 grid((unsigned)(tiles * segs * rows));
    if (c128) hipLaunchKernelGGL(k_dft<true>, grid, dim3(DFT_LANES), 0, st, d_x, len, d_freqs, num_freqs, fs, tiles, segs, seg_chunks, dst);
    else hipLaunchKernelGGL(k_dft<false>, grid, dim3(DFT_LANES), 0, st, d_x, len, d_freqs, num_freqs, fs, tiles, segs, seg_chunks, dst);
    CAF_HIP_TRY(hipGetLastError());
    if (segs > 1) {
        hipLaunchKernelGGL(k_dft_fold, dim3(cdiv(rows * num_freqs, 256)), dim3(256), 0, st, (const double2*)dst, rows, segs, num_freqs,
                           (double2*)d_out);
        CAF_HIP_TRY(hipGetLastError());
    }
    return sc.finish();
}

int32_t caf_integer_multiple_fft(const float* d_x, int64_t rows, int64_t len, int32_t multiple, int32_t reorder, float* d_out, void* stream) {
    CAF_REQUIRE(d_x != nullptr && d_out != nullptr, "caf_integer_multiple_fft: NULL pointer");
    CAF_REQUIRE(rows >= 1 && len >= 1 && multiple >= 1, "caf_integer_multiple_fft: needs at least one row, one sample and multiple >= 1");
    CAF_REQUIRE(len <= 0x7fffffff / (int64_t)multiple, "caf_integer_multiple_fft: the padded length multiple * len must stay below 2^31");
    const int64_t M = (int64_t)multiple * len;
    CAF_REQUIRE(rows <= MAX_ELEMS / M, "caf_integer_multiple_fft: too many rows for one launch");
    CAF_REQUIRE(aligned(d_x, 8) && aligned(d_out, 8), "caf_integer_multiple_fft: d_x and d_out must be 8-byte aligned");
    const int64_t total = rows * M, blocks = (total + 255) / 256;
    const int64_t tiles_c = (len + TR_TILE - 1) / TR_TILE, tiles_r = ((int64_t)multiple + TR_TILE - 1) / TR_TILE;
    CAF_REQUIRE(blocks <= 0x7fffffff && tiles_c * tiles_r <= 0x7fffffff / rows, "caf_integer_multiple_fft: too many rows for one launch");
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    // (multiple, N) and (N, multiple) are the same memory when either is 1: only a true transpose needs the scratch
    const bool transpose = reorder != 0 && multiple > 1 && len > 1;
    float2* work = (float2*)d_out;
    if (transpose)
        if (int rc = sc.get(&work, total)) return rc;
    hipLaunchKernelGGL(k_imfft_shift, dim3((unsigned)blocks), dim3(256), 0, st, (const float2*)d_x, rows, len, (int64_t)multiple, work);
    CAF_HIP_TRY(hipGetLastError());
    if (len > 1)  // (a one-point transform is the identity)
        if (int rc = fft_rows(work, work, rows * multiple, len, false, st)) return rc;
    if (transpose) {
        hipLaunchKernelGGL(k_imfft_transpose, dim3((unsigned)(tiles_c * tiles_r * rows)), dim3(TR_TILE * 8), 0, st, (const float2*)work,
                           (int64_t)multiple, len, tiles_c, tiles_r, (float2*)d_out);
        CAF_HIP_TRY(hipGetLastError());
    }
    return sc.finish();
}

int32_t caf_burst_fft(const float* d_x, int64_t rows, int64_t len, int64_t length, float* d_out, void* stream) {
    CAF_REQUIRE(d_x != nullptr && d_out != nullptr, "caf_burst_fft: NULL pointer");
    CAF_REQUIRE(rows >= 1 && len >= 1, "caf_burst_fft: needs at least one row and one sample");
    CAF_REQUIRE(length >= 1 && length <= 0x7fffffff, "caf_burst_fft: length must be in 1 .. 2^31 - 1");
    CAF_REQUIRE(rows <= MAX_ELEMS / len && rows <= MAX_ELEMS / length, "caf_burst_fft: too many rows for one launch");
    CAF_REQUIRE(aligned(d_x, 8) && aligned(d_out, 8), "caf_burst_fft: d_x and d_out must be 8-byte aligned");
    const int64_t alpha = (len + length - 1) / length, blocks = (rows * length + 255) / 256;
    CAF_REQUIRE(blocks <= 0x7fffffff, "caf_burst_fft: too many rows for one launch");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_burst_fold, dim3((unsigned)blocks), dim3(256), 0, st, (const float2*)d_x, rows, len, length, alpha, (float2*)d_out);
    CAF_HIP_TRY(hipGetLastError());
    if (length > 1)
        if (int rc = fft_rows((float2*)d_out, (float2*)d_out, rows, length, false, st)) return rc;
    return CAF_OK;
}
