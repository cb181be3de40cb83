// Cyclic-moment line search for batches of bursts (cyclostationaryRoutines.py: PSKOrderDetector, estimateOffsetViaCM,
// estimateBaud all raise a burst to a power or take its modulus, transform it and keep the strongest spectral line).
// Per (row, moment) the sequence
//     moment 0:        z = |x| - mean(|x|)            moment 1:   z = |x|^2 - mean(|x|^2)
//     moment 2, 4, 8:  z = x^m by repeated complex squaring
// over the row's own L samples (zeros up to nfft), Z = DFT_nfft(z), and over a band of signed bins: the FFT-order index of
// the largest |Z|^2 (the lower index of equal values), |Z| there and at its two circular neighbours, and the band's sum of |Z|^2.
//   * nfft = 2^6 .. 2^14: ONE kernel -- the row is loaded once, scaled, powered in registers, transformed in LDS
//     (caf_ldsfft.h), and the spectrum never leaves the workgroup.  Rows of up to 64 threads share a 256-thread workgroup.
//   * any other nfft: the same definitions composed from an elementwise kernel, the rocFFT rows and a band-limited line
//     kernel.
// Range: every row is scaled by 2^-e, e the exponent of its largest component, so x^8 stays inside float32 whatever the
// row's level; the scaling is exact and e goes back into the float64 outputs with ldexp.
// Reproducibility: a row's arithmetic depends on the row, nfft and the moments alone -- sums and arg max go through the
// fixed orders of caf_wave.h inside the row's own threads, nothing is accumulated across rows, no atomics.
#include "caf_internal.h"
#include "caf_ldsfft.h"
#include "caf_wave.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>

namespace caf {

namespace {

constexpr int CM_MAX_MOMENTS = 5;
constexpr int CM_THREADS = 256;           // composed form: threads per row
constexpr int64_t CM_CHUNK = 1 << 25;     // composed form: complex values of scratch per chunk of rows

struct CmArgs {
    const float2* x;
    int64_t pitch;
    const int32_t* lengths;
    int64_t rows;
    int32_t nfft, nm;
    int32_t mom[CM_MAX_MOMENTS], lo[CM_MAX_MOMENTS], hi[CM_MAX_MOMENTS];
    int32_t order[CM_MAX_MOMENTS];  // the moments in ascending order of their code: |x| forms first, then 2, 4, 8
    int32_t* index;
    double* peak;
    double* side;
    double* power;
};

template <int LOGN>
struct CmGeo {
    static constexpr int N = 1 << LOGN, NTR = N / 16, WG = NTR > 64 ? NTR : 256, RPW = WG / NTR, WAVES = WG / 64;
    static constexpr size_t LDS = (size_t)RPW * (N + N / 16) * sizeof(float2);
};

__device__ __forceinline__ float2 cm_sq(float2 a) { return make_float2(a.x * a.x - a.y * a.y, 2.0f * (a.x * a.y)); }
__device__ __forceinline__ double cm_abs2(float2 a) { return (double)a.x * (double)a.x + (double)a.y * (double)a.y; }
// |a| (moment 0) or |a|^2 (moment 1) in float64
__device__ __forceinline__ double cm_modulus(float2 a, int m) {
    const double d = cm_abs2(a);
    return m == 0 ? sqrt(d) : d;
}
__device__ __forceinline__ float2 cm_scale(float2 a, int e) { return make_float2(ldexpf(a.x, -e), ldexpf(a.y, -e)); }
// the exponent of the row's largest component: amax = f 2^e, 0.5 <= f < 1 (0 for a row of zeros)
__device__ __forceinline__ int cm_exponent(float amax) {
    int e = 0;
    if (amax > 0.0f && amax <= 3.4028234e38f) (void)frexpf(amax, &e);
    return e;
}
// the power of two that goes back into |Z| of a moment
__device__ __forceinline__ int cm_unscale(int32_t m, int e) { return (m == 0 ? 1 : m == 1 ? 2 : m) * e; }
__device__ __forceinline__ bool cm_in_band(int f, int n, int lo, int hi) {
    const int s = f > (n - 1) / 2 ? f - n : f;
    return s >= lo && s <= hi;
}

// what thread 0 of a row writes: `z` is the row's spectrum in FFT order, readable by that thread
__device__ __forceinline__ void cm_store(const CmArgs& a, int64_t row, int k, int n, double bv, int bi, double ps, int e,
                                         const float2* z) {
    const int64_t o = row * a.nm + k;
    const bool none = !(bv > 0.0) || bi < 0 || bi >= n;  // a row of zeros, an empty row, NaN throughout
    const int sh = cm_unscale(a.mom[k], e);
    a.index[o] = none ? -1 : bi;
    if (a.peak) a.peak[o] = none ? 0.0 : ldexp(sqrt(bv), sh);
    if (a.side) {
        a.side[2 * o] = none ? 0.0 : ldexp(sqrt(cm_abs2(z[bi == 0 ? n - 1 : bi - 1])), sh);
        a.side[2 * o + 1] = none ? 0.0 : ldexp(sqrt(cm_abs2(z[bi == n - 1 ? 0 : bi + 1])), sh);
    }
    if (a.power) a.power[o] = none ? 0.0 : ldexp(ps, 2 * sh);
}

// ---- the in-LDS form ---------------------------------------------------------------------------------------------------
// sum / maximum / arg max over the threads of ONE row: inside the wave for rows of up to 64 threads, else over the workgroup
// (which then holds exactly one row).  The maximum is wanted in every thread, where block_max of caf_wave.h leaves it in
// thread 0; a maximum has no order to keep, so the fold of the waves' values is written out here.
template <int LOGN>
__device__ __forceinline__ double cm_row_sum(double v, double (&lds)[CmGeo<LOGN>::WAVES]) {
    if constexpr (CmGeo<LOGN>::NTR <= 64) return wave_sum<CmGeo<LOGN>::NTR>(v);
    else return block_sum_all<CmGeo<LOGN>::WAVES>(v, lds);
}
template <int LOGN>
__device__ __forceinline__ float cm_row_max(float v, float (&lds)[CmGeo<LOGN>::WAVES]) {
    if constexpr (CmGeo<LOGN>::NTR <= 64) {
        return wave_max<CmGeo<LOGN>::NTR>(v);
    } else {
        v = wave_max(v);
        if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
        __syncthreads();
        v = lds[0];
#pragma unroll
        for (int w = 1; w < CmGeo<LOGN>::WAVES; ++w) v = lds[w] > v ? lds[w] : v;
        __syncthreads();
        return v;
    }
}
template <int LOGN>
__device__ __forceinline__ void cm_row_argmax(double& v, int& i, WaveSlots<CmGeo<LOGN>::WAVES, double, int>& lds) {
    if constexpr (CmGeo<LOGN>::NTR <= 64) wave_argmax<CmGeo<LOGN>::NTR / 2>(v, i);
    else block_argmax_all<CmGeo<LOGN>::WAVES>(lds, v, i);
}

template <int LOGN>
__global__ __launch_bounds__(CmGeo<LOGN>::WG) void k_cm_lds(const CmArgs a, const float2* __restrict__ tw) {
    using G = CmGeo<LOGN>;
    constexpr int N = G::N, NTR = G::NTR;
    extern __shared__ __attribute__((aligned(16))) float2 s_buf[];
    __shared__ double s_sum[G::WAVES];
    __shared__ float s_max[G::WAVES];
    __shared__ WaveSlots<G::WAVES, double, int> s_arg;
    const int tid = threadIdx.x;
    const int rl = tid / NTR, l = tid - rl * NTR;
    float2* buf = s_buf + rl * (N + N / 16);
    const int64_t row = (int64_t)blockIdx.x * G::RPW + rl;
    const bool live = row < a.rows;  // the row slots behind the last row run the barriers on zeros
    const int L = !live ? 0 : a.lengths ? a.lengths[row] : (int)a.pitch;

    // the row, once: p[t] = x[l + t N/16], zeros from L on
    float2 p[16];
    const float2* xr = a.x + (live ? row : 0) * a.pitch;
    float amax = 0.0f;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int i = l + t * NTR;
        p[t] = i < L ? xr[i] : make_float2(0.f, 0.f);
        amax = fmaxf(amax, fmaxf(fabsf(p[t].x), fabsf(p[t].y)));
    }
    amax = cm_row_max<LOGN>(amax, s_max);
    const int e = cm_exponent(amax);  // the same in every thread of the row
#pragma unroll
    for (int t = 0; t < 16; ++t) p[t] = cm_scale(p[t], e);

    int cur = 1;  // p holds x^cur
    for (int j = 0; j < a.nm; ++j) {
        const int k = a.order[j];
        const int m = a.mom[k];
        float2 v[16];
        if (m <= 1) {
            // |x| or |x|^2 in float64, its mean over the row's L samples in the orders of caf_wave.h, and ONE rounding of
            // the mean-removed value to float32
            // (formed twice rather than kept: sixteen float64 values are 32 registers)
            double s = 0.0;
#pragma unroll
            for (int t = 0; t < 16; ++t) s += cm_modulus(p[t], m);
            s = cm_row_sum<LOGN>(s, s_sum);
            const double mean = L > 0 ? s / (double)L : 0.0;
#pragma unroll
            for (int t = 0; t < 16; ++t) v[t] = make_float2(l + t * NTR < L ? (float)(cm_modulus(p[t], m) - mean) : 0.f, 0.f);
        } else {
            while (cur < m) {
#pragma unroll
                for (int t = 0; t < 16; ++t) p[t] = cm_sq(p[t]);
                cur *= 2;
            }
#pragma unroll
            for (int t = 0; t < 16; ++t) v[t] = p[t];
        }
        // The twiddles and the LDS addresses of a thread are the same for every moment, and hoisted out of this loop they
        // would occupy some 80 registers across it: the table's address and the thread's place in the row are made opaque
        // per turn, so twiddles are fetched (from L2) and addresses formed where they are used.
        const float2* twj = tw;
        int lj = l;
        asm volatile("" : "+s"(twj), "+v"(lj));
        // pd_fft is the inverse kernel: register r holds Y[q] = Z[(N - q) mod N]
        pd_fft<LOGN>(buf, twj, lj, v);
        // (the last pass ends behind a row barrier with every read of the image done: it may be overwritten)
        const int lo = a.lo[k], hi = a.hi[k];
        double bv = -1.0, ps = 0.0;
        int bi = INT_MAX;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = (N - pd_out_index<LOGN>(lj, r)) & (N - 1);
            buf[f] = v[r];  // the spectrum in FFT order, for the neighbours of the peak
            const double w = cm_abs2(v[r]);
            if (cm_in_band(f, N, lo, hi)) {
                ps += w;
                if (first_max(bv, bi, w, f)) bv = w, bi = f;
            }
        }
        ps = cm_row_sum<LOGN>(ps, s_sum);
        cm_row_argmax<LOGN>(bv, bi, s_arg);
        pd_row_sync<LOGN>();  // the image is complete
        if (live && l == 0) cm_store(a, row, k, N, bv, bi, ps, e, buf);
        pd_row_sync<LOGN>();  // ... and read before the next transform writes it
    }
}

template <int LOGN>
int cm_lds_launch(const CmArgs& a, const float2* tw, hipStream_t st) {
    using G = CmGeo<LOGN>;
    if (const int rc = allow_dynamic_lds(reinterpret_cast<const void*>(k_cm_lds<LOGN>), G::LDS)) return rc;
    const int64_t nwg = (a.rows + G::RPW - 1) / G::RPW;
    CAF_REQUIRE(nwg <= 0x7fffffff, "caf_cm_lines: too many rows for one launch");
    hipLaunchKernelGGL(k_cm_lds<LOGN>, dim3((unsigned)nwg), dim3(G::WG), G::LDS, st, a, tw);
    return CAF_OK;
}

// ---- the composed form -------------------------------------------------------------------------------------------------
// z of one moment for the rows row0 .. row0 + gridDim.x - 1: (rows, nfft) complex64, and the rows' exponents
__global__ __launch_bounds__(CM_THREADS) void k_cm_power(const CmArgs a, int k, int64_t row0, float2* __restrict__ z,
                                                         int32_t* __restrict__ expo) {
    constexpr int WAVES = CM_THREADS / 64;
    __shared__ float s_max[WAVES];
    __shared__ double s_sum[WAVES];
    const int64_t row = row0 + blockIdx.x;
    const int L = a.lengths ? a.lengths[row] : (int)a.pitch;
    const int n = a.nfft, m = a.mom[k];
    const float2* xr = a.x + row * a.pitch;
    float2* zr = z + (int64_t)blockIdx.x * n;
    float amax = 0.0f;
    for (int i = threadIdx.x; i < L; i += CM_THREADS) amax = fmaxf(amax, fmaxf(fabsf(xr[i].x), fabsf(xr[i].y)));
    amax = wave_max(amax);
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = amax;
    __syncthreads();
    amax = s_max[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) amax = s_max[w] > amax ? s_max[w] : amax;
    const int e = cm_exponent(amax);
    if (threadIdx.x == 0) expo[blockIdx.x] = e;
    double mean = 0.0;
    if (m <= 1) {
        double s = 0.0;
        for (int i = threadIdx.x; i < L; i += CM_THREADS) {
            const double d = cm_abs2(cm_scale(xr[i], e));
            s += m == 0 ? sqrt(d) : d;
        }
        s = block_sum<WAVES>(s, s_sum);
        mean = L > 0 ? s / (double)L : 0.0;
    }
    for (int i = threadIdx.x; i < n; i += CM_THREADS) {
        float2 v = make_float2(0.f, 0.f);
        if (i < L) {
            const float2 xs = cm_scale(xr[i], e);
            if (m <= 1) {
                const double d = cm_abs2(xs);
                v.x = (float)((m == 0 ? sqrt(d) : d) - mean);
            } else {
                v = xs;
                for (int c = 1; c < m; c *= 2) v = cm_sq(v);
            }
        }
        zr[i] = v;
    }
}

// the line of one moment in the band, from the rows' spectra
__global__ __launch_bounds__(CM_THREADS) void k_cm_line(const CmArgs a, int k, int64_t row0, const float2* __restrict__ z,
                                                        const int32_t* __restrict__ expo) {
    constexpr int WAVES = CM_THREADS / 64;
    __shared__ double s_sum[WAVES];
    __shared__ WaveSlots<WAVES, double, int> s_arg;
    const int64_t row = row0 + blockIdx.x;
    const int n = a.nfft, lo = a.lo[k], hi = a.hi[k];
    const float2* zr = z + (int64_t)blockIdx.x * n;
    double bv = -1.0, ps = 0.0;
    int bi = INT_MAX;
    // the band in FFT order: the bins 0 .. hi (from lo where lo > 0), then the negative bins n + lo .. n - 1 (to hi where hi < 0)
    const int a0 = lo > 0 ? lo : 0, a1 = hi;              // [a0, a1], empty when hi < 0
    const int b0 = n + lo, b1 = hi < 0 ? n + hi : n - 1;  // [b0, b1], empty when lo >= 0
    if (hi >= 0)
        for (int f = a0 + threadIdx.x; f <= a1; f += CM_THREADS) {
            const double w = cm_abs2(zr[f]);
            ps += w;
            if (first_max(bv, bi, w, f)) bv = w, bi = f;
        }
    if (lo < 0)
        for (int f = b0 + threadIdx.x; f <= b1; f += CM_THREADS) {
            const double w = cm_abs2(zr[f]);
            ps += w;
            if (first_max(bv, bi, w, f)) bv = w, bi = f;
        }
    ps = block_sum_all<WAVES>(ps, s_sum);
    block_argmax<WAVES>(s_arg, bv, bi);
    if (threadIdx.x == 0) cm_store(a, row, k, n, bv, bi, ps, expo[blockIdx.x], zr);
}

bool cm_lds_ok(int64_t nfft) { return nfft >= 64 && nfft <= 16384 && (nfft & (nfft - 1)) == 0; }
int cm_log2(int64_t n) {
    int l = 0;
    while (((int64_t)1 << l) < n) ++l;
    return l;
}

// CAF_CYCLO_DEBUG=1 (read per call, like CAF_FIR_DEBUG): one stderr line per caf_cm_lines call naming the form that ran
bool cm_debug() {
    const char* e = std::getenv("CAF_CYCLO_DEBUG");
    return e && e[0] == '1';
}

int cm_composed(const CmArgs& a, hipStream_t st) {
    Scratch sc(st);
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(a.rows, std::min<int64_t>(CM_CHUNK / a.nfft, 65535)));
    float2* z = nullptr;
    int32_t* expo = nullptr;
    if (const int rc = sc.get(&z, chunk * a.nfft)) return rc;
    if (const int rc = sc.get(&expo, chunk)) return rc;
    for (int64_t r0 = 0; r0 < a.rows; r0 += chunk) {
        const int64_t nr = std::min(chunk, a.rows - r0);
        for (int k = 0; k < a.nm; ++k) {
            hipLaunchKernelGGL(k_cm_power, dim3((unsigned)nr), dim3(CM_THREADS), 0, st, a, k, r0, z, expo);
            if (const int rc = fft_rows(z, z, nr, a.nfft, false, st)) return rc;
            hipLaunchKernelGGL(k_cm_line, dim3((unsigned)nr), dim3(CM_THREADS), 0, st, a, k, r0, (const float2*)z, (const int32_t*)expo);
        }
    }
    CAF_HIP_TRY(hipGetLastError());
    return sc.finish();
}

}  // namespace

}  // namespace caf

using namespace caf;

int32_t caf_cm_geometry(int64_t nfft, int32_t* form, int32_t* threads, int32_t* rows_per_wg, int64_t* lds_bytes) {
    int f = 0, t = 0, r = 0;
    int64_t b = 0;
    if (cm_lds_ok(nfft)) {
        const int ntr = (int)nfft / 16;
        f = 1, t = ntr > 64 ? ntr : 256, r = t / ntr, b = (int64_t)r * (nfft + nfft / 16) * (int64_t)sizeof(float2);
    } else if (nfft >= 1 && nfft < ((int64_t)1 << 31)) {
        f = 2, t = CM_THREADS, r = 1;
    }
    if (form) *form = f;
    if (threads) *threads = t;
    if (rows_per_wg) *rows_per_wg = r;
    if (lds_bytes) *lds_bytes = b;
    return CAF_OK;
}

int32_t caf_cm_lines(const float* d_x, int64_t rows, int64_t pitch, const int32_t* d_lengths, int64_t nfft, const int32_t* moments,
                     int32_t num_moments, const int32_t* band_lo, const int32_t* band_hi, int32_t* d_index, double* d_peak,
                     double* d_side, double* d_power, void* stream) {
    CAF_REQUIRE(d_x && d_index && moments && band_lo && band_hi, "caf_cm_lines: NULL argument");
    CAF_REQUIRE(rows >= 1 && pitch >= 1 && pitch < ((int64_t)1 << 31), "caf_cm_lines: rows >= 1 and 1 <= pitch < 2^31");
    CAF_REQUIRE(nfft >= 1 && nfft < ((int64_t)1 << 31), "caf_cm_lines: 1 <= nfft < 2^31");
    CAF_REQUIRE(num_moments >= 1 && num_moments <= CM_MAX_MOMENTS, "caf_cm_lines: 1 to 5 moments");
    CAF_REQUIRE(rows * num_moments < ((int64_t)1 << 31), "caf_cm_lines: rows x moments must stay below 2^31");
    hipStream_t st = (hipStream_t)stream;
    CmArgs a{};
    a.x = (const float2*)d_x, a.pitch = pitch, a.lengths = d_lengths, a.rows = rows, a.nfft = (int32_t)nfft, a.nm = num_moments;
    a.index = d_index, a.peak = d_peak, a.side = d_side, a.power = d_power;
    int n = 0;
    for (int code : {0, 1, 2, 4, 8})
        for (int k = 0; k < num_moments; ++k)
            if (moments[k] == code) a.order[n++] = k;
    CAF_REQUIRE(n == num_moments, "caf_cm_lines: a moment is one of 0, 1, 2, 4, 8");
    for (int k = 0; k < num_moments; ++k) {
        a.mom[k] = moments[k], a.lo[k] = band_lo[k], a.hi[k] = band_hi[k];
        CAF_REQUIRE(-(nfft / 2) <= a.lo[k] && a.lo[k] <= a.hi[k] && a.hi[k] <= (nfft - 1) / 2,
                    "caf_cm_lines: a band must satisfy -nfft/2 <= lo <= hi <= nfft/2 - 1");
    }
    if (d_lengths) {  // (downloaded and checked before a launch: complete on return)
        std::vector<int32_t> h((size_t)rows);
        if (const int rc = host_d2h(h.data(), d_lengths, rows * 4, st)) return rc;
        for (int64_t r = 0; r < rows; ++r) {
            if (h[r] < 0 || h[r] > pitch || h[r] > nfft) {
                set_error("caf_cm_lines: a row's length must lie within 0 .. min(pitch, nfft) (row " + std::to_string(r) + " has " +
                          std::to_string(h[r]) + ")");
                return CAF_ERR_INVALID;
            }
        }
    } else {
        CAF_REQUIRE(pitch <= nfft, "caf_cm_lines: nfft is shorter than the rows");
    }
    if (!cm_lds_ok(nfft)) {
        if (cm_debug()) std::fprintf(stderr, "[caf cyclo] cm_rocfft nfft=%lld\n", (long long)nfft);
        return cm_composed(a, st);
    }
    int dev = 0;
    CAF_HIP_TRY(hipGetDevice(&dev));
    const float2* tw = nullptr;
    if (const int rc = lds_fft_twiddles(dev, &tw)) return rc;
    int rc = CAF_OK, rpw = 0;
    switch (cm_log2(nfft)) {
#define CM_CASE(LOGN)                           \
    case LOGN:                                  \
        rpw = CmGeo<LOGN>::RPW;                 \
        rc = cm_lds_launch<LOGN>(a, tw, st);    \
        break;
        CM_CASE(6) CM_CASE(7) CM_CASE(8) CM_CASE(9) CM_CASE(10) CM_CASE(11) CM_CASE(12) CM_CASE(13) CM_CASE(14)
#undef CM_CASE
    }
    if (rc) return rc;
    if (cm_debug()) std::fprintf(stderr, "[caf cyclo] cm_lds nfft=%lld rows/wg=%d\n", (long long)nfft, rpw);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}
