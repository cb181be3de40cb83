// FAM spectral-correlation estimator for batches of records (cyclostationaryRoutines.py: scfFAM, cycleLines, estimateBaudSCF).
// Per row x of n complex64 samples, a window a(n) of N' points, a hop of L samples, P hops and a smoothing g(r) >= 0:
//     X(k, r)    = sum_{n < N'} a(n) x(rL + n) e^{-j 2 pi k (rL + n) / N'}            k in [-N'/2, N'/2), r < P
//     S(k, l, q) = sum_r g(r) X(k, r) conj(X(l, r)) e^{-j 2 pi q r / P}               q in [-M/2, M/2), M = P L / N'
// (the conjugate form drops the conj), psd(k) = sum_r g(r) |X(k, r)|^2, and a cell's value |S|^2 or |S|^2 / (psd(k) psd(l)).
// Three launches and a decode per chunk of rows, every intermediate in pooled scratch that stays in L2 / Infinity Cache:
//   k_scf_demod   the window's samples of 4096 / N' hops staged once (caf_stage.h), one N'-point transform per hop in LDS
//                 (caf_ldsfft.h), the absolute-phase rotation from the twiddle table at the INTEGER phase (k (rL mod N')) mod N'
//                 -- nothing grows with r -- and X written channel-major, (rows, N', P).
//   k_scf_psd     psd(k) in float64: a thread's hops in increasing order, then the orders of caf_wave.h.
//   k_scf_pair    per (row, k, l): the P products in registers from the two channel rows, pd_fft<log2 P> in LDS, |.|^2 and the
//                 quotient in float64 from the float32 transform, rounded once to float32; then the cell store and/or the fold
//                 into the profile.  The transform is never written.
// Work split of the pair kernel.  The pairs of one d (d = k - l, or k + l in the conjugate form) compete for the same alpha-bins.
// The diagonals d' and d' - N' hold N' - d' and d' pairs: joined they are N' "combined diagonals" of exactly N' pairs, cut into
// chunks of C pairs.  One chunk is the work of P / 16 threads (a whole workgroup from P = 2048 on, 256 / (P / 16) chunks to a
// workgroup below), which walk it in increasing s, keep the running maximum of every bin in registers (a strict > keeps the
// smaller s of equal values) and send ONE 64-bit integer maximum per bin and diagonal: the value's bits in the high word
// (non-negative floats order as integers; NaN is made the one positive quiet NaN and so orders above everything), ~(s + N') in
// the low word, as caf_mp_profile does.  No float atomics; an integer maximum does not depend on the order of arrival, so C,
// chosen from the number of rows to fill the device, changes no bit.
// Reproducibility: a row's arithmetic depends on the row and (N', L, P, g, a) alone; nothing is accumulated across rows; every
// byte of scratch is written before it is read.  A non-finite sample spoils its own row only.
#include "caf_internal.h"
#include "caf_ldsfft.h"
#include "caf_stage.h"
#include "caf_wave.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>

namespace caf {

namespace {

constexpr int SCF_THREADS = 256;
constexpr int SCF_MAX_CHUNK = 16;                  // pairs of one combined diagonal folded in registers before the integer maximum
constexpr int64_t SCF_SCRATCH = (int64_t)1 << 28;  // bytes of X per chunk of rows: inside the Infinity Cache
constexpr uint32_t SCF_NAN = 0x7FC00000u;

struct ScfArgs {
    const float2* x;
    int64_t pitch;
    int32_t np, hop, hops, m;  // N', L, P, M
    int32_t conjugate, coherence, chunk;
    const float* window;
    const float* smooth;
    float2* X;                 // (rows of the chunk, N', P)
    double* psd;               // (rows of the chunk, N')
    unsigned long long* keys;  // (rows of the chunk, A), or nullptr
    int64_t num_alpha;
    float* scf;
    float* alpha_val;
    int32_t* alpha_arg;
    double* out_psd;
};

// ---- demodulates ---------------------------------------------------------------------------------------------------------
template <int LOGN>
struct ScfDemodGeo {
    static constexpr int N = 1 << LOGN, NTR = N / 16, RPW = SCF_THREADS / NTR;
    static size_t lds(int hop) { return ((size_t)RPW * (N + N / 16) + (size_t)(RPW - 1) * hop + N) * sizeof(float2) + N * sizeof(float); }
};

template <int LOGN>
__global__ __launch_bounds__(SCF_THREADS) void k_scf_demod(const ScfArgs a, int64_t row0, const float2* __restrict__ tw) {
    using G = ScfDemodGeo<LOGN>;
    constexpr int N = G::N, NTR = G::NTR, RPW = G::RPW;
    extern __shared__ __attribute__((aligned(16))) float2 s_mem[];
    const int seg = (RPW - 1) * a.hop + N;  // the samples of the workgroup's RPW hops
    float2* s_x = s_mem + RPW * (N + N / 16);
    float* s_w = reinterpret_cast<float*>(s_x + seg);
    const int tid = threadIdx.x;
    const int rl = tid / NTR, l = tid - rl * NTR;
    float2* buf = s_mem + rl * (N + N / 16);
    const int r0 = blockIdx.x * RPW;  // (P is a multiple of RPW: every hop slot is a hop)
    const float2* xr = a.x + (row0 + blockIdx.y) * a.pitch + (int64_t)r0 * a.hop;
    stage_batched<4>(seg, [&](int t) { return xr[t]; }, [&](int t, float2 v) { s_x[t] = v; });
    stage_batched<1>(N, [&](int t) { return a.window[t]; }, [&](int t, float w) { s_w[t] = w; });
    __syncthreads();

    // forward = conj(IDFT(conj .)) on the shared inverse transform
    float2 v[16];
    const float2* xs = s_x + rl * a.hop;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int n = l + t * NTR;
        const float w = s_w[n];
        const float2 z = xs[n];
        v[t] = make_float2(w * z.x, -(w * z.y));
    }
    pd_fft<LOGN>(buf, tw, l, v);
    const int r = r0 + rl;
    const int rot = (r * a.hop) & (N - 1);
    float2* Xr = a.X + (int64_t)blockIdx.y * N * a.hops + r;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int m = pd_out_index<LOGN>(l, reg);             // the channel as an unsigned bin
        const int ph = (m * rot) & (N - 1);                   // (k (rL + n)) mod N' at n = 0: the absolute phase
        const float2 z = cmul(v[reg], tw[ph * (PD_TWN / N)]);  // conj(Y e^{+j}) = conj(Y) e^{-j}
        Xr[(int64_t)((m + N / 2) & (N - 1)) * a.hops] = make_float2(z.x, -z.y);
    }
}

template <int LOGN>
int scf_demod_launch(const ScfArgs& a, int64_t row0, int64_t nr, const float2* tw, hipStream_t st) {
    using G = ScfDemodGeo<LOGN>;
    const size_t lds = G::lds(a.hop);
    if (const int rc = allow_dynamic_lds(reinterpret_cast<const void*>(k_scf_demod<LOGN>), lds)) return rc;
    hipLaunchKernelGGL(k_scf_demod<LOGN>, dim3((unsigned)(a.hops / G::RPW), (unsigned)nr), dim3(SCF_THREADS), lds, st, a, row0, tw);
    return CAF_OK;
}

// ---- channel power -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SCF_THREADS) void k_scf_psd(const ScfArgs a, int64_t row0) {
    __shared__ double s_sum[SCF_THREADS / 64];
    const int c = blockIdx.x;
    const float2* xc = a.X + ((int64_t)blockIdx.y * a.np + c) * a.hops;
    double s = 0.0;
    for (int r = threadIdx.x; r < a.hops; r += SCF_THREADS) {
        const float2 z = xc[r];
        const double w = (double)z.x * (double)z.x + (double)z.y * (double)z.y;
        s += a.smooth ? (double)a.smooth[r] * w : w;
    }
    s = block_sum<SCF_THREADS / 64>(s, s_sum);
    if (threadIdx.x == 0) {
        a.psd[(int64_t)blockIdx.y * a.np + c] = s;
        if (a.out_psd) a.out_psd[(row0 + blockIdx.y) * a.np + c] = s;
    }
}

// ---- pairs ---------------------------------------------------------------------------------------------------------------
template <int LOGP>
struct ScfGeo {
    static constexpr int P = 1 << LOGP, NTR = P / 16, WG = NTR > 64 ? NTR : SCF_THREADS, RPW = WG / NTR;
    static constexpr size_t LDS = (size_t)RPW * (P + P / 16) * sizeof(float2);
};

// the product of the conjugate form: the same bits for (a, b) and (b, a), so that S(k, l, q) and S(l, k, q) -- equal by
// definition -- are equal on the device too and the profile's tie rule (the smaller s) decides between them
// (both products of each part are rounded before they are added: a contraction into an fma would round one of them only, and
// which one would depend on the order of the operands)
__device__ __forceinline__ float2 scf_mul_sym(float2 a, float2 b) {
#pragma clang fp contract(off)
    const float rr = a.x * b.x, ii = a.y * b.y, ri = a.x * b.y, ir = a.y * b.x;
    return make_float2(rr - ii, ri + ir);
}

// q + M/2 of the value that register `reg` of row-local thread l holds after pd_fft (the inverse kernel: register holds
// S(-m mod P) at m = pd_out_index), or -1 outside the tile
template <int LOGP>
__device__ __forceinline__ int scf_q(int l, int reg, int M) {
    constexpr int P = 1 << LOGP;
    const int f = (P - pd_out_index<LOGP>(l, reg)) & (P - 1);
    const int qo = (f < P / 2 ? f : f - P) + M / 2;
    return qo >= 0 && qo < M ? qo : -1;
}

template <int LOGP>
__global__ __launch_bounds__(ScfGeo<LOGP>::WG) void k_scf_pair(const ScfArgs a, int64_t row0, const float2* __restrict__ tw) {
    using G = ScfGeo<LOGP>;
    constexpr int P = G::P, NTR = G::NTR;
    extern __shared__ __attribute__((aligned(16))) float2 s_buf[];
    const int tid = threadIdx.x;
    const int rl = tid / NTR, l = tid - rl * NTR;
    float2* buf = s_buf + rl * (P + P / 16);
    const int N = a.np, H = N / 2, M = a.m, C = a.chunk;
    const int cpd = N / C;                         // chunks of a combined diagonal
    const int item = blockIdx.x * G::RPW + rl;     // (N cpd is a multiple of RPW: every slot is a chunk)
    const int e = item / cpd, c = item - e * cpd;  // combined diagonal e: the diagonal d' = e, then d' = e - N
    const float2* X = a.X + (int64_t)blockIdx.y * N * P;
    const double* psd = a.psd + (int64_t)blockIdx.y * N;
    unsigned long long* keys = a.keys ? a.keys + (int64_t)blockIdx.y * a.num_alpha : nullptr;
    const int64_t row = row0 + blockIdx.y;

    uint32_t bv[16];  // the running maximum of every bin this thread holds: the value's bits and the s of its pair
    int32_t bs[16];
    int cur = -1;     // d - dmin of the diagonal being folded
    auto flush = [&](int lj) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int qo = scf_q<LOGP>(lj, reg, M);
            if (qo >= 0) atomicMax(keys + (int64_t)cur * M + qo, ((unsigned long long)bv[reg] << 32) | (uint32_t)~(uint32_t)(bs[reg] + N));
        }
    };
    for (int j = c * C; j < (c + 1) * C; ++j) {
        const bool head = j < N - e;
        const int dp = head ? e : e - N, jj = head ? j : j - (N - e);  // pair jj of the diagonal d', in increasing s
        int k, ll, s;
        if (!a.conjugate) {  // d = d' = k - l
            ll = max(-H, -H - dp) + jj, k = ll + dp, s = k + ll;
        } else {  // d = d' - 1 = k + l
            k = max(-H, dp - H) + jj, ll = dp - 1 - k, s = k - ll;
        }
        // the twiddles and the LDS addresses are the same for every pair: made opaque per turn so that they are formed where
        // they are used and not kept in registers across the loop (k_cm_lds of caf_cyclo.hip)
        const float2* twj = tw;
        int lj = l;
        asm volatile("" : "+s"(twj), "+v"(lj));
        if (dp + N - 1 != cur) {
            if (keys && cur >= 0) flush(lj);
            cur = dp + N - 1;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) bv[reg] = 0u, bs[reg] = s;
        }
        float2 v[16];
        const float2* xk = X + (int64_t)(k + H) * P;
        const float2* xl = X + (int64_t)(ll + H) * P;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int r = lj + t * NTR;
            float2 y = xl[r];
            if (a.conjugate) {
                v[t] = scf_mul_sym(xk[r], y);
            } else {
                y.y = -y.y;
                v[t] = cmul(xk[r], y);
            }
            if (a.smooth) {
                const float g = a.smooth[r];
                v[t].x *= g, v[t].y *= g;
            }
        }
        pd_fft<LOGP>(buf, twj, lj, v);
        const double den = a.coherence ? psd[k + H] * psd[ll + H] : 1.0;
        float* cell = a.scf ? a.scf + ((row * N + (k + H)) * N + (ll + H)) * M : nullptr;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int qo = scf_q<LOGP>(lj, reg, M);
            if (qo >= 0) {
                const double w = (double)v[reg].x * (double)v[reg].x + (double)v[reg].y * (double)v[reg].y;
                const float val = den == 0.0 ? 0.0f : (float)(a.coherence ? w / den : w);
                const uint32_t bits = val != val ? SCF_NAN : __float_as_uint(val);
                if (cell) cell[qo] = __uint_as_float(bits);
                if (bits > bv[reg]) bv[reg] = bits, bs[reg] = s;
            }
        }
    }
    if (keys) flush(l);
}

template <int LOGP>
int scf_pair_launch(const ScfArgs& a, int64_t row0, int64_t nr, const float2* tw, hipStream_t st) {
    using G = ScfGeo<LOGP>;
    if (const int rc = allow_dynamic_lds(reinterpret_cast<const void*>(k_scf_pair<LOGP>), G::LDS)) return rc;
    const int64_t nwg = (int64_t)a.np * (a.np / a.chunk) / G::RPW;
    hipLaunchKernelGGL(k_scf_pair<LOGP>, dim3((unsigned)nwg, (unsigned)nr), dim3(G::WG), G::LDS, st, a, row0, tw);
    return CAF_OK;
}

// the profile from the keys: every bin has at least one pair, so every key was written
__global__ __launch_bounds__(SCF_THREADS) void k_scf_decode(const ScfArgs a, int64_t row0, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * SCF_THREADS + threadIdx.x;
    if (i >= count) return;
    const unsigned long long key = a.keys[i];
    const int64_t o = row0 * a.num_alpha + i;
    if (a.alpha_val) a.alpha_val[o] = __uint_as_float((uint32_t)(key >> 32));
    if (a.alpha_arg) a.alpha_arg[o] = (int32_t)(~(uint32_t)key) - a.np;
}

int scf_log2(int64_t n) {
    int l = 0;
    while (((int64_t)1 << l) < n) ++l;
    return l;
}
bool scf_pow2(int64_t n, int64_t lo, int64_t hi) { return n >= lo && n <= hi && (n & (n - 1)) == 0; }
bool scf_sizes_ok(int64_t np, int64_t hop, int64_t hops) {
    return scf_pow2(np, 64, 1024) && scf_pow2(hop, 1, np / 4) && scf_pow2(hops, 64, 16384) && hops * hop / np >= 2;
}

// CAF_SCF_DEBUG=1 (read per call, like CAF_CYCLO_DEBUG): one stderr line per caf_scf_fam call naming the forms that ran
bool scf_debug() {
    const char* e = std::getenv("CAF_SCF_DEBUG");
    return e && e[0] == '1';
}

}  // namespace

}  // namespace caf

using namespace caf;

int32_t caf_scf_geometry(int32_t num_channels, int32_t hop, int32_t num_hops, int32_t* m, int64_t* num_alpha, int64_t* min_samples,
                         int32_t* threads, int64_t* lds_bytes, int64_t* scratch_bytes_per_row) {
    CAF_REQUIRE(scf_sizes_ok(num_channels, hop, num_hops),
                "caf_scf_geometry: N' a power of two in 64 .. 1024, L a power of two in 1 .. N'/4, P a power of two in 64 .. 16384, P L / N' >= 2");
    const int64_t M = (int64_t)num_hops * hop / num_channels, A = (2 * (int64_t)num_channels - 1) * M;
    const int ntr = num_hops / 16, wg = ntr > 64 ? ntr : SCF_THREADS;
    if (m) *m = (int32_t)M;
    if (num_alpha) *num_alpha = A;
    if (min_samples) *min_samples = (int64_t)(num_hops - 1) * hop + num_channels;
    if (threads) *threads = wg;
    if (lds_bytes) *lds_bytes = (int64_t)(wg / ntr) * (num_hops + num_hops / 16) * (int64_t)sizeof(float2);
    if (scratch_bytes_per_row) *scratch_bytes_per_row = (int64_t)num_channels * num_hops * 8 + (int64_t)num_channels * 8 + A * 8;
    return CAF_OK;
}

int32_t caf_scf_fam(const caf_scf_desc* desc, const caf_scf_outputs* out) {
    CAF_REQUIRE(desc && out, "caf_scf_fam: NULL descriptor");
    const int64_t N = desc->num_channels, L = desc->hop, P = desc->num_hops;
    CAF_REQUIRE(scf_sizes_ok(N, L, P),
                "caf_scf_fam: N' a power of two in 64 .. 1024, L a power of two in 1 .. N'/4, P a power of two in 64 .. 16384, P L / N' >= 2");
    CAF_REQUIRE(desc->d_x && desc->d_window, "caf_scf_fam: d_x and d_window are required");
    CAF_REQUIRE(desc->rows >= 1 && desc->n >= 1 && desc->pitch >= desc->n && desc->pitch < ((int64_t)1 << 40),
                "caf_scf_fam: rows >= 1 and 1 <= n <= pitch");
    CAF_REQUIRE(desc->n >= (P - 1) * L + N, "caf_scf_fam: a row needs (P - 1) L + N' samples");
    CAF_REQUIRE((desc->conjugate | desc->coherence) >> 1 == 0, "caf_scf_fam: conjugate and coherence are 0 or 1");
    CAF_REQUIRE(out->d_scf || out->d_alpha_val || out->d_alpha_arg || out->d_psd, "caf_scf_fam: no output asked for");
    const int64_t M = P * L / N, A = (2 * N - 1) * M;
    CAF_REQUIRE(desc->rows * A < ((int64_t)1 << 40) && desc->rows * N * N < ((int64_t)1 << 50) / M, "caf_scf_fam: too many rows");
    hipStream_t st = (hipStream_t)desc->stream;
    const bool cells = out->d_scf != nullptr, profile = out->d_alpha_val || out->d_alpha_arg;

    ScfArgs a{};
    a.x = (const float2*)desc->d_x, a.pitch = desc->pitch, a.np = (int32_t)N, a.hop = (int32_t)L, a.hops = (int32_t)P, a.m = (int32_t)M;
    a.conjugate = desc->conjugate, a.coherence = desc->coherence, a.window = desc->d_window, a.smooth = desc->d_smooth;
    a.num_alpha = A, a.scf = out->d_scf, a.alpha_val = out->d_alpha_val, a.alpha_arg = out->d_alpha_arg, a.out_psd = out->d_psd;
    const int ntr = (int)P / 16, rpw = ntr > 64 ? 1 : SCF_THREADS / ntr;
    const int64_t chunk_rows = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(desc->rows, 65535), SCF_SCRATCH / (N * P * 8)));
    // pairs folded in registers per integer maximum: as many as still leave the device some thousand workgroups
    a.chunk = SCF_MAX_CHUNK;
    while (a.chunk > 1 && chunk_rows * (N * N / a.chunk) / rpw < 1024) a.chunk /= 2;

    int dev = 0;
    CAF_HIP_TRY(hipGetDevice(&dev));
    const float2* tw = nullptr;
    if (const int rc = lds_fft_twiddles(dev, &tw)) return rc;
    Scratch sc(st);
    if (const int rc = sc.get(&a.X, chunk_rows * N * P)) return rc;
    if (const int rc = sc.get(&a.psd, chunk_rows * N)) return rc;
    if (profile)
        if (const int rc = sc.get(&a.keys, chunk_rows * A)) return rc;
    for (int64_t r0 = 0; r0 < desc->rows; r0 += chunk_rows) {
        const int64_t nr = std::min(chunk_rows, desc->rows - r0);
        int rc = CAF_OK;
        switch (scf_log2(N)) {
#define SCF_CASE(LOGN)                                      \
    case LOGN:                                              \
        rc = scf_demod_launch<LOGN>(a, r0, nr, tw, st);     \
        break;
            SCF_CASE(6) SCF_CASE(7) SCF_CASE(8) SCF_CASE(9) SCF_CASE(10)
#undef SCF_CASE
        }
        if (rc) return rc;
        hipLaunchKernelGGL(k_scf_psd, dim3((unsigned)N, (unsigned)nr), dim3(SCF_THREADS), 0, st, a, r0);
        if (!cells && !profile) continue;
        if (profile) CAF_HIP_TRY(hipMemsetAsync(a.keys, 0, (size_t)(nr * A) * 8, st));
        switch (scf_log2(P)) {
#define SCF_CASE(LOGP)                                     \
    case LOGP:                                             \
        rc = scf_pair_launch<LOGP>(a, r0, nr, tw, st);     \
        break;
            SCF_CASE(6) SCF_CASE(7) SCF_CASE(8) SCF_CASE(9) SCF_CASE(10) SCF_CASE(11) SCF_CASE(12) SCF_CASE(13) SCF_CASE(14)
#undef SCF_CASE
        }
        if (rc) return rc;
        if (profile)
            hipLaunchKernelGGL(k_scf_decode, dim3(cdiv(nr * A, SCF_THREADS)), dim3(SCF_THREADS), 0, st, a, r0, nr * A);
    }
    if (scf_debug())
        std::fprintf(stderr, "[caf scf] fam np=%d hop=%d hops=%d m=%d rows=%lld conj=%d coh=%d demod=lds%d psd=f64 pair=%s chunk=%d out=%s%s%s\n",
                     (int)N, (int)L, (int)P, (int)M, (long long)desc->rows, desc->conjugate, desc->coherence, (int)N,
                     cells || profile ? ("lds" + std::to_string(P)).c_str() : "none", a.chunk, cells ? "cells," : "",
                     profile ? "profile," : "", "psd");
    CAF_HIP_TRY(hipGetLastError());
    return sc.finish();
}
