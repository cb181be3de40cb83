// WOLA polyphase channeliser (filterRoutines.wola / cpuWola.cpu_threaded_wola, filterRoutines.py:578-632, cpuWolaDll.c:38-178):
// for output row r (input sample n = r Dec) of N channels from L = P N real taps,
//   v[a]      = sum_{b < P} taps[b N + a] * xe[n - b N - a],            a < N  (xe: carried-in history, then x; zero before)
//   out[r][k] = sum_a v[a] e^{+j 2 pi a k / N}                            (unscaled inverse DFT, IPP NODIV)
//   N == 2 Dec and r odd: out[r][k] *= (-1)^k, i.e. v rotated by N/2 before the transform -- folded into the index v is
//   written at, so no extra pass.
//   * fused (k_wola): N a power of two 64..16384, P <= WOLA_FUSED_PMAX.  The polyphase sums land directly in the input
//     registers of the in-LDS transform (caf_ldsfft.h: thread l of a row holds branches l + t N/16, t < 16), the
//     transform runs in LDS, the row leaves once.  A workgroup holds consecutive rows; the overlapping input windows of
//     neighbouring rows are re-read from L1/L2.
//   * general (k_wola_poly + rocFFT rows): any N; the (rows, N) matrix of polyphase sums (rotation folded in) is
//     transformed in place by a batched backward rocFFT (caf_wola below).
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "caf_internal.h"
#include "caf_ldsfft.h"

namespace caf {

namespace {

constexpr int WOLA_FUSED_PMAX = 64;

// extended input: i in [-hlen, 0) -> carried-in history, [0, n) -> x, before the history 0 (i < n always holds here)
__device__ __forceinline__ float2 wola_xe(const float2* __restrict__ x, const float2* __restrict__ hist, int64_t hlen, int64_t i) {
    if (i >= 0) return x[i];
    return i >= -hlen ? hist[hlen + i] : make_float2(0.f, 0.f);
}

template <int LOGN>
__global__ __launch_bounds__((1 << LOGN) / 16 > 256 ? (1 << LOGN) / 16 : 256) void k_wola(
    const float2* __restrict__ x, const float2* __restrict__ hist, int64_t hlen, const float* __restrict__ taps, int32_t P,
    int32_t dec, int32_t layout, float2* __restrict__ out, int64_t rows, const float2* __restrict__ tw) {
    constexpr int N = 1 << LOGN, NTR = N / 16, WG = NTR > 256 ? NTR : 256, RPW = WG / NTR;
    extern __shared__ __attribute__((aligned(16))) float2 s_buf[];
    const int tid = threadIdx.x;
    const int rl = tid / NTR, l = tid - rl * NTR;
    float2* buf = s_buf + rl * (N + N / 16);
    const bool half = (dec * 2 == N);
    // one pass of RPW consecutive rows per workgroup.  (Walking 8 passes per workgroup, to keep a window resident longer,
    // hoisted state across the walk -- 155 -> 108 VGPRs at N = 1024 without it -- and took 2.04 ms against 0.90 at the
    // first shape of scripts/time_wola.py: profiles/r06/wola.log.)
    {
        // XCD-aware order: the dispatcher deals consecutive workgroups round-robin to the 8 XCDs, each with its own L2, so
        // neighbouring passes -- which share all but Dec of each row's L input samples -- would each fetch the window into
        // a different L2.  Workgroup b takes pass (b % 8) G8/8 + b / 8 instead (a bijection on the first G8 = G - G % 8
        // workgroups; the tail keeps its own index): every XCD walks one contiguous stretch of rows.
        const int64_t G = gridDim.x, G8 = G - G % 8, b = blockIdx.x;
        const int64_t pass = b < G8 ? (b % 8) * (G8 / 8) + b / 8 : b;
        const int64_t row0 = pass * RPW;
        const int64_t r = row0 + rl;
        const bool live = r < rows;  // dead row slots run the barriers on zeros
        const int64_t n = r * dec;
        float2 acc[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) acc[t] = make_float2(0.f, 0.f);
        if (live) {
            // deepest sample of the row: n - (P - 1) N - (N - 1); all inside x -> plain loads
            const int64_t lo = n - (int64_t)P * N + 1;
            if (lo >= 0) {
                const float2* xs = x + (n - l);
                const float* hs = taps + l;
                for (int b = 0; b < P; ++b) {
#pragma unroll
                    for (int t = 0; t < 16; ++t) {
                        const float h = hs[t * NTR];
                        const float2 v = xs[-(int64_t)t * NTR];
                        acc[t].x = fmaf(h, v.x, acc[t].x);
                        acc[t].y = fmaf(h, v.y, acc[t].y);
                    }
                    xs -= N;
                    hs += N;
                }
            } else {
                for (int b = 0; b < P; ++b) {
#pragma unroll
                    for (int t = 0; t < 16; ++t) {
                        const int a = l + t * NTR;
                        const float h = taps[(int64_t)b * N + a];
                        const float2 v = wola_xe(x, hist, hlen, n - (int64_t)b * N - a);
                        acc[t].x = fmaf(h, v.x, acc[t].x);
                        acc[t].y = fmaf(h, v.y, acc[t].y);
                    }
                }
            }
        }
        // odd rows with N == 2 Dec: transform input position i takes v[(i + N/2) mod N], i.e. register t takes t + 8
        float2 v[16];
        const bool rot = half && (r & 1);
#pragma unroll
        for (int t = 0; t < 16; ++t) v[t] = rot ? acc[(t + 8) & 15] : acc[t];
        pd_fft<LOGN>(buf, tw, l, v);
        if (layout == 0) {
            if (live) {
                float2* o = out + r * N;
#pragma unroll
                for (int q = 0; q < 16; ++q) o[pd_out_index<LOGN>(l, q)] = v[q];
            }
            // (no barrier: the last pass ends with one after its reads, the next row's first pass reads no image)
        } else {
            // channel-major: the RPW rows in flight go through LDS, so each channel's RPW consecutive rows leave together
#pragma unroll
            for (int q = 0; q < 16; ++q) buf[pd_pad(pd_out_index<LOGN>(l, q))] = v[q];
            __syncthreads();
            const int nlive = (int)((rows - row0) < RPW ? (rows - row0) : RPW);
            for (int e = tid; e < RPW * N; e += WG) {
                const int j = e % RPW, k = e / RPW;
                if (j < nlive) out[(int64_t)k * rows + row0 + j] = s_buf[j * (N + N / 16) + pd_pad(k)];
            }
            __syncthreads();
        }
    }
}

// general path, step 1: V[r][(a + N/2 rot) mod N] = v[a] for every row and branch (rotation folded into the index)
__global__ __launch_bounds__(256) void k_wola_poly(const float2* __restrict__ x, const float2* __restrict__ hist, int64_t hlen,
                                                  const float* __restrict__ taps, int32_t P, int32_t N, int32_t dec,
                                                  float2* __restrict__ V, int64_t rows) {
    const int64_t r = blockIdx.y + (int64_t)blockIdx.z * 65535;
    if (r >= rows) return;
    const int64_t n = r * dec;
    const bool rot = (dec * 2 == N) && (r & 1);
    for (int a = blockIdx.x * 256 + threadIdx.x; a < N; a += gridDim.x * 256) {
        float2 acc = make_float2(0.f, 0.f);
        for (int b = 0; b < P; ++b) {
            const int64_t i = n - (int64_t)b * N - a;
            if (i < -hlen) break;  // deeper taps only reach further back
            const float h = taps[(int64_t)b * N + a];
            const float2 v = wola_xe(x, hist, hlen, i);
            acc.x = fmaf(h, v.x, acc.x);
            acc.y = fmaf(h, v.y, acc.y);
        }
        const int dst = rot ? (a + N / 2) % N : a;
        V[r * N + dst] = acc;
    }
}

// general path, layout 1: (rows, N) -> (N, rows) through 32 x 32 LDS tiles
__global__ __launch_bounds__(256) void k_wola_transpose(const float2* __restrict__ src, int64_t rows, int32_t N,
                                                       float2* __restrict__ dst) {
    __shared__ float2 tile[32][33];
    const int64_t r0 = (int64_t)blockIdx.y * 32;
    const int k0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    for (int j = ty; j < 32; j += 8) {
        const int64_t r = r0 + j;
        const int k = k0 + tx;
        if (r < rows && k < N) tile[j][tx] = src[r * N + k];
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int k = k0 + j;
        const int64_t r = r0 + tx;
        if (r < rows && k < N) dst[(int64_t)k * rows + r] = tile[tx][j];
    }
}

template <int LOGN>
int wola_fused_launch(const float2* x, const float2* hist, int64_t hlen, const float* taps, int32_t P, int32_t dec,
                      int32_t layout, float2* out, int64_t rows, const float2* tw, hipStream_t st) {
    constexpr int N = 1 << LOGN, NTR = N / 16, WG = NTR > 256 ? NTR : 256, RPW = WG / NTR;
    const size_t lds = (size_t)RPW * (N + N / 16) * sizeof(float2);
    {
        const int rc_lds = allow_dynamic_lds(reinterpret_cast<const void*>(k_wola<LOGN>), lds);
        if (rc_lds) return rc_lds;
    }
    const int64_t nwg = (rows + RPW - 1) / RPW;
    CAF_REQUIRE(nwg <= 0x7fffffff, "caf_wola: too many rows for one launch");
    hipLaunchKernelGGL(k_wola<LOGN>, dim3((unsigned)nwg), dim3(WG), lds, st, x, hist, hlen, taps, P, dec, layout, out, rows, tw);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

bool wola_fused_ok(int32_t N, int64_t P) {
    return N >= 64 && N <= 16384 && (N & (N - 1)) == 0 && P >= 1 && P <= WOLA_FUSED_PMAX;
}

int launch_wola_fused(const float2* x, const float2* hist, int64_t hlen, const float* taps, int32_t P, int32_t N, int32_t dec,
                      int32_t layout, float2* out, int64_t rows, hipStream_t st) {
    int dev = 0;
    CAF_HIP_TRY(hipGetDevice(&dev));
    const float2* tw = nullptr;
    int rc = lds_fft_twiddles(dev, &tw);
    if (rc) return rc;
    switch (N) {
        case 64: return wola_fused_launch<6>(x, hist, hlen, taps, P, dec, layout, out, rows, tw, st);
        case 128: return wola_fused_launch<7>(x, hist, hlen, taps, P, dec, layout, out, rows, tw, st);
        case 256: return wola_fused_launch<8>(x, hist, hlen, taps, P, dec, layout, out, rows, tw, st);
        case 512: return wola_fused_launch<9>(x, hist, hlen, taps, P, dec, layout, out, rows, tw, st);
        case 1024: return wola_fused_launch<10>(x, hist, hlen, taps, P, dec, layout, out, rows, tw, st);
        case 2048: return wola_fused_launch<11>(x, hist, hlen, taps, P, dec, layout, out, rows, tw, st);
        case 4096: return wola_fused_launch<12>(x, hist, hlen, taps, P, dec, layout, out, rows, tw, st);
        case 8192: return wola_fused_launch<13>(x, hist, hlen, taps, P, dec, layout, out, rows, tw, st);
        case 16384: return wola_fused_launch<14>(x, hist, hlen, taps, P, dec, layout, out, rows, tw, st);
    }
    set_error("caf_wola: no fused kernel for this channel count");
    return CAF_ERR_INVALID;
}

int launch_wola_poly(const float2* x, const float2* hist, int64_t hlen, const float* taps, int32_t P, int32_t N, int32_t dec,
                     float2* V, int64_t rows, hipStream_t st) {
    const unsigned gx = (unsigned)std::min<int64_t>((N + 255) / 256, 64);
    const int64_t gz = (rows + 65534) / 65535;
    CAF_REQUIRE(gz <= 65535, "caf_wola: too many rows for one launch");
    const unsigned gy = (unsigned)std::min<int64_t>(rows, 65535);
    hipLaunchKernelGGL(k_wola_poly, dim3(gx, gy, (unsigned)gz), dim3(256), 0, st, x, hist, hlen, taps, P, N, dec, V, rows);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int launch_wola_transpose(const float2* src, int64_t rows, int32_t N, float2* dst, hipStream_t st) {
    const int64_t gy = (rows + 31) / 32;
    CAF_REQUIRE(gy <= 0x7fffffff, "caf_wola: too many rows for the transpose");
    hipLaunchKernelGGL(k_wola_transpose, dim3((unsigned)((N + 31) / 32), (unsigned)gy), dim3(256), 0, st, src, rows, N, dst);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

}  // namespace

}  // namespace caf

using namespace caf;

int32_t caf_wola(const float* d_x, int64_t n, const float* d_hist, int64_t hist_len, const float* d_taps, int64_t num_taps,
                 int32_t num_channels, int32_t dec, int32_t layout, float* d_out, int64_t rows, void* stream) {
    const int32_t N = num_channels;
    CAF_REQUIRE(N >= 1 && dec >= 1 && (N == dec || N == 2 * dec),
                "caf_wola: num_channels must equal dec or 2 * dec (the reference's phase correction)");
    CAF_REQUIRE(num_taps >= 1 && num_taps % N == 0, "caf_wola: num_taps must be a positive multiple of num_channels");
    CAF_REQUIRE(layout == 0 || layout == 1, "caf_wola: layout must be 0 (rows, N) or 1 (N, rows)");
    CAF_REQUIRE(n >= 0 && rows >= 0 && rows <= n / dec, "caf_wola: rows must be <= n / dec");
    CAF_REQUIRE(hist_len >= 0 && (hist_len == 0 || d_hist), "caf_wola: hist_len > 0 needs d_hist");
    if (rows == 0) return CAF_OK;
    CAF_REQUIRE(d_x && d_taps && d_out, "caf_wola: NULL buffer");
    const int64_t P = num_taps / N;
    CAF_REQUIRE(P <= 0x7fffffff, "caf_wola: too many taps");
    hipStream_t st = (hipStream_t)stream;
    const float2* x = (const float2*)d_x;
    const float2* h = (const float2*)d_hist;
    float2* out = (float2*)d_out;
    // CAF_WOLA_FUSED=0 forces the rocFFT rows (A/B and cross-checks); read per call like CAF_JIT
    const char* ef = std::getenv("CAF_WOLA_FUSED");
    const bool fused = wola_fused_ok(N, P) && !(ef && ef[0] == '0');
    if (const char* ed = std::getenv("CAF_WOLA_DEBUG"))
        if (ed[0] == '1')
            std::fprintf(stderr, "[caf wola] path=%s N=%d dec=%d P=%lld rows=%lld layout=%d\n", fused ? "fused" : "rocfft", (int)N,
                         (int)dec, (long long)P, (long long)rows, (int)layout);
    if (fused) return launch_wola_fused(x, h, hist_len, d_taps, (int32_t)P, N, dec, layout, out, rows, st);
    // general path: polyphase sums (rotation folded in) -> batched backward rocFFT in place -> (layout 1) transpose
    Scratch sc(st);
    float2* V = out;
    int rc;
    if (layout == 1 && (rc = sc.get(&V, rows * (int64_t)N))) return rc;
    if ((rc = launch_wola_poly(x, h, hist_len, d_taps, (int32_t)P, N, dec, V, rows, st))) return rc;
    if ((rc = fft_rows(V, V, rows, N, true, st))) return rc;
    if (layout == 1 && (rc = launch_wola_transpose(V, rows, N, out, st))) return rc;
    return sc.finish();
}
