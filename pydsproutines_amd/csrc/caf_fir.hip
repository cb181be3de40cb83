// gfx950 FIR family of the stand-alone toolbox: the direct-form kernels, the choice among them and the overlap-save forms
// of caf_firos.hip, and the entry points.  CDNA4 counterparts -- by semantics, not by code -- of the reference's
//   custom_kernels/filter.cu:9-181            filter_smtaps*  (lfilter semantics)
//   custom_kernels/upfirdn.cu:6-182           upfirdn_naive / upfirdn_sm
// HBM-bound or, for long FIRs, VALU-bound sliding-window work.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "caf_internal.h"
#include "caf_stage.h"

namespace caf {

// ---------------------------------------------------------------------------------------
// FIR == scipy.signal.lfilter(taps, 1, x) on complex64 with real float32 taps, optional carried-in
// history (`delay` = the dlen samples preceding x) and decimation out[k] = y[k*dsr + phase].
// Taps and the input window of the tile are staged in LDS.
// ---------------------------------------------------------------------------------------
constexpr int FIR_TILE = 1024;  // outputs (before decimation) per workgroup

__global__ __launch_bounds__(256) void k_fir(const float2* __restrict__ x, int64_t n, const float* __restrict__ taps,
                                             int32_t ntaps, const float2* __restrict__ delay, int32_t dlen,
                                             int32_t dsr, int32_t phase, float2* __restrict__ out, int64_t nout) {
    extern __shared__ float s_fir[];
    float* s_taps = s_fir;                                              // ntaps
    float2* s_in = reinterpret_cast<float2*>(s_fir + ((ntaps + 1) & ~1));  // FIR_TILE + ntaps - 1
    const int64_t i0 = (int64_t)blockIdx.x * FIR_TILE;  // first un-decimated output index of the tile
    for (int t = threadIdx.x; t < ntaps; t += 256) s_taps[t] = taps[t];
    const int span = FIR_TILE + ntaps - 1;
    stage_batched<8>(
        span,
        [&](int t) {
            const int64_t j = i0 - (ntaps - 1) + t;  // input index
            float2 v = make_float2(0.f, 0.f);
            if (j >= 0) {
                if (j < n) v = x[j];
            } else if (delay && -j <= dlen) {
                v = delay[dlen + j];
            }
            return v;
        },
        [&](int t, float2 v) { s_in[t] = v; });
    __syncthreads();
    for (int l = threadIdx.x; l < FIR_TILE; l += 256) {
        const int64_t i = i0 + l;
        if (i >= n) break;
        if (dsr > 1 && ((i - phase) % dsr != 0 || i < phase)) continue;
        float ar = 0.f, ai = 0.f;
        // y[i] = sum_k taps[k] x[i-k];  x[i-k] sits at s_in[l + ntaps-1 - k]
        const float2* w = s_in + l + ntaps - 1;
        for (int k = 0; k < ntaps; ++k) {
            const float c = s_taps[k];
            ar += c * w[-k].x;
            ai += c * w[-k].y;
        }
        const int64_t o = (i - phase) / dsr;
        if (o < nout) out[o] = make_float2(ar, ai);
    }
}

// Undecimated FIR, register-tiled: a thread produces FIRF_R consecutive outputs from a sliding window that lives
// in registers, so every tap costs one LDS read of a new sample + one (broadcast) read of the tap for FIRF_R complex
// FMAs -- the kernel above reads a tap and a sample per FMA and is bound by the LDS instruction rate.  The tap loop is
// unrolled by FIRF_R so that the window rotates through fixed register names (no moves).  The input window of the
// workgroup is stored transposed, element e at (e % FIRF_R) * pitch + e / FIRF_R: lanes, whose windows start
// FIRF_R samples apart, then read consecutive addresses (no bank conflicts).
constexpr int FIRF_R = 8;
constexpr int FIRF_TILE = 256 * FIRF_R;  // outputs per workgroup

__global__ __launch_bounds__(256) void k_fir_fast(const float2* __restrict__ x, int64_t n, const float* __restrict__ taps,
                                                  int32_t ntaps, const float2* __restrict__ delay, int32_t dlen,
                                                  float2* __restrict__ out) {
    extern __shared__ float s_firf[];
    const int ntp = (ntaps + FIRF_R - 1) / FIRF_R * FIRF_R;  // taps padded with zeros to a multiple of FIRF_R
    float* s_taps = s_firf;                                  // ntp
    float2* s_in = reinterpret_cast<float2*>(s_firf + ntp);  // FIRF_R rows of `pitch`
    const int span = FIRF_TILE + ntp;                        // samples i0 - ntp .. i0 + FIRF_TILE - 1
    const int pitch = span / FIRF_R + 1;
    const int64_t i0 = (int64_t)blockIdx.x * FIRF_TILE;
    for (int t = threadIdx.x; t < ntp; t += 256) s_taps[t] = t < ntaps ? taps[t] : 0.f;
    stage_batched<8>(
        span,
        [&](int t) {
            const int64_t j = i0 - ntp + t;
            float2 v = make_float2(0.f, 0.f);
            if (j >= 0) {
                if (j < n) v = x[j];
            } else if (delay && -j <= dlen) {
                v = delay[dlen + j];
            }
            return v;
        },
        [&](int t, float2 v) { s_in[(t % FIRF_R) * pitch + t / FIRF_R] = v; });
    __syncthreads();
    // outputs l0 .. l0 + R - 1 of the tile; sample index (tile-local, offset ntp) of output l and tap k: ntp + l - k
    const int l0 = threadIdx.x * FIRF_R;
    float2 acc[FIRF_R], win[FIRF_R];
#pragma unroll
    for (int r = 0; r < FIRF_R; ++r) {
        acc[r] = make_float2(0.f, 0.f);
        const int e = ntp + l0 + r;  // tap 0
        win[r] = s_in[(e % FIRF_R) * pitch + e / FIRF_R];
    }
    for (int k0 = 0; k0 < ntp; k0 += FIRF_R) {
#pragma unroll
        for (int kk = 0; kk < FIRF_R; ++kk) {
            const float c = s_taps[k0 + kk];
            // at tap k = k0 + kk output r needs sample e = ntp + l0 + r - k, held in win[(r - kk) mod R]
#pragma unroll
            for (int r = 0; r < FIRF_R; ++r) {
                const float2 w = win[(r - kk + FIRF_R) % FIRF_R];
                acc[r].x += c * w.x;
                acc[r].y += c * w.y;
            }
            // the sample of output R-1 (slot (R-1-kk) mod R) is not needed again: replace it with the one output 0
            // needs at the next tap, e = ntp + l0 - (k + 1)
            const int e = ntp + l0 - (k0 + kk + 1);
            win[(FIRF_R - 1 - kk) % FIRF_R] = s_in[((e % FIRF_R + FIRF_R) % FIRF_R) * pitch + e / FIRF_R];
        }
    }
#pragma unroll
    for (int r = 0; r < FIRF_R; ++r) {
        const int64_t i = i0 + l0 + r;
        if (i < n) out[i] = acc[r];
    }
}

// Decimating FIR (2 <= dsr <= FIRD_MAXDSR), optionally fused with the int16 IQ ingest (the front-end
// filter/decimate folded into the rx load): out[o] = y[o*dsr + phase], y = lfilter(taps, 1, scale * x).  Only the
// kept outputs are computed -- k_fir evaluates the tile un-decimated and leaves (dsr-1)/dsr of its lanes idle.
// A thread owns `per` kept outputs o0 + lane + r*256; the workgroup's input window is stored in polyphase order
// (element e at (e % dsr) * pitch + e / dsr), so that at every tap the lanes, whose samples are dsr apart, read
// consecutive LDS words.  TIn = float2 (complex64) or short2 (interleaved int16 IQ: 4 B read per sample).
constexpr int FIRD_MAXDSR = 16;
constexpr int FIRD_MAXPER = 4;

__device__ __forceinline__ float2 fird_load(const float2* p, int64_t i, float) { return p[i]; }
__device__ __forceinline__ float2 fird_load(const short2* p, int64_t i, float scale) {
    const short2 v = p[i];
    return make_float2((float)v.x * scale, (float)v.y * scale);
}

template <typename TIn>
__global__ __launch_bounds__(256) void k_fir_decim(const TIn* __restrict__ x, int64_t n, float scale,
                                                   const float* __restrict__ taps, int32_t ntaps,
                                                   const TIn* __restrict__ delay, int32_t dlen, int32_t dsr, int32_t phase,
                                                   int32_t per, float2* __restrict__ out, int64_t nout) {
    extern __shared__ float s_fird[];
    float* s_taps = s_fird;                                              // ntaps
    float2* s_in = reinterpret_cast<float2*>(s_fird + ((ntaps + 1) & ~1));  // dsr rows of `pitch`
    const int tile = 256 * per;                                          // kept outputs per workgroup
    const int span = (tile - 1) * dsr + ntaps;                           // inputs i0 .. i0 + span - 1
    const int pitch = span / dsr + 1;
    const int64_t o0 = (int64_t)blockIdx.x * tile;
    const int64_t i0 = o0 * dsr + phase - (ntaps - 1);                   // input index of window element 0
    for (int t = threadIdx.x; t < ntaps; t += 256) s_taps[t] = taps[t];
    stage_batched<(sizeof(TIn) == 8 ? 8 : 1)>(
        span,
        [&](int t) {
            const int64_t j = i0 + t;
            float2 v = make_float2(0.f, 0.f);
            if (j >= 0) {
                if (j < n) v = fird_load(x, j, scale);
            } else if (delay && -j <= dlen) {
                v = fird_load(delay, dlen + j, scale);
            }
            return v;
        },
        [&](int t, float2 v) { s_in[(t % dsr) * pitch + t / dsr] = v; });
    __syncthreads();
    // output l of the tile at tap k reads window element e = l*dsr + (ntaps-1-k): row (ntaps-1-k) % dsr,
    // column l + (ntaps-1-k) / dsr
    float2 acc[FIRD_MAXPER];
#pragma unroll
    for (int r = 0; r < FIRD_MAXPER; ++r) acc[r] = make_float2(0.f, 0.f);
    int m = ntaps - 1;
    int row = m % dsr, col = m / dsr;
    for (int k = 0; k < ntaps; ++k) {
        const float c = s_taps[k];
        const float2* w = s_in + row * pitch + col + threadIdx.x;
#pragma unroll
        for (int r = 0; r < FIRD_MAXPER; ++r) {
            if (r < per) {
                const float2 v = w[r * 256];
                acc[r].x += c * v.x;
                acc[r].y += c * v.y;
            }
        }
        if (--row < 0) {
            row = dsr - 1;
            --col;
        }
    }
#pragma unroll
    for (int r = 0; r < FIRD_MAXPER; ++r) {
        const int64_t o = o0 + threadIdx.x + r * 256;
        if (r < per && o < nout && o * dsr + phase < n) out[o] = acc[r];
    }
}

// Register-tiled decimating FIR for small decimation factors (window of the tile below ~7000 samples).  Polyphase
// view: with m = ntaps-1-k = q*dsr + rho, output l reads sample (l + q)*dsr + rho, i.e. column l + q of branch rho,
// so per branch the filter is a sliding dot product over columns with the sub-filter g_rho[q] = taps[ntaps-1-m]
// -- the structure of k_fir_fast.  A thread owns FIRP_R consecutive outputs and keeps their FIRP_R-column window of
// the current branch in registers (the q loop is unrolled by FIRP_R, the window rotates through fixed names): one LDS
// sample read and one broadcast tap read per FIRP_R complex-by-real MACs, 2.5x fewer LDS reads than k_fir_decim.
// Branch rows are stored with the columns transposed (c % FIRP_R major) so that lanes read consecutive words.
constexpr int FIRP_R = 4;
constexpr int FIRP_TILE = 256 * FIRP_R;
constexpr int FIRP_MAXSPAN = 7400;  // samples of the tile window (+ the tap table: < 64 KB of LDS)

// A workgroup walks tiles blockIdx.x, blockIdx.x + gridDim.x, ...: the next tile's window is fetched into REGISTERS (raw
// TIn: one register per int16 IQ sample) right after the barrier that hands the current one to the sliding dot products, so its
// round trips to memory run under a tile's worth of arithmetic instead of in front of it (one tile per workgroup: stage ->
// barrier -> compute, 62 % of the wave cycles parked; the launch now keeps as many workgroups as are resident).
__device__ __forceinline__ float2 fird_cvt(float2 v, float) { return v; }
__device__ __forceinline__ float2 fird_cvt(short2 v, float scale) { return make_float2((float)v.x * scale, (float)v.y * scale); }
template <typename TIn>
__device__ __forceinline__ TIn fird_zero();
template <>
__device__ __forceinline__ float2 fird_zero<float2>() { return make_float2(0.f, 0.f); }
template <>
__device__ __forceinline__ short2 fird_zero<short2>() { return make_short2(0, 0); }

// EPT: window elements a thread stages per tile (instantiated for 8 / 16 / 24 / 32: the prefetch registers of the shape at hand)
template <typename TIn, int NT, int EPT>
__global__ __launch_bounds__(NT) void k_fir_poly(const TIn* __restrict__ x, int64_t n, float scale,
                                                  const float* __restrict__ taps, int32_t ntaps,
                                                  const TIn* __restrict__ delay, int32_t dlen, int32_t dsr, int32_t phase,
                                                  float2* __restrict__ out, int64_t nout, int64_t ntiles) {
    extern __shared__ float s_firp[];
    const int qmax = (ntaps + dsr - 1) / dsr;                      // sub-filter length of branch 0 (the longest)
    const int qpad = (qmax + FIRP_R - 1) / FIRP_R * FIRP_R;        // padded with zero taps
    const int ncols = NT * FIRP_R + qpad;                            // columns per branch row
    const int pitch2 = ncols / FIRP_R + 1;
    const int rowpitch = FIRP_R * pitch2;
    float* s_g = s_firp;                                           // dsr * qpad sub-filter taps
    float2* s_x = reinterpret_cast<float2*>(s_firp + ((dsr * qpad + 1) & ~1));  // dsr rows of rowpitch
    for (int t = threadIdx.x; t < dsr * qpad; t += NT) {
        const int rho = t / qpad, q = t - rho * qpad;
        const int m = q * dsr + rho;
        s_g[t] = m < ntaps ? taps[ntaps - 1 - m] : 0.f;
    }
    // window element e = c*dsr + rho -> row rho, column c; a thread stages the elements tid, tid + NT, ...
    constexpr int MAXE = EPT;
    const int total = ncols * dsr;
    TIn pre[MAXE];
    auto fetch = [&](int64_t tile) {
        const int64_t i0 = tile * (NT * FIRP_R) * dsr + phase - (ntaps - 1);  // input index of window element 0
        // elements lo <= e < hi come from x (uniform base + 32-bit offsets), dl <= e < lo from the delay line, the rest are zeros
        const int lo = (int)std::min<int64_t>(std::max<int64_t>(-i0, 0), total), hi = (int)std::min<int64_t>(std::max<int64_t>(n - i0, 0), total);
        const int dl = delay ? (int)std::min<int64_t>(std::max<int64_t>(-i0 - dlen, 0), total) : lo;
        const TIn* xb = x + i0;
        const TIn* db = delay + (dlen + i0);
#pragma unroll
        for (int u = 0; u < MAXE; ++u) {
            const int e = (int)threadIdx.x + NT * u;
            TIn v = fird_zero<TIn>();
            if (e >= lo) {
                if (e < hi) v = xb[e];
            } else if (e >= dl) {
                v = db[e];
            }
            pre[u] = v;
        }
    };
    int64_t tile = blockIdx.x;
    if (tile < ntiles) fetch(tile);
    for (; tile < ntiles; tile += gridDim.x) {
        {   // (rho, c) advance without divisions
            int c = threadIdx.x / dsr, rho = threadIdx.x - c * dsr;
            const int dc = NT / dsr, dr = NT - dc * dsr;
#pragma unroll
            for (int u = 0; u < MAXE; ++u) {
                if ((int)threadIdx.x + NT * u < total) s_x[rho * rowpitch + (c % FIRP_R) * pitch2 + c / FIRP_R] = fird_cvt(pre[u], scale);
                c += dc;
                rho += dr;
                if (rho >= dsr) {
                    rho -= dsr;
                    ++c;
                }
            }
        }
        __syncthreads();
        if (tile + gridDim.x < ntiles) fetch(tile + gridDim.x);
        const int64_t o0 = tile * (NT * FIRP_R);
        float2 acc[FIRP_R];
#pragma unroll
        for (int r = 0; r < FIRP_R; ++r) acc[r] = make_float2(0.f, 0.f);
        for (int rho = 0; rho < dsr; ++rho) {
            const float2* xr = s_x + rho * rowpitch + threadIdx.x;  // column l0 + r + q with l0 = R * tid
            const float* g = s_g + rho * qpad;
            float2 win[FIRP_R];
#pragma unroll
            for (int r = 0; r < FIRP_R; ++r) win[r] = xr[r * pitch2];  // columns l0 + r (q = 0)
            for (int q0 = 0; q0 < qpad; q0 += FIRP_R) {
#pragma unroll
                for (int qq = 0; qq < FIRP_R; ++qq) {
                    const float c = g[q0 + qq];
                    // output r at q reads column l0 + r + q, held in slot (r + qq) mod R
#pragma unroll
                    for (int r = 0; r < FIRP_R; ++r) {
                        const float2 w = win[(r + qq) % FIRP_R];
                        acc[r].x += c * w.x;
                        acc[r].y += c * w.y;
                    }
                    // column l0 + q is done; slot qq takes column l0 + q + R
                    win[qq] = xr[qq * pitch2 + q0 / FIRP_R + 1];
                }
            }
        }
#pragma unroll
        for (int r = 0; r < FIRP_R; ++r) {
            const int64_t o = o0 + threadIdx.x * FIRP_R + r;
            if (o < nout && o * dsr + phase < n) out[o] = acc[r];
        }
        __syncthreads();  // the window is overwritten by the next tile
    }
}

// upfirdn == scipy.signal.upfirdn(taps, x, up, down) per row; out[r][o] = sum_k taps[k] xu[o*down - k],
// xu = x upsampled by `up` (zeros between samples).  Optional |.| output.
// The taps that meet a sample of x for output o are k = k0, k0 + up, ... with k0 = (o down) mod up, and they meet
// x[j0], x[j0 - 1], ... (j0 = (o down - k0) / up): one division per output, none per tap.
// STAGE: the workgroup's input window x[jlo .. jhi] (256 consecutive outputs: (255 down + ntaps) / up + 2 samples)
// is staged in LDS with coalesced loads (upfirdn.cu:68-182 does the same with its shared-memory window); without it
// every tap re-reads x from global memory.
template <bool STAGE>
__global__ __launch_bounds__(256) void k_upfirdn(const float2* __restrict__ x, int64_t n, const float* __restrict__ taps,
                                                 int32_t ntaps, int32_t up, int32_t down, int64_t nout, int32_t span,
                                                 float2* __restrict__ out, float* __restrict__ out_abs) {
    extern __shared__ float s_tp[];
    float2* s_x = reinterpret_cast<float2*>(s_tp + ((ntaps + 1) & ~1));
    for (int t = threadIdx.x; t < ntaps; t += 256) s_tp[t] = taps[t];
    const int64_t row = blockIdx.y;
    const float2* xr = x + row * n;
    const int64_t o0 = (int64_t)blockIdx.x * 256;
    // first sample any output of the workgroup can touch: floor((o0 down - (ntaps - 1)) / up), clipped below
    const int64_t plo = o0 * down - (ntaps - 1);
    const int64_t jlo = plo >= 0 ? plo / up : -((-plo + up - 1) / up);
    if (STAGE) {
        stage_batched<8>(span, [&](int i) { const int64_t j = jlo + i; return (j >= 0 && j < n) ? xr[j] : make_float2(0.f, 0.f); },
                         [&](int i, float2 v) { s_x[i] = v; });
    }
    __syncthreads();
    const int64_t o = o0 + threadIdx.x;
    if (o >= nout) return;
    const int64_t pos = o * down;  // index into the upsampled stream
    const int k0 = (int)(pos % up);
    int64_t j = (pos - k0) / up;
    float ar = 0.f, ai = 0.f;
    for (int k = k0; k < ntaps && j >= 0; k += up, --j) {
        if (j < n) {
            const float c = s_tp[k];
            const float2 v = STAGE ? s_x[j - jlo] : xr[j];
            ar += c * v.x;
            ai += c * v.y;
        }
    }
    if (out) out[row * nout + o] = make_float2(ar, ai);
    if (out_abs) out_abs[row * nout + o] = sqrtf(ar * ar + ai * ai);
}

// Polyphase form of the same filter for small interpolation factors (up <= 16).
// A thread owns one GROUP of `up` consecutive outputs o = g up + p, p = 0 .. up-1.  For phase p the taps are
// k0 + i up with k0 = (p down) mod up and the samples x[g down + c - i] with c = (p down) div up: within a wave the tap
// index is the same for every lane (one broadcast 16-byte LDS read serves four taps) and the sample index runs with the
// lane.  The window is stored by residue modulo `down` and the taps of a phase are walked residue by residue
// (i = i' down + rho), so that inside a residue both the sample column (tid + q0 - i') and the tap index (i') are
// linear: conflict-free reads at immediate offsets, no address arithmetic per tap.  Phases that share c (c is
// non-decreasing in p) share the samples, which are read once for up to four of them.  Against k_upfirdn this is ~3x
// fewer LDS reads per multiply-add, no per-lane tap addressing and no integer division per output.  The tile's
// 256 up outputs leave through LDS as whole rows.  (upfirdn.cu:68-182 keeps one output per thread.)
constexpr int UFP_MAXUP = 16;
template <int NP>
__device__ __forceinline__ void ufp_residue(const float2* __restrict__ xcol, const float* __restrict__ tp, int tp_phase_stride,
                                            int ntip, float (&ar)[4], float (&ai)[4]) {
    for (int i = 0; i < ntip; i += 4) {
        float2 xs[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) xs[u] = xcol[-(i + u)];
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const float4 t4 = *reinterpret_cast<const float4*>(tp + q * tp_phase_stride + i);
            ar[q] += t4.x * xs[0].x + t4.y * xs[1].x + t4.z * xs[2].x + t4.w * xs[3].x;
            ai[q] += t4.x * xs[0].y + t4.y * xs[1].y + t4.z * xs[2].y + t4.w * xs[3].y;
        }
    }
}
__global__ __launch_bounds__(256) void k_upfirdn_poly(const float2* __restrict__ x, int64_t n, const float* __restrict__ taps,
                                                      int32_t ntaps, int32_t up, int32_t down, int64_t nout, int32_t ntip,
                                                      int32_t pitch, int32_t span, float2* __restrict__ out,
                                                      float* __restrict__ out_abs) {
    extern __shared__ __attribute__((aligned(16))) float s_ufp[];
    float* s_tp = s_ufp;                                             // [up][down][ntip] taps, zero-padded
    float2* s_x = reinterpret_cast<float2*>(s_tp + up * down * ntip);  // [down][pitch] window by residue
    float2* s_out = s_x + down * pitch;                              // [256][up] outputs of the tile
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.y;
    const float2* xr = x + row * n;
    const int64_t gg0 = (int64_t)blockIdx.x * 256;                   // first group of the workgroup
    const int i_max = ntip * down - 1;                               // largest (padded) tap number of a phase
    for (int e = tid; e < up * down * ntip; e += 256) {
        const int ip = e % ntip, pr = e / ntip;                      // pr = p * down + rho
        const int rho = pr % down, p = pr / down;
        const int k = (p * down) % up + (ip * down + rho) * up;
        s_tp[e] = k < ntaps ? taps[k] : 0.f;
    }
    const int64_t jlo = gg0 * down - i_max;
    for (int idx = tid; idx < span; idx += 256) {
        const int64_t j = jlo + idx;
        const int q = idx / down, r = idx - q * down;
        s_x[r * pitch + q] = (j >= 0 && j < n) ? xr[j] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    for (int p = 0; p < up;) {
        const int c = (p * down) / up;
        int np = 1;
        while (np < 4 && p + np < up && ((p + np) * down) / up == c) ++np;  // phases p .. p+np-1 share their samples
        float ar[4] = {0.f, 0.f, 0.f, 0.f}, ai[4] = {0.f, 0.f, 0.f, 0.f};
        for (int rho = 0; rho < down; ++rho) {
            // tap i = i' down + rho reads window index tid down + (c + i_max - rho) - i' down
            const int e = c + i_max - rho;
            const int eq = e / down, er = e - eq * down;
            const float2* xcol = s_x + er * pitch + eq + tid;
            const float* tp = s_tp + (p * down + rho) * ntip;
            if (np == 1) ufp_residue<1>(xcol, tp, down * ntip, ntip, ar, ai);
            else if (np == 2) ufp_residue<2>(xcol, tp, down * ntip, ntip, ar, ai);
            else if (np == 3) ufp_residue<3>(xcol, tp, down * ntip, ntip, ar, ai);
            else ufp_residue<4>(xcol, tp, down * ntip, ntip, ar, ai);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < np) s_out[tid * up + p + q] = make_float2(ar[q], ai[q]);
        p += np;
    }
    __syncthreads();
    const int64_t o0 = gg0 * up;
    for (int e = tid; e < 256 * up; e += 256) {
        const int64_t o = o0 + e;
        if (o < nout) {
            const float2 v = s_out[e];
            if (out) out[row * nout + o] = v;
            if (out_abs) out_abs[row * nout + o] = sqrtf(v.x * v.x + v.y * v.y);
        }
    }
}

// interleaved int16 IQ -> complex64 (usrpRoutines.simpleBinRead's .astype(float32).view(complex64),
// usrpRoutines.py:51-67, done on the device as in benchmarks/benchmark_cupyCopyAndConvert.py:17-25):
// 4 B read + 8 B write per sample; one thread converts 4 samples (16-B load, 2 x 16-B stores).
__global__ __launch_bounds__(256) void k_iq16_to_c64(const short* __restrict__ in, int64_t nsamp, float scale,
                                                     float2* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * 256 * 4;
    for (int64_t s = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; s < nsamp; s += stride) {
        if (s + 4 <= nsamp) {
            const short4 a = *reinterpret_cast<const short4*>(in + 2 * s);
            const short4 b = *reinterpret_cast<const short4*>(in + 2 * s + 4);
            float4 o0 = make_float4(a.x * scale, a.y * scale, a.z * scale, a.w * scale);
            float4 o1 = make_float4(b.x * scale, b.y * scale, b.z * scale, b.w * scale);
            *reinterpret_cast<float4*>(out + s) = o0;
            *reinterpret_cast<float4*>(out + s + 2) = o1;
        } else {
            for (int64_t k = s; k < nsamp; ++k) out[k] = make_float2(in[2 * k] * scale, in[2 * k + 1] * scale);
        }
    }
}

static bool fir_decim_ok(int32_t ntaps, int32_t dsr) { return dsr >= 1 && dsr <= FIRD_MAXDSR && ntaps <= 2048; }
// the register-tiled polyphase form (k_fir_poly) applies: its tile window of 1024 kept outputs fits the LDS
static size_t fir_poly_lds(int32_t ntaps, int32_t dsr, int* ncols_out) {
    const int qmax = (ntaps + dsr - 1) / dsr;
    const int qpad = (qmax + FIRP_R - 1) / FIRP_R * FIRP_R;
    const int ncols = FIRP_TILE + qpad;
    if (ncols_out) *ncols_out = ncols;
    return (size_t)((dsr * qpad + 1) & ~1) * sizeof(float) + (size_t)dsr * FIRP_R * (ncols / FIRP_R + 1) * sizeof(float2);
}
static bool fir_poly_fits(int32_t ntaps, int32_t dsr) {
    int ncols = 0;
    const size_t smp = fir_poly_lds(ntaps, dsr, &ncols);
    return dsr >= 1 && smp <= 64 * 1024 && (size_t)ncols * dsr <= (size_t)FIRP_MAXSPAN + 4 * FIRP_R * dsr;
}

// (the launchers of the FIR family return the name of the kernel they chose: the CAF_FIR_DEBUG report below)
template <typename TIn>
static const char* launch_fir_decim(const TIn* x, int64_t n, float scale, const float* taps, int32_t ntaps, const TIn* delay,
                                    int32_t dlen, int32_t dsr, int32_t phase, float2* out, int64_t nout, hipStream_t st) {
    if (nout <= 0) return "none";
    {   // register-tiled polyphase form when its tile window fits the LDS (small decimation factors)
        int ncols = 0;
        const size_t smp = fir_poly_lds(ntaps, dsr, &ncols);
        if (fir_poly_fits(ntaps, dsr)) {
            // (Tiles of 512 outputs on 128 threads -- half the LDS, twice the independent workgroups per CU, the same waves -- measured
            //  the same as 1024 on 256 with one tile per workgroup: 55.8 / 56.1 us for 2^24 int16 samples, 64 taps, dsr 4
            //  (profiles/r05/ab_fir_poly_nt.log).)
            // resident workgroups: what the LDS holds per CU, at most 16 waves' worth of registers (CAF_FIR_POLY_WGS: per CU, A/B)
            static const int wgs_env = [] {
                const char* e = getenv("CAF_FIR_POLY_WGS");
                return e ? atoi(e) : 0;
            }();
            static const int ncu = [] {
                int dev = 0, c = 256;
                (void)hipGetDevice(&dev);
                (void)hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev);
                return c;
            }();
            const int64_t ntiles = cdiv(nout, FIRP_TILE);
            const int ept = (ncols * dsr + 255) / 256;
            // the grid is what is RESIDENT (tiles are dealt by striding: a workgroup that waits for a slot would start its share late)
            auto resident = [&](const void* kern) {
                thread_local std::map<std::pair<const void*, size_t>, int> cache;
                auto it = cache.find({kern, smp});
                if (it != cache.end()) return it->second;
                int nb = 1;
                if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, 256, smp) != hipSuccess || nb < 1) nb = 1;
                cache[{kern, smp}] = nb;
                return nb;
            };
#define CAF_FIR_POLY(E)                                                                                                            \
    do {                                                                                                                           \
        const int per_cu = wgs_env > 0 ? wgs_env : resident(reinterpret_cast<const void*>(&k_fir_poly<TIn, 256, E>));                \
        const dim3 grid((unsigned)std::min<int64_t>(ntiles, (int64_t)ncu * per_cu));                                               \
        hipLaunchKernelGGL((k_fir_poly<TIn, 256, E>), grid, dim3(256), smp, st, x, n, scale, taps, ntaps, delay, dlen, dsr, phase, \
                           out, nout, ntiles);                                                                                     \
    } while (0)
            if (ept <= 8) CAF_FIR_POLY(8); else if (ept <= 16) CAF_FIR_POLY(16); else if (ept <= 24) CAF_FIR_POLY(24); else CAF_FIR_POLY(32);
#undef CAF_FIR_POLY
            return ept <= 8 ? "fir_poly E=8" : (ept <= 16 ? "fir_poly E=16" : (ept <= 24 ? "fir_poly E=24" : "fir_poly E=32"));
        }
    }
    // kept outputs per thread: the window (tile - 1) * dsr + ntaps stays below ~6200 samples (LDS < 64 KB with the taps)
    const int per = dsr <= 4 ? 4 : (dsr <= 8 ? 2 : 1);
    const int tile = 256 * per;
    const int span = (tile - 1) * dsr + ntaps;
    const size_t sm = (size_t)((ntaps + 1) & ~1) * sizeof(float) + (size_t)dsr * (span / dsr + 1) * sizeof(float2);
    if (nout > 0)
        hipLaunchKernelGGL(k_fir_decim<TIn>, dim3(cdiv(nout, tile)), dim3(256), sm, st, x, n, scale, taps, ntaps, delay,
                           dlen, dsr, phase, per, out, nout);
    return "fir_decim";
}

static const char* launch_fir(const float2* x, int64_t n, const float* taps, int32_t ntaps, const float2* delay, int32_t dlen,
                int32_t dsr, int32_t phase, float2* out, int64_t nout, hipStream_t st) {
    if (dsr == 1 && phase == 0 && nout >= n && ntaps <= 2048) {  // undecimated: the register-tiled kernel (LDS < 64 KB)
        const int ntp = (ntaps + FIRF_R - 1) / FIRF_R * FIRF_R;
        const int pitch = (FIRF_TILE + ntp) / FIRF_R + 1;
        const size_t smf = (size_t)ntp * sizeof(float) + (size_t)FIRF_R * pitch * sizeof(float2);
        hipLaunchKernelGGL(k_fir_fast, dim3(cdiv(n, FIRF_TILE)), dim3(256), smf, st, x, n, taps, ntaps, delay, dlen, out);
        return "fir_fast";
    }
    if (fir_decim_ok(ntaps, dsr))  // decimating: only the kept outputs are computed
        return launch_fir_decim(x, n, 1.0f, taps, ntaps, delay, dlen, dsr, phase, out, nout, st);
    const size_t sm = (size_t)((ntaps + 1) & ~1) * sizeof(float) + (size_t)(FIR_TILE + ntaps) * sizeof(float2);
    hipLaunchKernelGGL(k_fir, dim3(cdiv(n, FIR_TILE)), dim3(256), sm, st, x, n, taps, ntaps, delay, dlen, dsr, phase, out,
                       nout);
    return "fir";
}

static const char* launch_upfirdn(const float2* x, int64_t rows, int64_t n, const float* taps, int32_t ntaps, int32_t up, int32_t down,
                    int64_t nout, float2* out, float* out_abs, hipStream_t st) {
    if (up <= UFP_MAXUP) {
        // polyphase form: 256 groups of `up` outputs per workgroup; taps of a phase split by residue of the tap number
        const int nt = (ntaps - 1) / up + 1;                          // taps per phase
        const int ntip = ((nt + down - 1) / down + 3) & ~3;           // per residue, padded to whole 16-byte reads
        const int cmax = (int)(((int64_t)(up - 1) * down) / up);
        const int64_t span = 255 * (int64_t)down + cmax + (int64_t)ntip * down;
        const int64_t pitch = span / down + 2;
        const size_t lds = (size_t)up * down * ntip * sizeof(float) + (size_t)down * pitch * sizeof(float2) +
                           (size_t)256 * up * sizeof(float2);
        if (lds <= 64 * 1024) {
            const int64_t ngroups = (nout + up - 1) / up;
            hipLaunchKernelGGL(k_upfirdn_poly, dim3(cdiv(ngroups, 256), (unsigned)rows), dim3(256), lds, st, x, n, taps, ntaps, up,
                               down, nout, ntip, (int32_t)pitch, (int32_t)span, out, out_abs);
            return "upfirdn_poly";
        }
    }
    // input window of 256 consecutive outputs; staged in LDS when it fits beside the taps (<= 64 KB)
    const int64_t span = (255 * (int64_t)down + ntaps - 1) / up + 3;
    const size_t tap_bytes = (size_t)((ntaps + 1) & ~1) * sizeof(float);
    if (tap_bytes + (size_t)span * sizeof(float2) <= 64 * 1024) {
        hipLaunchKernelGGL(k_upfirdn<true>, dim3(cdiv(nout, 256), (unsigned)rows), dim3(256),
                           tap_bytes + (size_t)span * sizeof(float2), st, x, n, taps, ntaps, up, down, nout, (int32_t)span, out,
                           out_abs);
        return "upfirdn_lds";
    }
    hipLaunchKernelGGL(k_upfirdn<false>, dim3(cdiv(nout, 256), (unsigned)rows), dim3(256), tap_bytes, st, x, n, taps,
                       ntaps, up, down, nout, 0, out, out_abs);
    return "upfirdn_global";
}

}  // namespace caf

using namespace caf;

namespace {

// Overlap-save FIR (caf_firos.hip).  Direct form costs ntaps multiply-adds per KEPT output, overlap-save ~130 flops
// per full-rate output: measured on 2^24 samples it is level with the direct kernels at ~96 taps per unit of
// decimation (0.10 vs 0.14 ms at 128 taps, dsr 1; 0.10 vs 0.11 ms at 256 taps, dsr 4) and ahead beyond, and it is the
// only form for tap sets longer than the direct kernels' LDS windows.  CAF_FIR_OS_MIN_TAPS overrides the 96
// (A/B switch; 0 = always).
bool fir_use_overlap_save(int32_t ntaps, int32_t dsr, int32_t direct_limit) {
    static const int min_taps = [] {
        const char* e = getenv("CAF_FIR_OS_MIN_TAPS");
        return e ? atoi(e) : 96;
    }();
    // decimation factors beyond the register-tiled polyphase kernel's window run on k_fir_decim (a tap and a sample read from LDS
    // per multiply-add): level with overlap-save at 64 taps, half its speed at 128 (2^24 int16 samples, /8: 133 against 77 us) --
    // there the 96 taps count as such, not per unit of decimation
    if (dsr >= 2 && !fir_poly_fits(ntaps, dsr) && ntaps >= std::max(min_taps, 1) && fir_os_fused_block(ntaps)) return true;
    return ntaps > direct_limit || (int64_t)ntaps > (int64_t)min_taps * dsr;
}

// CAF_FIR_DEBUG=1 (read per call, like CAF_WOLA_DEBUG): one stderr line per caf_fir_lfilter / caf_iq16_fir_decimate /
// caf_upfirdn call naming the kernel that ran (and the transform length B of the overlap-save forms), so that a test can
// assert the path it means to test
bool fir_debug() {
    const char* e = std::getenv("CAF_FIR_DEBUG");
    return e && e[0] == '1';
}
void fir_report(const char* call, bool is_iq16, const char* kernel, int64_t B, int32_t ntaps, int32_t up, int32_t dsr,
                int32_t phase, int64_t rows, int64_t n, int64_t nout) {
    char blk[32] = "";
    if (B) std::snprintf(blk, sizeof(blk), " B=%lld", (long long)B);
    std::fprintf(stderr, "[caf fir] call=%s path=%s%s%s ntaps=%d up=%d down=%d phase=%d rows=%lld n=%lld out=%lld\n", call,
                 is_iq16 ? "iq16_" : "", kernel, blk, (int)ntaps, (int)up, (int)dsr, (int)phase, (long long)rows, (long long)n,
                 (long long)nout);
}

// is_iq16: x / delay are interleaved int16 IQ pairs scaled by `scale`, else complex64
int fir_overlap_save(const void* x, int64_t n, bool is_iq16, float scale, const float* taps, int32_t ntaps, const void* delay,
                     int32_t dlen, int32_t dsr, int32_t phase, float2* out, int64_t nout, hipStream_t st) {
    const char* call = is_iq16 ? "iq16_fir_decimate" : "fir_lfilter";
    if (nout <= 0) {
        if (fir_debug()) fir_report(call, is_iq16, "none", 0, ntaps, 1, dsr, phase, 1, n, nout);
        return CAF_OK;
    }
    Scratch sc(st);
    int rc;
    if (const int fb = fir_os_fused_block(ntaps)) {
        if (fir_debug()) fir_report(call, is_iq16, "os_fused", fb, ntaps, 1, dsr, phase, 1, n, nout);
        float2* ht = nullptr;
        if ((rc = sc.get(&ht, fb))) return rc;
        rc = is_iq16 ? launch_iq16_fir_os_fused((const int16_t*)x, n, scale, taps, ntaps, (const int16_t*)delay, dlen, dsr, phase,
                                                out, nout, ht, st)
                     : launch_fir_os_fused((const float2*)x, n, taps, ntaps, (const float2*)delay, dlen, dsr, phase, out, nout,
                                           ht, st);
        if (rc) return rc;
    } else {
        // long tap sets: rocFFT rows of B >= 4 ntaps points (>= 75 % new outputs per block)
        int64_t B = 65536;
        while (B < 4 * (int64_t)ntaps) B <<= 1;
        CAF_REQUIRE(B <= ((int64_t)1 << 26), "overlap-save FIR: more than 2^24 taps");
        if (fir_debug()) fir_report(call, is_iq16, "os_rocfft", B, ntaps, 1, dsr, phase, 1, n, nout);
        const int64_t L = B - ntaps + 1;
        const int64_t last = phase + (nout - 1) * (int64_t)dsr;
        const int64_t nblk = last / L + 1;
        const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nblk, 65535), ((int64_t)1 << 25) / B));
        float2 *rows = nullptr, *hrow = nullptr;
        if ((rc = sc.get(&rows, chunk * B)) || (rc = sc.get(&hrow, B))) return rc;
        launch_fos_taps_pad(taps, ntaps, B, hrow, st);
        if ((rc = fft_rows(hrow, hrow, 1, B, false, st))) return rc;
        for (int64_t b0 = 0; b0 < nblk; b0 += chunk) {
            const int64_t nb = std::min(chunk, nblk - b0);
            if (is_iq16)
                launch_fos_gather_iq16((const int16_t*)x, n, scale, (const int16_t*)delay, dlen, b0, nb, L, B, ntaps, rows, st);
            else
                launch_fos_gather((const float2*)x, n, (const float2*)delay, dlen, b0, nb, L, B, ntaps, rows, st);
            if ((rc = fft_rows(rows, rows, nb, B, false, st))) return rc;
            launch_rows_mul_vec(rows, B, 0, hrow, B, rows, B, B, nb, 1.0f / (float)B, st);
            if ((rc = fft_rows(rows, rows, nb, B, true, st))) return rc;
            launch_fos_scatter(rows, b0, nb, L, B, ntaps, dsr, phase, out, nout, st);
        }
    }
    return sc.finish();
}

}  // namespace

int32_t caf_fir_lfilter(const float* d_x, int64_t n, const float* d_taps, int32_t num_taps, const float* d_delay,
                        int32_t delay_len, int32_t dsr, int32_t ds_phase, float* d_out, int64_t out_len, void* stream) {
    CAF_REQUIRE(d_x && d_taps && d_out && n >= 1 && num_taps >= 1, "caf_fir_lfilter: bad arguments");
    CAF_REQUIRE(dsr >= 1 && ds_phase >= 0 && ds_phase < dsr, "dsPhase must be between in the range [0,dsr-1].");
    CAF_REQUIRE(delay_len >= 0 && (delay_len == 0 || d_delay), "delay_len > 0 needs d_delay");
    CAF_REQUIRE(out_len >= 0 && out_len <= (n - ds_phase + dsr - 1) / dsr, "caf_fir_lfilter: out_len exceeds len(x[dsPhase::dsr])");
    if (fir_use_overlap_save(num_taps, dsr, 4096))  // long tap sets: frequency-domain blocks (any length)
        return fir_overlap_save(d_x, n, false, 1.0f, d_taps, num_taps, d_delay, delay_len, dsr, ds_phase, (float2*)d_out, out_len,
                                (hipStream_t)stream);
    const char* kernel = launch_fir((const float2*)d_x, n, d_taps, num_taps, (const float2*)d_delay, delay_len, dsr, ds_phase,
                                    (float2*)d_out, out_len, (hipStream_t)stream);
    if (fir_debug()) fir_report("fir_lfilter", false, kernel, 0, num_taps, 1, dsr, ds_phase, 1, n, out_len);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_iq16_fir_decimate(const int16_t* d_iq, int64_t num_samples, float scale, const float* d_taps, int32_t num_taps,
                              const int16_t* d_delay, int32_t delay_len, int32_t dsr, int32_t ds_phase, float* d_out,
                              int64_t out_len, void* stream) {
    CAF_REQUIRE(d_iq && d_taps && d_out && num_samples >= 1 && num_taps >= 1, "caf_iq16_fir_decimate: bad arguments");
    CAF_REQUIRE(dsr >= 1 && ds_phase >= 0 && ds_phase < dsr, "dsPhase must be between in the range [0,dsr-1].");
    CAF_REQUIRE(delay_len >= 0 && (delay_len == 0 || d_delay), "delay_len > 0 needs d_delay");
    CAF_REQUIRE(((uintptr_t)d_iq & 3) == 0 && ((uintptr_t)d_delay & 3) == 0, "caf_iq16_fir_decimate: IQ pairs must be 4-byte aligned");
    CAF_REQUIRE(out_len >= 0 && out_len <= (num_samples - ds_phase + dsr - 1) / dsr,
                "caf_iq16_fir_decimate: out_len exceeds len(x[dsPhase::dsr])");
    // direct polyphase form: <= 2048 taps and dsr <= 16; anything else (and long tap sets) goes overlap-save
    if (!fir_decim_ok(num_taps, dsr) || fir_use_overlap_save(num_taps, dsr, 2048))
        return fir_overlap_save(d_iq, num_samples, true, scale, d_taps, num_taps, d_delay, delay_len, dsr, ds_phase,
                                (float2*)d_out, out_len, (hipStream_t)stream);
    const char* kernel = launch_fir_decim(reinterpret_cast<const short2*>(d_iq), num_samples, scale, d_taps, num_taps,
                                          reinterpret_cast<const short2*>(d_delay), delay_len, dsr, ds_phase, (float2*)d_out,
                                          out_len, (hipStream_t)stream);
    if (fir_debug()) fir_report("iq16_fir_decimate", true, kernel, 0, num_taps, 1, dsr, ds_phase, 1, num_samples, out_len);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_upfirdn(const float* d_x, int64_t rows, int64_t n, const float* d_taps, int32_t num_taps, int32_t up,
                    int32_t down, float* d_out, float* d_out_abs, int64_t out_len, void* stream) {
    CAF_REQUIRE(d_x && d_taps && (d_out || d_out_abs) && rows >= 1 && rows <= 65535 && n >= 1, "caf_upfirdn: bad arguments");
    CAF_REQUIRE(num_taps >= 1 && num_taps <= 16384 && up >= 1 && down >= 1, "caf_upfirdn: bad taps/up/down");
    const int64_t full = ((n - 1) * up + num_taps + down - 1) / down;
    CAF_REQUIRE(out_len >= 1 && out_len <= full, "caf_upfirdn: out_len larger than the full upfirdn length");
    // up == 1 is a FIR with decimation: full-convolution outputs [0 :: down] (zeros beyond the input).  From 96 taps per unit of
    // decimation on, the overlap-save form (caf_firos.hip: the rows are blockIdx.y of ONE launch) -- 64 x 262144 samples, 128
    // taps, up = down = 1: 0.38 ms through the polyphase kernel (0.09 of the HBM bound), the same job as caf_fir_lfilter otherwise
    if (up == 1 && d_out && !d_out_abs && fir_os_fused_block(num_taps) && fir_use_overlap_save(num_taps, down, 1 << 30)) {
        hipStream_t st = (hipStream_t)stream;
        const int fb = fir_os_fused_block(num_taps);  // (launch_fir_os_fused picks its kernel by the same function)
        if (fir_debug()) fir_report("upfirdn", false, "os_fused", fb, num_taps, 1, down, 0, rows, n, out_len);
        Scratch sc(st);
        float2* ht = nullptr;
        int rc = sc.get(&ht, fb);
        if (rc) return rc;
        rc = launch_fir_os_fused((const float2*)d_x, n, d_taps, num_taps, nullptr, 0, down, 0, (float2*)d_out, out_len, ht, st, rows, n,
                                 out_len);
        if (rc) return rc;
        return sc.finish();
    }
    const char* kernel = launch_upfirdn((const float2*)d_x, rows, n, d_taps, num_taps, up, down, out_len, (float2*)d_out, d_out_abs,
                                        (hipStream_t)stream);
    if (fir_debug()) fir_report("upfirdn", false, kernel, 0, num_taps, up, down, 0, rows, n, out_len);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_iq16_to_c64(const int16_t* d_iq, int64_t num_samples, float scale, float* d_out, void* stream) {
    CAF_REQUIRE(d_iq && d_out && num_samples >= 0, "caf_iq16_to_c64: bad arguments");
    CAF_REQUIRE((reinterpret_cast<uintptr_t>(d_iq) & 7) == 0 && (reinterpret_cast<uintptr_t>(d_out) & 15) == 0,
                "caf_iq16_to_c64: d_iq must be 8-byte and d_out 16-byte aligned");
    if (num_samples > 0)
        hipLaunchKernelGGL(k_iq16_to_c64, dim3(std::min<unsigned>(cdiv(num_samples, 1024), 8192)), dim3(256), 0, (hipStream_t)stream,
                           d_iq, num_samples, scale, (float2*)d_out);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}
