// CP2FSK demodulation (demodulationRoutines.py:20-37, 1214-1330: demodulateCP2FSK / cupyDemodulateCP2FSK and
// BurstyDemodulatorCP2FSK.demod).  With g[n] = exp(j pi h n / up), n < up (float64 on the host, rounded once to float32):
//   c0[i] = |sum_n x[i + n] g[n]|, c1[i] = |sum_n x[i + n] conj(g[n])|, bit[i] = c1[i] > c0[i], m[i] = max(c0[i], c1[i]).
//
//   k_cp2fsk_tone    one workgroup per tile of positions i = start + k step: the tile's samples and the tone in LDS, one pass
//                    over n for both sums -- x g and x conj(g) share the four real products xr gr, xi gi, xr gi, xi gr.
//   k_cp2fsk_comb    c[i] = sum_{j < burst_len} m[i + j up]: a moving sum along each of the up polyphase branches, per tile in
//                    LDS with a halo of (burst_len - 1) up values (from global memory where that halo does not fit), float64.
//   k_cp2fsk_costs   costs[k] = sum_b c[search_start + k + burst_starts[b]]; k_cp2fsk_costs_tile the same from a tile of c in
//                    LDS where the bursts' span fits one (c is then read about twice instead of once per burst).
//   k_argmax_f64     first-occurrence arg max of a row of float64 (chunks, then the chunks' winners).
//   k_cp2fsk_gather  dbits[b][j] = bit[mi + burst_starts[b] + j up].
//
// Summation order (fixed, a function of the position alone): the four products of one position are each accumulated by one
// fmaf chain over n = 0 .. up - 1 in float32; then one difference and one sum per component and one magnitude
// (sqrt(re^2 + im^2) on operands scaled by an exact power of two).  Everything after that is float64: a comb value is the sum of
// its burst_len terms in increasing j at the first row of a segment of its branch, and from there one addition and one
// subtraction per step; a cost adds its bursts' comb values in the order of burst_starts.
// Floating-point contraction is off in this file: every product and sum below is rounded where it is written.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "caf_internal.h"
#include "caf_wave.h"

#pragma clang fp contract(off)

namespace caf {

namespace {

constexpr int CT = 256;                // threads per workgroup
constexpr int CP_MAX_UP = 256;         // samples per symbol
constexpr int TONE_PPT = 4;            // positions per thread
constexpr int TONE_TILE = CT * TONE_PPT;
constexpr int TONE_SPAN = 4096;        // staged samples of a tile with step > 1 (32 KiB + padding)
constexpr int COMB_CAP = 12288;        // floats of one comb tile and its halo in LDS (48 KiB: three workgroups per CU)
constexpr int COMB_MIN_TILE = 2048;    // a halo that leaves fewer outputs than this is read from global memory instead
constexpr int COMB_GLOBAL_TILE = 8192;
constexpr int COST_T = 1024;           // threads of the tiled cost kernel
constexpr int COST_CAP = 16384;        // comb values of one cost tile and the bursts' span in LDS (128 KiB: one workgroup per CU)
constexpr int COST_MIN_TILE = 4096;    // a span that leaves fewer outputs than this, or fewer than COST_MIN_BURSTS bursts: no tile
constexpr int COST_MIN_BURSTS = 4;
constexpr int COST_MAX_BURSTS = 4096;  // ... or more than this (their offsets are staged in LDS, 16 KiB)
constexpr int COST_PPT = COST_CAP / COST_T;
constexpr int AM_CHUNK = CT * 32;      // elements per workgroup of the first arg max stage

constexpr int REL_ARGS = 128;          // burst starts that travel as kernel arguments (more are uploaded)

struct Tones {
    float2 g[CP_MAX_UP];
};

// the burst starts less the smallest one: in the kernel arguments, or (d != NULL) in device memory
struct Rel {
    int64_t r[REL_ARGS];
    const int64_t* d;
    __device__ __forceinline__ int64_t operator[](int b) const { return d ? d[b] : r[b]; }
};

// a tile read at a stride keeps 32 consecutive samples and then skips one slot: positions step apart fall on different banks
template <bool PAD>
__device__ __forceinline__ int lds_at(int i) {
    return PAD ? i + (i >> 5) : i;
}

// |re + j im|: both operands scaled by the same exact power of two, so two roundings in the radicand and one in the root
__device__ __forceinline__ float cabs32(float re, float im) {
    const float ax = fabsf(re), ay = fabsf(im);
    const float hi = ax > ay ? ax : ay;
    if (!(hi > 0.f) || isinf(hi)) return isnan(ax) || isnan(ay) ? ax + ay : hi;
    const int e = ilogbf(hi);
    const float sr = ldexpf(re, -e), si = ldexpf(im, -e);
    return ldexpf(sqrtf(fmaf(sr, sr, si * si)), e);
}

template <bool PAD>
__global__ __launch_bounds__(CT) void k_cp2fsk_tone(const float2* __restrict__ x, int64_t rows, int64_t xlength, int up, int64_t start,
                                                    int64_t step, int64_t count, int tile, const Tones tn, float* __restrict__ c0,
                                                    float* __restrict__ c1, float* __restrict__ mx, uint8_t* __restrict__ bits) {
    extern __shared__ float4 s_dyn[];
    float2* s_g = (float2*)s_dyn;
    float2* s_x = s_g + CP_MAX_UP;
    const int tid = threadIdx.x;
    const int64_t k0 = (int64_t)blockIdx.x * tile;
    const int npos = (int)std::min<int64_t>(tile, count - k0);
    const int istep = (int)step;  // (a tile of more than one position has step <= TONE_SPAN)
    const int span = (npos - 1) * istep + up;
    if (tid < up) s_g[tid] = tn.g[tid];
    for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
        // the tile's samples: x[row][start + k0 step ...], span of them, all inside the row (checked on the host)
        const float2* src = x + row * xlength + start + k0 * step;
        const int head = (int)((((uintptr_t)src) >> 3) & 1);  // one sample up to the 16-byte boundary
        if (tid == 0 && head) s_x[lds_at<PAD>(0)] = src[0];
        const int pairs = (span - head) >> 1;
        const float4* src4 = (const float4*)(src + head);
        for (int q = tid; q < pairs; q += CT) {
            const float4 v = src4[q];
            s_x[lds_at<PAD>(head + 2 * q)] = make_float2(v.x, v.y);
            s_x[lds_at<PAD>(head + 2 * q + 1)] = make_float2(v.z, v.w);
        }
        if (tid == 0 && ((span - head) & 1)) s_x[lds_at<PAD>(span - 1)] = src[span - 1];
        __syncthreads();

        int base[TONE_PPT];
        float a[TONE_PPT], b[TONE_PPT], c[TONE_PPT], d[TONE_PPT];
#pragma unroll
        for (int j = 0; j < TONE_PPT; j++) {
            const int p = tid + j * CT;
            base[j] = (p < npos ? p : npos - 1) * istep;  // (a thread without a position repeats the last one and stores nothing)
            a[j] = b[j] = c[j] = d[j] = 0.f;
        }
        for (int n = 0; n < up; n++) {
            const float2 g = s_g[n];
#pragma unroll
            for (int j = 0; j < TONE_PPT; j++) {
                const float2 v = s_x[lds_at<PAD>(base[j] + n)];
                a[j] = fmaf(v.x, g.x, a[j]);
                b[j] = fmaf(v.y, g.y, b[j]);
                c[j] = fmaf(v.x, g.y, c[j]);
                d[j] = fmaf(v.y, g.x, d[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < TONE_PPT; j++) {
            const int p = tid + j * CT;
            if (p >= npos) continue;
            const float m0 = cabs32(a[j] - b[j], c[j] + d[j]);  // x g
            const float m1 = cabs32(a[j] + b[j], d[j] - c[j]);  // x conj(g)
            const int64_t o = row * count + k0 + p;
            if (c0) c0[o] = m0;
            if (c1) c1[o] = m1;
            if (mx) mx[o] = m1 > m0 ? m1 : m0;
            if (bits) bits[o] = (uint8_t)(m1 > m0);  // a tie is bit 0
        }
        __syncthreads();  // the tile goes to the next row
    }
}

// c[row][o] = sum_{j < L} m[row][first + o + j up], o < clen
template <bool LDS>
__global__ __launch_bounds__(CT) void k_cp2fsk_comb(const float* __restrict__ m, int64_t pitch, int64_t first, int64_t rows, int up, int L,
                                                    int64_t clen, int tile, double* __restrict__ c) {
    extern __shared__ float4 s_dyn[];
    const float* s_m = (const float*)s_dyn;
    const int tid = threadIdx.x;
    const int64_t o0 = (int64_t)blockIdx.x * tile;
    const int nout = (int)std::min<int64_t>(tile, clen - o0);
    const int64_t halo = (int64_t)(L - 1) * up;
    // one work item = one segment of one polyphase branch: the first window is summed, the following ones slide
    const int nseg = up < CT ? CT / up : 1;
    const int R = (nout + up - 1) / up;
    const int seg = (R + nseg - 1) / nseg;
    for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
        const float* src = m + row * pitch + first + o0;  // src[0, nout + halo) lies inside the row (checked on the host)
        if constexpr (LDS) {
            float* s_w = (float*)s_dyn;
            const int n = nout + (int)halo;
            for (int i = tid; i < n; i += CT) s_w[i] = src[i];
            __syncthreads();
        }
        auto at = [&](int64_t i) -> double {
            if constexpr (LDS) return (double)s_m[(int)i];
            else return (double)src[i];
        };
        double* out = c + row * clen + o0;
        for (int item = tid; item < up * nseg; item += CT) {
            const int p = item % up, s = item / up;
            const int r0 = s * seg, r1 = std::min(r0 + seg, R);
            int o = r0 * up + p;
            if (r0 >= r1 || o >= nout) continue;
            double sum = 0.0;
            for (int j = 0; j < L; j++) sum += at((int64_t)o + (int64_t)j * up);
            out[o] = sum;
            for (int r = r0 + 1; r < r1; r++) {
                o += up;
                if (o >= nout) break;
                sum = (sum + at((int64_t)o + halo)) - at((int64_t)o - up);
                out[o] = sum;
            }
        }
        if constexpr (LDS) __syncthreads();
    }
}

// costs[row][k] = sum_b c[row][k + rel[b]]
__global__ __launch_bounds__(CT) void k_cp2fsk_costs(const double* __restrict__ c, int64_t clen, int64_t rows, const Rel rel, int nb,
                                                     int64_t S, double* __restrict__ costs) {
    const int64_t k = (int64_t)blockIdx.x * CT + threadIdx.x;
    if (k >= S) return;
    for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
        const double* cr = c + row * clen + k;
        double acc = 0.0;
        for (int b = 0; b < nb; b++) {
            const int64_t off = rel[b];
            if (k + off < clen) acc += cr[off];  // (always true for arguments that passed the host checks)
        }
        costs[row * S + k] = acc;
    }
}

// The same sums in the same order, from a tile of nout <= tile outputs and the span = max(rel) values behind them in LDS; the
// offsets are staged there too (one broadcast read per burst, shared by a thread's outputs k = t, t + 1024, ...).
__global__ __launch_bounds__(COST_T) void k_cp2fsk_costs_tile(const double* __restrict__ c, int64_t clen, int64_t rows, const Rel rel,
                                                              int nb, int64_t S, int tile, int span, double* __restrict__ costs) {
    extern __shared__ float4 s_dyn[];
    double* s_c = (double*)s_dyn;
    int* s_rel = (int*)(s_c + COST_CAP);
    const int tid = threadIdx.x;
    const int64_t k0 = (int64_t)blockIdx.x * tile;
    const int nout = (int)std::min<int64_t>(tile, S - k0);
    const int n = nout + span;  // k0 + n <= S + span = clen
    for (int b = tid; b < nb; b += COST_T) {
        const int64_t off = rel[b];
        s_rel[b] = off <= span ? (int)off : span;  // (span is the largest of them)
    }
    for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
        const double* cr = c + row * clen + k0;
        for (int i = tid; i < n; i += COST_T) s_c[i] = cr[i];
        __syncthreads();
        int at[COST_PPT];
        double acc[COST_PPT];
#pragma unroll
        for (int q = 0; q < COST_PPT; q++) {
            const int k = tid + q * COST_T;
            at[q] = k < nout ? k : nout - 1;  // (a slot without an output repeats the last one and stores nothing)
            acc[q] = 0.0;
        }
        for (int b = 0; b < nb; b++) {
            const int off = s_rel[b];
#pragma unroll
            for (int q = 0; q < COST_PPT; q++)
                if (q * COST_T < nout) acc[q] += s_c[at[q] + off];
        }
#pragma unroll
        for (int q = 0; q < COST_PPT; q++) {
            const int k = tid + q * COST_T;
            if (k < nout) costs[row * S + k0 + k] = acc[q];
        }
        __syncthreads();
    }
}

// Arg max of v[row][0, n), the first index among equal maxima (caf_wave.h); a NaN never wins.  Workgroup blockIdx.x takes the
// elements [blockIdx.x chunk, ...) and leaves its winner at [row][blockIdx.x].  idx_in: the indices the values stand for (the
// winners of a first stage, in increasing order of index), NULL for 0, 1, 2, ...  With out_final the winner is written as
// add + index, and an index outside [0, limit) -- a row with nothing but NaN -- as add.
__global__ __launch_bounds__(CT) void k_argmax_f64(const double* __restrict__ v, const int64_t* __restrict__ idx_in, int64_t n, int64_t rows,
                                                   int64_t chunk, double* __restrict__ pv, int64_t* __restrict__ pi,
                                                   int64_t* __restrict__ out_final, int64_t add, int64_t limit) {
    __shared__ WaveSlots<CT / 64, double, long long> s_best;
    const int64_t e0 = (int64_t)blockIdx.x * chunk, e1 = std::min(n, e0 + chunk);
    for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
        double bv = -INFINITY;
        long long bi = INT64_MAX;
        for (int64_t e = e0 + threadIdx.x; e < e1; e += CT) {
            const double val = v[row * n + e];
            const long long i = idx_in ? (long long)idx_in[row * n + e] : (long long)e;
            if (first_max(bv, bi, val, i)) {
                bv = val;
                bi = i;
            }
        }
        block_argmax(s_best, bv, bi);
        if (threadIdx.x == 0) {
            const int64_t o = row * gridDim.x + blockIdx.x;
            if (pv) pv[o] = bv;
            if (pi) pi[o] = (int64_t)bi;
            if (out_final) out_final[row] = add + ((bi >= 0 && bi < limit) ? (int64_t)bi : 0);
        }
        __syncthreads();
    }
}

// out[row][b L + j] = bits[row][(mi[row] - search_start) + rel[b] + j up]
__global__ __launch_bounds__(CT) void k_cp2fsk_gather(const uint8_t* __restrict__ bits, int64_t bpitch, int64_t rows,
                                                      const int64_t* __restrict__ mi, int64_t search_start, const Rel rel, int nb, int L,
                                                      int up, uint8_t* __restrict__ out) {
    const int64_t total = (int64_t)nb * L;
    for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
        const int64_t at = mi[row] - search_start;
        for (int64_t t = (int64_t)blockIdx.x * CT + threadIdx.x; t < total; t += (int64_t)gridDim.x * CT) {
            const int64_t b = t / L, j = t - b * L;
            const int64_t off = at + rel[(int)b] + j * up;
            out[row * total + t] = (off >= 0 && off < bpitch) ? bits[row * bpitch + off] : (uint8_t)0;  // (always inside after the host checks)
        }
    }
}

unsigned rows_grid(int64_t rows) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(rows, 65535)); }

int tone_tile(int up, int64_t step) {
    if (step == 1) return TONE_TILE;
    if (step > TONE_SPAN - up) return 1;
    return (int)std::min<int64_t>(TONE_TILE, (TONE_SPAN - up) / step + 1);
}

// the caller has checked: 1 <= up <= CP_MAX_UP, start >= 0, step >= 1, count >= 1, start + (count - 1) step + up <= xlength
int launch_tone(const float2* x, int64_t rows, int64_t xlength, int up, double h, int64_t start, int64_t step, int64_t count, float* c0,
                float* c1, float* mx, uint8_t* bits, hipStream_t st) {
    Tones tn;
    for (int n = 0; n < CP_MAX_UP; n++) {
        const double ph = M_PI * h * (double)n / (double)up;
        tn.g[n] = n < up ? make_float2((float)std::cos(ph), (float)std::sin(ph)) : make_float2(0.f, 0.f);
    }
    const int tile = tone_tile(up, step);
    const int span = (int)((tile - 1) * step) + up;
    const int64_t tiles = (count + tile - 1) / tile;
    const dim3 grid((unsigned)tiles, rows_grid(rows));
    if (step == 1) {
        const size_t bytes = (size_t)(CP_MAX_UP + span) * sizeof(float2);
        hipLaunchKernelGGL(k_cp2fsk_tone<false>, grid, dim3(CT), bytes, st, x, rows, xlength, up, start, step, count, tile, tn, c0, c1, mx, bits);
    } else {
        const size_t bytes = (size_t)(CP_MAX_UP + span + (span >> 5) + 1) * sizeof(float2);
        hipLaunchKernelGGL(k_cp2fsk_tone<true>, grid, dim3(CT), bytes, st, x, rows, xlength, up, start, step, count, tile, tn, c0, c1, mx, bits);
    }
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

// what the host knows of a set of burst starts: the range they span and, for the kernels, each start less the smallest
struct Bursts {
    int64_t lo = 0, hi = 0;
    Rel rel;
};

int check_comb(int64_t rows, int64_t length, int32_t up, int32_t burst_len, const int64_t* burst_starts, int32_t num_bursts,
               int64_t search_start, int64_t search_count, int64_t tail, Bursts* bu) {
    CAF_REQUIRE(rows >= 0 && length >= 1 && length <= ((int64_t)1 << 31) - 1, "caf cp2fsk: rows must be >= 0 and the row length in [1, 2^31)");
    CAF_REQUIRE(up >= 1 && up <= CP_MAX_UP, "caf cp2fsk: up must be in [1, 256]");
    CAF_REQUIRE(burst_len >= 1 && num_bursts >= 1 && burst_starts != nullptr, "caf cp2fsk: burst_len and num_bursts must be >= 1");
    CAF_REQUIRE(search_start >= 0 && search_count >= 1 && search_count <= length && search_start <= length, "caf cp2fsk: search range");
    CAF_REQUIRE(burst_len <= length, "caf cp2fsk: the bursts extend past the row");
    int64_t lo = burst_starts[0], hi = burst_starts[0];
    for (int b = 1; b < num_bursts; b++) {
        lo = std::min(lo, burst_starts[b]);
        hi = std::max(hi, burst_starts[b]);
    }
    CAF_REQUIRE(lo >= 0 && hi <= length, "caf cp2fsk: burst starts must lie inside the row");
    // every term is at most 2^39 here, so the sum cannot overflow; tail = the samples one value needs beyond its position
    CAF_REQUIRE(search_start + search_count - 1 + hi + (int64_t)(burst_len - 1) * up + tail < length,
                "caf cp2fsk: the search range and the bursts extend past the row");
    bu->lo = lo;
    bu->hi = hi;
    return CAF_OK;
}

// up to REL_ARGS bursts ride in the kernel arguments and nothing waits; a longer list is uploaded, which waits for the stream once
int pass_rel(const int64_t* burst_starts, int32_t num_bursts, Bursts* bu, Scratch& sc, hipStream_t st) {
    bu->rel.d = nullptr;
    for (int b = 0; b < REL_ARGS; b++) bu->rel.r[b] = b < num_bursts ? burst_starts[b] - bu->lo : 0;
    if (num_bursts <= REL_ARGS) return CAF_OK;
    std::vector<int64_t> rel(num_bursts);
    for (int b = 0; b < num_bursts; b++) rel[b] = burst_starts[b] - bu->lo;
    int64_t* d = nullptr;
    if (const int rc = sc.get(&d, num_bursts)) return rc;
    bu->rel.d = d;
    return host_h2d(d, rel.data(), (int64_t)num_bursts * 8, st);
}

// comb, costs: m[row][first + ...] with first = the position of search_start + the smallest burst start in the row
int launch_comb_costs(const float* m, int64_t pitch, int64_t first, int64_t rows, int up, int L, const Bursts& bu, int nb, int64_t S,
                      double* d_c, double* costs, hipStream_t st) {
    const int64_t clen = S + (bu.hi - bu.lo), halo = (int64_t)(L - 1) * up;
    if (halo <= COMB_CAP - COMB_MIN_TILE) {
        const int tile = COMB_CAP - (int)halo;
        hipLaunchKernelGGL(k_cp2fsk_comb<true>, dim3((unsigned)((clen + tile - 1) / tile), rows_grid(rows)), dim3(CT), COMB_CAP * sizeof(float),
                           st, m, pitch, first, rows, up, L, clen, tile, d_c);
    } else {
        const int tile = COMB_GLOBAL_TILE;
        hipLaunchKernelGGL(k_cp2fsk_comb<false>, dim3((unsigned)((clen + tile - 1) / tile), rows_grid(rows)), dim3(CT), 0, st, m, pitch, first,
                           rows, up, L, clen, tile, d_c);
    }
    CAF_HIP_TRY(hipGetLastError());
    const int64_t span = bu.hi - bu.lo;
    if (nb >= COST_MIN_BURSTS && nb <= COST_MAX_BURSTS && span <= COST_CAP - COST_MIN_TILE) {
        const int tile = COST_CAP - (int)span;
        const size_t bytes = COST_CAP * sizeof(double) + (size_t)nb * sizeof(int);
        if (const int rc = allow_dynamic_lds((const void*)k_cp2fsk_costs_tile, bytes)) return rc;
        hipLaunchKernelGGL(k_cp2fsk_costs_tile, dim3((unsigned)((S + tile - 1) / tile), rows_grid(rows)), dim3(COST_T), bytes, st, d_c, clen,
                           rows, bu.rel, nb, S, tile, (int)span, costs);
    } else {
        hipLaunchKernelGGL(k_cp2fsk_costs, dim3((unsigned)((S + CT - 1) / CT), rows_grid(rows)), dim3(CT), 0, st, d_c, clen, rows, bu.rel, nb,
                           S, costs);
    }
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

}  // namespace

}  // namespace caf

using namespace caf;

int32_t caf_cp2fsk_tone_metric(const float* d_x, int64_t rows, int64_t xlength, int32_t up, double h, int64_t start, int64_t step,
                               int64_t count, float* d_c0, float* d_c1, float* d_max, uint8_t* d_bits, void* stream) {
    CAF_REQUIRE(up >= 1 && up <= CP_MAX_UP, "caf_cp2fsk_tone_metric: up must be in [1, 256]");
    CAF_REQUIRE(rows >= 0 && xlength >= 1 && xlength <= ((int64_t)1 << 31) - 1, "caf_cp2fsk_tone_metric: rows must be >= 0 and xlength in [1, 2^31)");
    CAF_REQUIRE(start >= 0 && start <= xlength && step >= 1 && step <= xlength && count >= 1 && count <= xlength,
                "caf_cp2fsk_tone_metric: start, step and count");
    CAF_REQUIRE(start + (count - 1) * step + up <= xlength, "caf_cp2fsk_tone_metric: the positions extend past the row");
    CAF_REQUIRE(std::isfinite(h), "caf_cp2fsk_tone_metric: h must be finite");
    if (rows == 0) return CAF_OK;
    CAF_REQUIRE(d_x != nullptr, "caf_cp2fsk_tone_metric: NULL input");
    if (!d_c0 && !d_c1 && !d_max && !d_bits) return CAF_OK;
    return launch_tone((const float2*)d_x, rows, xlength, up, h, start, step, count, d_c0, d_c1, d_max, d_bits, (hipStream_t)stream);
}

int32_t caf_cp2fsk_comb_costs(const float* d_max, int64_t rows, int64_t mlength, int32_t up, int32_t burst_len, const int64_t* burst_starts,
                              int32_t num_bursts, int64_t search_start, int64_t search_count, double* d_costs, void* stream) {
    Bursts bu;
    if (const int rc = check_comb(rows, mlength, up, burst_len, burst_starts, num_bursts, search_start, search_count, 0, &bu)) return rc;
    if (rows == 0) return CAF_OK;
    CAF_REQUIRE(d_max && d_costs, "caf_cp2fsk_comb_costs: NULL buffer");
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    double* d_c = nullptr;
    int rc = sc.get(&d_c, rows * (search_count + bu.hi - bu.lo));
    if (rc) return rc;
    if ((rc = pass_rel(burst_starts, num_bursts, &bu, sc, st))) return rc;
    if ((rc = launch_comb_costs(d_max, mlength, search_start + bu.lo, rows, up, burst_len, bu, num_bursts, search_count, d_c, d_costs, st)))
        return rc;
    return sc.finish();
}

int32_t caf_cp2fsk_bursty_demod(const float* d_x, int64_t rows, int64_t xlength, int32_t up, double h, int32_t burst_len,
                                const int64_t* burst_starts, int32_t num_bursts, int64_t search_start, int64_t search_count, int64_t* d_mi,
                                uint8_t* d_dbits, double* d_costs, void* stream) {
    Bursts bu;
    // the last metric that is read sits at search_start + search_count - 1 + max(burst_starts) + (burst_len - 1) up and needs up samples
    if (const int rc = check_comb(rows, xlength, up, burst_len, burst_starts, num_bursts, search_start, search_count, (int64_t)up - 1, &bu))
        return rc;
    CAF_REQUIRE(std::isfinite(h), "caf_cp2fsk_bursty_demod: h must be finite");
    if (rows == 0) return CAF_OK;
    CAF_REQUIRE(d_x && d_mi && d_dbits, "caf_cp2fsk_bursty_demod: NULL buffer");
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    // the metrics of the positions [first, first + mcount): everything a cost of the search range reads
    const int64_t first = search_start + bu.lo, clen = search_count + (bu.hi - bu.lo);
    const int64_t mcount = clen + (int64_t)(burst_len - 1) * up;
    const int64_t nchunks = (search_count + AM_CHUNK - 1) / AM_CHUNK;
    float* d_m = nullptr;
    uint8_t* d_bits = nullptr;
    double *d_c = nullptr, *d_cost = d_costs, *d_pv = nullptr;
    int64_t* d_pi = nullptr;
    int rc;
    if ((rc = sc.get(&d_m, rows * mcount))) return rc;
    if ((rc = sc.get(&d_bits, rows * mcount))) return rc;
    if ((rc = sc.get(&d_c, rows * clen))) return rc;
    if (!d_cost && (rc = sc.get(&d_cost, rows * search_count))) return rc;
    if (nchunks > 1 && ((rc = sc.get(&d_pv, rows * nchunks)) || (rc = sc.get(&d_pi, rows * nchunks)))) return rc;
    if ((rc = pass_rel(burst_starts, num_bursts, &bu, sc, st))) return rc;
    if ((rc = launch_tone((const float2*)d_x, rows, xlength, up, h, first, 1, mcount, nullptr, nullptr, d_m, d_bits, st))) return rc;
    if ((rc = launch_comb_costs(d_m, mcount, 0, rows, up, burst_len, bu, num_bursts, search_count, d_c, d_cost, st))) return rc;
    if (nchunks > 1) {
        hipLaunchKernelGGL(k_argmax_f64, dim3((unsigned)nchunks, rows_grid(rows)), dim3(CT), 0, st, d_cost, nullptr, search_count, rows,
                           (int64_t)AM_CHUNK, d_pv, d_pi, nullptr, 0, 0);
        CAF_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_argmax_f64, dim3(1, rows_grid(rows)), dim3(CT), 0, st, d_pv, d_pi, nchunks, rows, nchunks, nullptr, nullptr, d_mi,
                           search_start, search_count);
    } else {
        hipLaunchKernelGGL(k_argmax_f64, dim3(1, rows_grid(rows)), dim3(CT), 0, st, d_cost, nullptr, search_count, rows, search_count, nullptr,
                           nullptr, d_mi, search_start, search_count);
    }
    CAF_HIP_TRY(hipGetLastError());
    const int64_t total = (int64_t)num_bursts * burst_len;
    hipLaunchKernelGGL(k_cp2fsk_gather, dim3((unsigned)std::min<int64_t>((total + CT - 1) / CT, 1024), rows_grid(rows)), dim3(CT), 0, st,
                       d_bits, mcount, rows, d_mi, search_start, bu.rel, num_bursts, burst_len, up, d_dbits);
    CAF_HIP_TRY(hipGetLastError());
    return sc.finish();
}
