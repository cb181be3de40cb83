// Batched Viterbi sequence detection (viterbiDemodClasses.py: ViterbiDemodulator, BurstyViterbiDemodulator).  Everything is
// float64; a row of y is complex64 or complex128, converted on load.  With A states (the alphabet), T pretransitions per state,
// L sources with their pulses (L, pulselen) and frequency offsets omegas (L), `up` samples per symbol, and w the absolute sample:
//
//   P_n[m] = sum_i exp(-j omegas[i] (n up + m)) pulses[i][m], m < pulselen       (k_viterbi_table: one table per demodulator)
//   the signal of a symbol sequence g: x[w] = sum_k g[k] P_k[w - k up]
//
// The survivor of state q carries its tail H_q[m] = the signal of its symbols before step n over the window that starts at
// n up, so at step n, for state p and its t-th pretransition q:
//   long[p, t]  = sum_{m < pulselen} |y[n up + m] - H_q[m] - alphabet[p] P_n[m]|^2,   short[p, t] = the same over m < up
//   t* = the FIRST minimum of long[p, :] alone (the accumulated metric is not added before the choice: the reference's rule),
//   pm'[p] = pm[q*] + short[p, t*],   H'_p[m] = H_q*[m + up] + alphabet[p] P_n[m + up] (zero past the pulse).
// An entry whose predecessor has pm = inf is inf; a state whose entries are all inf gets pm' = inf and keeps its path.
// Step 0 charges the short metric of the allowed states alone.  With a burst period (nb burst symbols, ng guard symbols): a
// guard step (n mod (nb + ng) >= nb) does nothing; a new-burst step (n mod (nb + ng) == 0, n > 0) connects every state q to the
// allowed states p alone and first charges g_q = sum_{m < ng up} |y[(n - ng) up + m] - H_q[m]|^2 to both metrics of q (the
// previous burst's tail over the guard), after which the tails move on by ng up samples.
//
//   k_viterbi<W>  one wave of 64 lanes per row and one row per workgroup, so the barrier of a step costs nothing and the
//                 hardware places as many rows on a compute unit as their LDS allows.  LDS: the A tails twice (a step reads one
//                 set and writes the other), the window of y and P_n: (2 A + 2) pulselen complex128.  The A T residual norms of a
//                 step are dealt to groups of W lanes (W = 64 / A T rounded down to a power of two, so that all of them are in
//                 flight at once, and no more lanes than the pulse has samples), a lane sums its samples m = lane,
//                 lane + W, ... in increasing order and caf::wave_sum<W> closes the sum; the choice is
//                 caf::wave_argmax on the negated long metric over the 8 lanes of a state (the lower t wins a tie).  One decision
//                 byte per (step, state) goes to global scratch: the predecessor, or 255 for "all inf, path kept" (and for every
//                 guard step).  Survivors are never copied: the paths are traced back at the end through LDS, VIT_DC steps of
//                 decisions at a time.
//
// The order of every sum depends on (A, T, pulselen, up, ng) alone, rows never talk to each other, and nothing is atomic: a row's
// outputs are bitwise the same whatever the batch.  Every loop bound is an argument the host has validated; nothing spins.
// Floating-point contraction is off in this file: decisions must not hinge on how a product was fused.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "caf_internal.h"
#include "caf_wave.h"

#pragma clang fp contract(off)

namespace caf {

namespace {

constexpr int VIT_A = 8;       // states at most (a state's pretransitions sit in 8 lanes)
constexpr int VIT_PL = 512;    // pulse samples at most ((2 A + 2) pulselen complex128 within the LDS of a compute unit)
constexpr int VIT_DC = 256;    // steps of decisions per traceback chunk
constexpr int VIT_WAVE = 64;
constexpr int VIT_PF = 2;      // window samples per lane fetched one step ahead (the whole window up to pulselen 128)
constexpr uint8_t VIT_KEPT = 255;

struct VitArgs {
    double ar[VIT_A], ai[VIT_A];   // the alphabet
    uint8_t pre[VIT_A * VIT_A];    // pretransitions (A, T), every entry < A
    int32_t A, T, up, pulselen, pathlen;
    int32_t nb, ng;                // burst and guard symbols; nb = 0: no period
    uint32_t allowed;              // bit a: state a may start (a burst)
    int32_t y_c128;
    int64_t ylen;                  // samples per row of y
};

__device__ __forceinline__ double2 load_y(const void* y, int y_c128, int64_t at) {
    if (y_c128) return ((const double2*)y)[at];
    const float2 v = ((const float2*)y)[at];
    return make_double2((double)v.x, (double)v.y);
}

__device__ __forceinline__ double magsq(double2 d) { return d.x * d.x + d.y * d.y; }

// P_n[m] for n < pathlen, m < pulselen: double sincos of the once-rounded product (-omegas[i]) w, the sources summed in order
__global__ __launch_bounds__(256) void k_viterbi_table(const double2* __restrict__ pulses, const double* __restrict__ omegas, int32_t L,
                                                       int32_t pulselen, int32_t up, int64_t total, double2* __restrict__ table) {
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= total) return;
    const int64_t n = at / pulselen;
    const int32_t m = (int32_t)(at - n * pulselen);
    const double w = (double)(n * up + m);
    double2 acc = make_double2(0.0, 0.0);
    for (int32_t i = 0; i < L; i++) {
        const double th = -omegas[i] * w;
        double s, c;
        sincos(th, &s, &c);
        const double2 p = pulses[(int64_t)i * pulselen + m];
        const double re = c * p.x - s * p.y, im = c * p.y + s * p.x;
        acc.x = i ? acc.x + re : re;
        acc.y = i ? acc.y + im : im;
    }
    table[at] = acc;
}

template <int W>
__global__ __launch_bounds__(VIT_WAVE) void k_viterbi(const VitArgs a, const void* __restrict__ y_all, const double2* __restrict__ table,
                                                      uint8_t* __restrict__ dec_all, uint8_t* __restrict__ states,
                                                      double* __restrict__ metrics, int32_t* __restrict__ best,
                                                      uint8_t* __restrict__ best_path) {
    extern __shared__ double2 s_dyn[];
    __shared__ double s_ar[VIT_A], s_ai[VIT_A], s_pm[VIT_A], s_g[VIT_A];
    __shared__ double s_long[VIT_A * 8], s_short[VIT_A * 8];
    __shared__ uint8_t s_pre[VIT_A * VIT_A], s_q[VIT_A * 8], s_choice[VIT_A];
    __shared__ uint8_t s_dec[VIT_DC * VIT_A];
    __shared__ int s_best;

    constexpr int NG = VIT_WAVE / W;  // residual norms in flight
    const int lane = threadIdx.x;
    const int grp = lane / W, gl = lane % W;
    const int A = a.A, T = a.T, up = a.up, PL = a.pulselen, pathlen = a.pathlen;
    const int period = a.nb + a.ng;
    const int64_t row = blockIdx.x;
    const char* y = (const char*)y_all + row * a.ylen * (a.y_c128 ? 16 : 8);
    uint8_t* dec = dec_all + row * (int64_t)pathlen * A;

    double2* H = s_dyn;                       // the tails a step reads, (A, PL)
    double2* Hn = s_dyn + (size_t)A * PL;     // the tails it writes
    double2* s_y = s_dyn + (size_t)2 * A * PL;
    double2* s_p = s_y + PL;

    if (lane < A) {
        s_ar[lane] = a.ar[lane];
        s_ai[lane] = a.ai[lane];
        s_pm[lane] = 0.0;  // (step 0 adds its short metric to this)
    }
    if (lane < A * T) s_pre[lane] = a.pre[lane];
    for (int e = lane; e < A * PL; e += VIT_WAVE) H[e] = make_double2(0.0, 0.0);
    for (int m = lane; m < PL; m += VIT_WAVE) {  // the window of step 0; every later one is fetched a step ahead
        s_y[m] = load_y(y, a.y_c128, m);
        s_p[m] = table[m];
    }
    __syncthreads();

    for (int n = 0; n < pathlen; n++) {
        // 0: the start, 1: an ordinary step, 2: the first symbol of a burst
        int kind = n == 0 ? 0 : 1;
        if (n > 0 && period > 0) {
            const int r = n % period;
            if (r >= a.nb) {  // a guard step: nothing happens, every path is kept
                if (lane < A) dec[(int64_t)n * A + lane] = VIT_KEPT;
                continue;
            }
            if (r == 0) kind = 2;
        }
        const int Te = kind == 1 ? T : (kind == 0 ? 1 : A);
        const int64_t w0 = (int64_t)n * up;

        // the next step that is no guard step: its window of y and its row of the table are asked for now and land in LDS when
        // this step is over, so their latency hides behind the step
        int64_t nn = (int64_t)n + 1;
        if (period > 0 && nn % period >= a.nb) nn = (nn / period + 1) * period;
        const bool more = nn < pathlen;
        double2 fy[VIT_PF], fp[VIT_PF];
#pragma unroll
        for (int j = 0; j < VIT_PF; j++) {
            const int m = lane + j * VIT_WAVE;
            fy[j] = fp[j] = make_double2(0.0, 0.0);
            if (more && m < PL) {
                fy[j] = load_y(y, a.y_c128, nn * up + m);
                fp[j] = table[nn * PL + m];
            }
        }

        if (kind == 2 && a.ng > 0) {
            // the previous burst's tail over the guard, then the tails move on to this step's window
            const int64_t glen = (int64_t)a.ng * up, g0 = w0 - glen;
            for (int qb = 0; qb < A; qb += NG) {
                const int q = qb + grp;
                double acc = 0.0;
                if (q < A)
                    for (int64_t m = gl; m < glen; m += W) {
                        const double2 v = load_y(y, a.y_c128, g0 + m);
                        const double2 h = m < PL ? H[q * PL + (int)m] : make_double2(0.0, 0.0);
                        acc += magsq(make_double2(v.x - h.x, v.y - h.y));
                    }
                acc = wave_sum<W>(acc);
                if (q < A && gl == 0) s_g[q] = acc;
            }
            for (int e = lane; e < A * PL; e += VIT_WAVE) {
                const int q = e / PL, m = e - q * PL;
                Hn[e] = m + glen < PL ? H[q * PL + m + (int)glen] : make_double2(0.0, 0.0);
            }
            __syncthreads();
            double2* t = H;
            H = Hn;
            Hn = t;
        }

        // the residual norms, NG of them at a time
        const int npairs = A * Te;
        for (int eb = 0; eb < npairs; eb += NG) {
            const int e = eb + grp;
            int p = 0, t = 0, q = 0;
            bool live = false;
            if (e < npairs) {
                p = e / Te;
                t = e - p * Te;
                q = kind == 1 ? s_pre[p * T + t] : (kind == 0 ? p : t);
                live = (kind == 1 || ((a.allowed >> p) & 1u)) && (kind == 0 || s_pm[q] < INFINITY);
            }
            double lg = 0.0, sh = 0.0;
            if (live) {
                const double cr = s_ar[p], ci = s_ai[p];
                const double2* h = H + q * PL;
                for (int m = gl; m < PL; m += W) {
                    const double2 pv = s_p[m], yv = s_y[m], hv = h[m];
                    const double xr = cr * pv.x - ci * pv.y, xi = cr * pv.y + ci * pv.x;
                    const double v = magsq(make_double2((yv.x - hv.x) - xr, (yv.y - hv.y) - xi));
                    lg += v;
                    if (m < up) sh += v;
                }
            }
            lg = wave_sum<W>(lg);
            sh = wave_sum<W>(sh);
            if (e < npairs && gl == 0) {
                const double g = (kind == 2 && a.ng > 0) ? s_g[q] : 0.0;
                s_long[p * 8 + t] = live ? g + lg : (double)INFINITY;
                s_short[p * 8 + t] = live ? g + sh : (double)INFINITY;
                s_q[p * 8 + t] = (uint8_t)q;
            }
        }
        __syncthreads();

        // the first minimum of a state's long metrics: lane = 8 p + t
        {
            const int p = lane >> 3, t = lane & 7;
            const bool in = p < A && t < Te;
            double v = in ? -s_long[lane] : -(double)INFINITY;
            int i = t;
            double sh = in ? s_short[lane] : 0.0;
            int q = in ? (int)s_q[lane] : 0;
            wave_argmax<4, 1>(v, i, sh, q);
            const bool none = !(v > -(double)INFINITY);
            const double pm = (in && !none) ? s_pm[q] + sh : (double)INFINITY;
            __syncthreads();  // every s_pm[q] is read before any is replaced
            if (t == 0 && p < A) {
                s_pm[p] = pm;
                s_choice[p] = none ? VIT_KEPT : (uint8_t)q;
                dec[(int64_t)n * A + p] = none ? VIT_KEPT : (uint8_t)q;
            }
        }
        __syncthreads();

        // the next tails
        for (int e = lane; e < A * PL; e += VIT_WAVE) {
            const int p = e / PL, m = e - p * PL;
            const int c = s_choice[p];
            double2 o = make_double2(0.0, 0.0);
            if (c != VIT_KEPT && m + up < PL) {
                const double2 hv = H[c * PL + m + up], pv = s_p[m + up];
                const double cr = s_ar[p], ci = s_ai[p];
                o.x = hv.x + (cr * pv.x - ci * pv.y);
                o.y = hv.y + (cr * pv.y + ci * pv.x);
            }
            Hn[e] = o;
        }
        __syncthreads();
        double2* t = H;
        H = Hn;
        Hn = t;
        if (more) {
#pragma unroll
            for (int j = 0; j < VIT_PF; j++) {
                const int m = lane + j * VIT_WAVE;
                if (m < PL) {
                    s_y[m] = fy[j];
                    s_p[m] = fp[j];
                }
            }
            for (int m = lane + VIT_PF * VIT_WAVE; m < PL; m += VIT_WAVE) {
                s_y[m] = load_y(y, a.y_c128, nn * up + m);
                s_p[m] = table[nn * PL + m];
            }
        }
        __syncthreads();
    }

    // a state that never got a metric reports inf (pathlen >= 1, so step 0 has run)
    if (lane < A && metrics) metrics[row * A + lane] = s_pm[lane];
    if (lane == 0) {
        int b = 0;
        for (int p = 1; p < A; p++)
            if (s_pm[p] < s_pm[b]) b = p;
        s_best = b;
        if (best) best[row] = b;
    }
    __syncthreads();
    if (!states && !best_path) return;

    // traceback, VIT_DC steps at a time from the end: lane p follows state p's survivor
    int cur = lane;
    const int bp = s_best;
    for (int c0 = ((pathlen - 1) / VIT_DC) * VIT_DC; c0 >= 0; c0 -= VIT_DC) {
        const int n1 = std::min(c0 + VIT_DC, pathlen);
        const int cnt = (n1 - c0) * A;
        for (int e = lane; e < cnt; e += VIT_WAVE) s_dec[e] = dec[(int64_t)c0 * A + e];
        __syncthreads();
        if (lane < A)
            for (int n = n1 - 1; n >= c0; n--) {
                const uint8_t d = s_dec[(n - c0) * A + cur];
                const uint8_t o = d == VIT_KEPT ? VIT_KEPT : (uint8_t)cur;
                if (d != VIT_KEPT) cur = d;
                if (states) states[(row * A + lane) * (int64_t)pathlen + n] = o;
                if (best_path && lane == bp) best_path[row * (int64_t)pathlen + n] = o;
            }
        __syncthreads();
    }
}

template <int W>
int launch_viterbi(const VitArgs& a, int64_t rows, size_t lds, hipStream_t st, const void* y, const double2* table, uint8_t* dec,
                   uint8_t* states, double* metrics, int32_t* best, uint8_t* best_path) {
    if (const int rc = allow_dynamic_lds((const void*)k_viterbi<W>, lds)) return rc;
    hipLaunchKernelGGL(k_viterbi<W>, dim3((unsigned)rows), dim3(VIT_WAVE), lds, st, a, y, table, dec, states, metrics, best, best_path);
    return CAF_OK;
}

}  // namespace

}  // namespace caf

using namespace caf;

int32_t caf_viterbi_geometry(int32_t* max_states, int32_t* max_pulselen, int32_t* decision_chunk) {
    if (max_states) *max_states = VIT_A;
    if (max_pulselen) *max_pulselen = VIT_PL;
    if (decision_chunk) *decision_chunk = VIT_DC;
    return CAF_OK;
}

int32_t caf_viterbi_table(const double* d_pulses, const double* d_omegas, int32_t L, int32_t pulselen, int32_t up, int32_t pathlen,
                          double* d_table, void* stream) {
    CAF_REQUIRE(L >= 1 && pulselen >= 1 && up >= 1 && pathlen >= 1, "caf_viterbi_table: L, pulselen, up and pathlen must be positive");
    CAF_REQUIRE(pulselen >= up, "caf_viterbi_table: pulselen must be at least up");
    CAF_REQUIRE((int64_t)pathlen * up + pulselen < ((int64_t)1 << 52), "caf_viterbi_table: the sample index must be exact in float64");
    const int64_t total = (int64_t)pathlen * pulselen;
    CAF_REQUIRE((total + 255) / 256 <= 0x7fffffff, "caf_viterbi_table: too many entries for one launch");
    CAF_REQUIRE(d_pulses && d_omegas && d_table, "caf_viterbi_table: NULL argument");
    hipLaunchKernelGGL(k_viterbi_table, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const double2*)d_pulses,
                       d_omegas, L, pulselen, up, total, (double2*)d_table);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_viterbi_demod(const caf_viterbi_desc* desc, void* stream) {
    CAF_REQUIRE(desc != nullptr, "caf_viterbi_demod: NULL descriptor");
    const caf_viterbi_desc& d = *desc;
    CAF_REQUIRE(d.num_states >= 1 && d.num_states <= VIT_A, "caf_viterbi_demod: 1 <= states <= 8");
    CAF_REQUIRE(d.num_trans >= 1 && d.num_trans <= d.num_states, "caf_viterbi_demod: 1 <= pretransitions per state <= states");
    CAF_REQUIRE(d.up >= 1 && d.pulselen >= d.up, "caf_viterbi_demod: up >= 1 and pulselen >= up");
    CAF_REQUIRE(d.pulselen <= VIT_PL, "caf_viterbi_demod: pulselen <= 512");
    CAF_REQUIRE(d.pathlen >= 1, "caf_viterbi_demod: pathlen >= 1");
    CAF_REQUIRE(d.num_burst_syms >= 0 && d.num_guard_syms >= 0 && (d.num_burst_syms > 0 || d.num_guard_syms == 0) &&
                    (int64_t)d.num_burst_syms + d.num_guard_syms <= 0x7fffffff,
                "caf_viterbi_demod: guard symbols need burst symbols (0, 0: no period)");
    CAF_REQUIRE(d.y_c128 == 0 || d.y_c128 == 1, "caf_viterbi_demod: y_c128 must be 0 or 1");
    CAF_REQUIRE(d.rows >= 1 && d.rows <= 0x7fffffff, "caf_viterbi_demod: 1 <= rows < 2^31");
    CAF_REQUIRE(d.ylength >= (int64_t)(d.pathlen - 1) * d.up + d.pulselen,
                "caf_viterbi_demod: a row of y needs at least (pathlen - 1) up + pulselen samples");
    CAF_REQUIRE(d.h_alphabet && d.h_pretransitions, "caf_viterbi_demod: NULL alphabet or pretransitions");
    CAF_REQUIRE(d.num_allowed >= 0 && (d.num_allowed == 0 || d.h_allowed), "caf_viterbi_demod: NULL start states");
    VitArgs a = {};
    a.A = d.num_states;
    a.T = d.num_trans;
    a.up = d.up;
    a.pulselen = d.pulselen;
    a.pathlen = d.pathlen;
    a.nb = d.num_burst_syms;
    a.ng = d.num_guard_syms;
    a.y_c128 = d.y_c128;
    a.ylen = d.ylength;
    for (int p = 0; p < a.A; p++) {
        a.ar[p] = d.h_alphabet[2 * p];
        a.ai[p] = d.h_alphabet[2 * p + 1];
    }
    for (int e = 0; e < a.A * a.T; e++) {
        CAF_REQUIRE(d.h_pretransitions[e] >= 0 && d.h_pretransitions[e] < a.A, "caf_viterbi_demod: a pretransition names no state");
        a.pre[e] = (uint8_t)d.h_pretransitions[e];
    }
    for (int e = 0; e < d.num_allowed; e++) {
        CAF_REQUIRE(d.h_allowed[e] >= 0 && d.h_allowed[e] < a.A, "caf_viterbi_demod: a start state names no state");
        a.allowed |= 1u << d.h_allowed[e];
    }
    CAF_REQUIRE(d.d_y && d.d_table, "caf_viterbi_demod: NULL y or table");
    if (!d.d_states && !d.d_metrics && !d.d_best && !d.d_best_path) return CAF_OK;

    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    uint8_t* dec = nullptr;
    if (const int rc = sc.get(&dec, d.rows * (int64_t)a.pathlen * a.A)) return rc;
    const size_t lds = (size_t)(2 * a.A + 2) * a.pulselen * sizeof(double2);
    const double2* table = (const double2*)d.d_table;
    // lanes per residual norm: as few as keep every norm of an ordinary step in flight at once (the fewer lanes, the shorter the
    // butterfly that closes a sum), and no more than the pulse has samples
    int pairs2 = 1, cover = 1;
    while (pairs2 < a.A * a.T) pairs2 <<= 1;
    while (cover < a.pulselen && cover < VIT_WAVE) cover <<= 1;
    const int W = std::min(VIT_WAVE / pairs2, cover);
#define CAF_VIT_LAUNCH(WIDTH) \
    launch_viterbi<WIDTH>(a, d.rows, lds, st, d.d_y, table, dec, d.d_states, d.d_metrics, d.d_best, d.d_best_path)
    const int rc = W == 1 ? CAF_VIT_LAUNCH(1) : W == 2 ? CAF_VIT_LAUNCH(2) : W == 4 ? CAF_VIT_LAUNCH(4) : W == 8 ? CAF_VIT_LAUNCH(8)
                 : W == 16 ? CAF_VIT_LAUNCH(16) : W == 32 ? CAF_VIT_LAUNCH(32) : CAF_VIT_LAUNCH(64);
#undef CAF_VIT_LAUNCH
    if (rc) return rc;
    CAF_HIP_TRY(hipGetLastError());
    return sc.finish();
}
