// Signal cancellation (cancellationRoutines.py: cancelSignalAtIdx, searchAndCancel, cancelSignalsAtIdx, SuccessiveCanceller).
// For a job with template s[0 .. N), start idx, frequency nu (cycles per sample) and rate alpha (cycles per sample^2):
//
//   m[n]  = s[n] exp(+j 2 pi (nu n + alpha n^2 / 2))                     the model
//   D     = sum_n conj(m[n]) rx[idx + n],  Es = sum |s[n]|^2,  Er = sum |rx[idx + n]|^2
//   amp   = D / Es,  QF^2 = |D|^2 / (Es Er),  resid = Er - |D|^2 / Es
//   cancelled[idx + n] = rx[idx + n] - amp m[n]                          elsewhere cancelled = rx
//
//   k_cancel_search    D for J rates (any list) x K frequencies nu0 + k dnu of B jobs.  A work item (one workgroup of 256 threads)
//                      is (job, chunk of CS_CHUNK template samples); thread t owns the samples chunk CS_CHUNK + t + 256 i,
//                      i < CS_SPT.  It loads p[i] = conj(s[n]) rx[idx + n] and the step rotor w[i] = exp(-j 2 pi dnu n) (rounded once
//                      from float64) once and loops over the rates inside the item.  Per rate the start phase
//                      nu0 n + alpha_j n^2 / 2 is formed in float64, reduced exactly to a fraction of a turn (n^2 < 2^40 is exact,
//                      the products go through mul_split).  The rotor z[i] is seeded from that phase plus the exactly reduced
//                      dnu (k n) at every k that is a multiple of CS_RESEED, and stepped z *= w in float32 in between: 8 float32
//                      lane operations per term (4 for p z into the sum, 4 for the step).  Where jobs x chunks would leave most
//                      CUs idle, the (rate, block of CS_RESEED frequencies) units of a (job, chunk) are dealt to several items
//                      (grid z): a unit starts with a seed, so no bit depends on the dealing.
//                      A thread's CS_SPT terms of one k are summed in float32; the 256 threads' sums of a tile of CS_KT
//                      frequencies go through LDS and are added in float64 in one fixed order (16 threads per frequency: 16
//                      values in turn each, then the xor butterfly of caf_wave.h).  The item writes its partial of D[j][k] and of
//                      Es, Er.  Nothing is atomic, and nothing depends on B: a job is bitwise the same in any batch.
//   k_cancel_fold      per (job, tile of 256 hypotheses): the chunks' partials added in increasing chunk order in float64, |D|^2,
//                      the optional float32 QF^2 surface, the tile's arg max (lower flat index j K + k wins ties).
//   k_cancel_pick      per job: the arg max over the tiles (same tie rule), amp, QF^2, resid and the winning nu and alpha.
//   k_cancel_subtract  one thread per rx sample; out[m] = rx[m] - sum_b amp_b m_b[m - idx_b] over the covering jobs in increasing
//                      b, one float32 complex multiply-add each.  A workgroup first lists the jobs that meet its 256 samples (in
//                      order, by ballot).  The phase of every sample comes from float64, reduced exactly.  A thread reads and
//                      writes only its own sample, so out may alias rx.
//
// Floating-point contraction is off in this file (mul_split needs that); the fused multiply-adds are written out.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "caf_internal.h"
#include "caf_phase.h"  // mul_split, frac_turn, unit_f32, cmulf
#include "caf_wave.h"   // wave_sum, wave_argmax, block_sum, block_argmax

#pragma clang fp contract(off)

namespace caf {

namespace {

constexpr int CS_THREADS = 256;
constexpr int CS_SPT = 8;                        // samples per thread
constexpr int CS_CHUNK = CS_THREADS * CS_SPT;    // template samples per work item
constexpr int CS_RESEED = 64;                    // rotor steps between float64 seeds (the bound of tests/cancel_ref.py grows with it)
constexpr int CS_KT = 16;                        // frequencies per LDS tile; CS_RESEED is a multiple of it
constexpr int CS_MAXN = 1 << 20;
constexpr int CS_MAXJ = 64;
constexpr int CS_MAXK = 1024;
constexpr int CS_MAXB = 256;                     // also the subtract's threads per workgroup: thread b tests job b
constexpr int CS_TARGET_ITEMS = 2048;                // work items wanted in a launch (8 per CU)
constexpr int64_t CS_SCRATCH_DOUBLES = (int64_t)1 << 27;  // partials of one pass (1 GiB); more jobs are run in passes
static_assert(CS_RESEED % CS_KT == 0 && CS_THREADS % CS_KT == 0 && CS_THREADS / CS_KT == 16, "the tile fold assumes 16 threads per frequency");
static_assert(CS_MAXB <= CS_THREADS, "one thread per job in the subtract's list");

// fraction of a turn of a b (|result| <= 1/2 + an ulp)
__device__ __forceinline__ double turn_of(double a, double b) {
    double whole, rest;
    mul_split(a, b, &whole, &rest);
    return rest;
}

// job_nu / job_rate != NULL: job b has its own nu0 = job_nu[b] and its one rate job_rate[b] (J == 1)
__global__ __launch_bounds__(CS_THREADS) void k_cancel_search(const float2* __restrict__ sigs, int32_t N, const float2* __restrict__ rx,
                                                            int64_t rx_len, const int32_t* __restrict__ idx, double nu0, double dnu, int32_t K,
                                                            const double* __restrict__ rates, int32_t J, const double* __restrict__ job_nu,
                                                            const double* __restrict__ job_rate, int32_t chunks, int32_t units_per_item,
                                                            double2* __restrict__ part, double2* __restrict__ energy) {
    __shared__ float2 s_acc[CS_KT][CS_THREADS];
    __shared__ WaveSlots<CS_THREADS / 64, double, double> s_e;
    const int tid = threadIdx.x;
    const int32_t chunk = (int32_t)blockIdx.x, b = (int32_t)blockIdx.y;
    const int64_t start = idx[b];
    const float2* __restrict__ s = sigs + (int64_t)b * N;
    if (job_nu) {
        nu0 = job_nu[b];
        rates = job_rate + b;
    }

    float2 p[CS_SPT], w[CS_SPT], z[CS_SPT];
    double es = 0.0, er = 0.0;
#pragma unroll
    for (int i = 0; i < CS_SPT; i++) {
        const int32_t n = chunk * CS_CHUNK + tid + CS_THREADS * i;
        const int64_t at = start + n;
        float2 a = make_float2(0.f, 0.f), x = make_float2(0.f, 0.f);
        if (n < N && at >= 0 && at < rx_len) {  // (the entry point has checked the window; nothing is read outside either array)
            a = s[n];
            x = rx[at];
        }
        p[i] = make_float2(fmaf(a.x, x.x, a.y * x.y), fmaf(a.x, x.y, -(a.y * x.x)));  // conj(a) x
        es += (double)a.x * (double)a.x + (double)a.y * (double)a.y;
        er += (double)x.x * (double)x.x + (double)x.y * (double)x.y;
        double ws, wc;
        sincospi(-2.0 * frac_turn(turn_of(dnu, (double)n)), &ws, &wc);
        w[i] = make_float2((float)wc, (float)ws);
    }
    block_sum(s_e, es, er);
    if (tid == 0 && blockIdx.z == 0) energy[(int64_t)b * chunks + chunk] = make_double2(es, er);

    // A unit is (rate j, block of CS_RESEED frequencies): it starts with a seed, so its values do not depend on which item runs it.
    const int kt = tid >> 4, sub = tid & 15;  // the tile fold: frequency kt of the tile, 16 values in turn from sub
    double2* __restrict__ mine = part + ((int64_t)b * chunks + chunk) * J * K;
    const int32_t kblocks = (K + CS_RESEED - 1) / CS_RESEED;
    const int32_t u0 = (int32_t)blockIdx.z * units_per_item, u1 = min(u0 + units_per_item, J * kblocks);
    for (int32_t u = u0; u < u1; u++) {
        const int32_t j = u / kblocks, kb = (u - j * kblocks) * CS_RESEED;
        const double half_rate = 0.5 * rates[j];
#pragma unroll
        for (int i = 0; i < CS_SPT; i++) {
            const double n = (double)(chunk * CS_CHUNK + tid + CS_THREADS * i);
            const double base = frac_turn(turn_of(nu0, n) + turn_of(half_rate, n * n));
            z[i] = unit_f32(frac_turn(-(base + turn_of(dnu, (double)kb * n))));
        }
        const int32_t kend = min(K, kb + CS_RESEED);
        for (int32_t k0 = kb; k0 < kend; k0 += CS_KT) {
#pragma unroll 4
            for (int t = 0; t < CS_KT; t++) {  // (past K the tile goes on with values nobody reads)
                float ar = 0.f, ai = 0.f;
#pragma unroll
                for (int i = 0; i < CS_SPT; i++) {
                    ar = fmaf(p[i].x, z[i].x, ar);
                    ar = fmaf(-p[i].y, z[i].y, ar);
                    ai = fmaf(p[i].x, z[i].y, ai);
                    ai = fmaf(p[i].y, z[i].x, ai);
                    z[i] = cmulf(z[i], w[i]);
                }
                s_acc[t][tid] = make_float2(ar, ai);
            }
            __syncthreads();
            double sr = 0.0, si = 0.0;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const float2 v = s_acc[kt][i * 16 + sub];
                sr += (double)v.x;
                si += (double)v.y;
            }
            sr = wave_sum<16>(sr);
            si = wave_sum<16>(si);
            if (sub == 0 && k0 + kt < K) mine[(int64_t)j * K + k0 + kt] = make_double2(sr, si);
            __syncthreads();
        }
    }
}

struct CancelBest {
    double v, dr, di;
    int32_t f, pad;
};

__global__ __launch_bounds__(CS_THREADS) void k_cancel_fold(const double2* __restrict__ part, const double2* __restrict__ energy, int32_t chunks,
                                                          int32_t JK, int32_t tiles, float* __restrict__ surface, int32_t job0,
                                                          CancelBest* __restrict__ best) {
    __shared__ WaveSlots<CS_THREADS / 64, double, int32_t, double, double> s_best;
    const int tid = threadIdx.x;
    const int32_t tile = (int32_t)blockIdx.x, b = (int32_t)blockIdx.y;
    const int32_t f = tile * CS_THREADS + tid;
    double es = 0.0, er = 0.0;
    for (int32_t c = 0; c < chunks; c++) {  // (the same address in every lane)
        const double2 e = energy[(int64_t)b * chunks + c];
        es += e.x;
        er += e.y;
    }
    double dr = 0.0, di = 0.0;
    if (f < JK) {
        const double2* __restrict__ q = part + (int64_t)b * chunks * JK + f;
        for (int32_t c = 0; c < chunks; c++) {
            const double2 d = q[(int64_t)c * JK];
            dr += d.x;
            di += d.y;
        }
    }
    double v = f < JK ? dr * dr + di * di : -1.0;
    if (v != v) v = -1.0;  // (a NaN never wins)
    if (surface && f < JK) surface[(int64_t)(job0 + b) * JK + f] = (float)(v < 0.0 ? NAN : v / (es * er));
    int32_t fi = f;
    block_argmax(s_best, v, fi, dr, di);
    if (tid == 0) best[(int64_t)b * tiles + tile] = CancelBest{v, dr, di, fi, 0};
}

__global__ __launch_bounds__(64) void k_cancel_pick(const CancelBest* __restrict__ best, const double2* __restrict__ energy, int32_t chunks,
                                                  int32_t tiles, int32_t K, double nu0, double dnu, const double* __restrict__ rates,
                                                  const double* __restrict__ job_nu, const double* __restrict__ job_rate, int32_t job0,
                                                  int32_t* __restrict__ o_j, int32_t* __restrict__ o_k, double* __restrict__ o_nu,
                                                  double* __restrict__ o_rate, double* __restrict__ o_amp, double* __restrict__ o_qf2,
                                                  double* __restrict__ o_es, double* __restrict__ o_er, double* __restrict__ o_resid) {
    const int lane = threadIdx.x;
    const int32_t b = (int32_t)blockIdx.x;
    double v = -2.0, dr = 0.0, di = 0.0;
    int32_t f = 0x7fffffff;
    for (int32_t t = lane; t < tiles; t += 64) {  // (increasing flat index within a lane: a strict > keeps the first maximum)
        const CancelBest o = best[(int64_t)b * tiles + t];
        if (o.v > v) {
            v = o.v;
            dr = o.dr;
            di = o.di;
            f = o.f;
        }
    }
    wave_argmax(v, f, dr, di);
    if (lane != 0) return;
    double es = 0.0, er = 0.0;
    for (int32_t c = 0; c < chunks; c++) {
        const double2 e = energy[(int64_t)b * chunks + c];
        es += e.x;
        er += e.y;
    }
    const int32_t j = f / K, k = f - j * K;
    const int32_t g = job0 + b;
    if (v < 0.0) v = NAN;  // (every |D|^2 of the job was NaN: hypothesis 0, and NaN in what follows from D)
    if (job_nu) {
        nu0 = job_nu[g];
        rates = job_rate + g;
    }
    if (o_j) o_j[g] = j;
    if (o_k) o_k[g] = k;
    if (o_nu) o_nu[g] = nu0 + (double)k * dnu;
    if (o_rate) o_rate[g] = rates[j];
    if (o_amp) {
        o_amp[2 * g] = dr / es;
        o_amp[2 * g + 1] = di / es;
    }
    if (o_qf2) o_qf2[g] = v / (es * er);
    if (o_es) o_es[g] = es;
    if (o_er) o_er[g] = er;
    if (o_resid) o_resid[g] = er - v / es;
}

__global__ __launch_bounds__(CS_THREADS) void k_cancel_subtract(const float2* __restrict__ sigs, int32_t B, int32_t N, const float2* rx,
                                                              int64_t rx_len, const int32_t* __restrict__ idx, const double* __restrict__ nu,
                                                              const double* __restrict__ rate, const double* __restrict__ amp, float2* out) {
    __shared__ int32_t s_list[CS_MAXB];
    __shared__ int32_t s_count[CS_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * CS_THREADS;
    const int64_t m = m0 + tid;
    // the jobs whose windows meet this workgroup's samples, in increasing b
    bool meets = false;
    if (tid < B) {
        const int64_t a = idx[tid];
        meets = a < m0 + CS_THREADS && a + N > m0;
    }
    const unsigned long long mask = __ballot(meets);
    // (the carry AND the total from one store and barrier: block_exclusive and block_sum_totals of caf_wave.h would take two)
    if (lane == 0) s_count[wave] = __popcll(mask);
    __syncthreads();
    int32_t before = 0, count = 0;
#pragma unroll
    for (int w = 0; w < CS_THREADS / 64; w++) {
        if (w < wave) before += s_count[w];
        count += s_count[w];
    }
    if (meets) s_list[before + __popcll(mask & ((1ull << lane) - 1ull))] = tid;
    __syncthreads();
    if (m >= rx_len) return;
    float2 x = rx[m];
    for (int32_t i = 0; i < count; i++) {
        const int32_t b = s_list[i];
        const int64_t n64 = m - (int64_t)idx[b];
        if (n64 < 0 || n64 >= N) continue;
        const double n = (double)n64;
        const float2 zz = unit_f32(frac_turn(turn_of(nu[b], n) + turn_of(0.5 * rate[b], n * n)));
        const float2 md = cmulf(sigs[(int64_t)b * N + n64], zz);
        const float ar = (float)amp[2 * b], ai = (float)amp[2 * b + 1];
        x.x = fmaf(-ar, md.x, x.x);
        x.x = fmaf(ai, md.y, x.x);
        x.y = fmaf(-ar, md.y, x.y);
        x.y = fmaf(-ai, md.x, x.y);
    }
    out[m] = x;
}

// the windows of B jobs lie wholly inside rx (the indices are downloaded: B <= 256 words, complete on return)
int check_windows(const int32_t* d_idx, int32_t B, int32_t N, int64_t rx_len, hipStream_t st, const char* what) {
    std::vector<int32_t> h((size_t)B);
    if (const int rc = host_d2h(h.data(), d_idx, (int64_t)B * 4, st)) return rc;
    for (int32_t b = 0; b < B; b++) {
        if (h[b] < 0 || (int64_t)h[b] + N > rx_len) {
            set_error(std::string(what) + ": the window of job " + std::to_string(b) + " (idx " + std::to_string(h[b]) + ", " +
                      std::to_string(N) + " samples) is not inside rx (" + std::to_string(rx_len) + " samples)");
            return CAF_ERR_INVALID;
        }
    }
    return CAF_OK;
}

struct SearchOut {
    int32_t *j, *k;
    double *nu, *rate, *amp, *qf2, *es, *er, *resid;
    float* surface;
};

int run_search(const float2* sigs, int32_t B, int32_t N, const float2* rx, int64_t rx_len, const int32_t* d_idx, double nu0, double dnu,
               int32_t K, const double* d_rates, int32_t J, const double* job_nu, const double* job_rate, const SearchOut& o, hipStream_t st) {
    const int32_t chunks = (N + CS_CHUNK - 1) / CS_CHUNK;
    const int32_t JK = J * K;
    const int32_t tiles = (JK + CS_THREADS - 1) / CS_THREADS;
    const int64_t per_job = 2 * (int64_t)chunks * JK;  // doubles
    const int32_t pass = (int32_t)std::max<int64_t>(1, std::min<int64_t>(B, CS_SCRATCH_DOUBLES / per_job));
    Scratch sc(st);
    double2 *part = nullptr, *energy = nullptr;
    CancelBest* best = nullptr;
    if (const int rc = sc.get(&part, (int64_t)pass * chunks * JK)) return rc;
    if (const int rc = sc.get(&energy, (int64_t)pass * chunks)) return rc;
    if (const int rc = sc.get(&best, (int64_t)pass * tiles)) return rc;
    for (int32_t b0 = 0; b0 < B; b0 += pass) {  // (a job's results do not depend on the pass it runs in)
        const int32_t nb = std::min(pass, B - b0);
        // few (job, chunk) pairs: the units (rate, block of CS_RESEED frequencies) are dealt to several items, which changes no bit
        const int32_t units = J * ((K + CS_RESEED - 1) / CS_RESEED);
        const int64_t want = (CS_TARGET_ITEMS + (int64_t)chunks * nb - 1) / ((int64_t)chunks * nb);
        const int32_t per_item = (int32_t)((units + std::min<int64_t>(want, units) - 1) / std::min<int64_t>(want, units));
        const int32_t groups = (units + per_item - 1) / per_item;
        hipLaunchKernelGGL(k_cancel_search, dim3((unsigned)chunks, (unsigned)nb, (unsigned)groups), dim3(CS_THREADS), 0, st,
                           sigs + (int64_t)b0 * N, N, rx, rx_len, d_idx + b0, nu0, dnu, K, d_rates, J, job_nu ? job_nu + b0 : nullptr,
                           job_rate ? job_rate + b0 : nullptr, chunks, per_item, part, energy);
        hipLaunchKernelGGL(k_cancel_fold, dim3((unsigned)tiles, (unsigned)nb), dim3(CS_THREADS), 0, st, (const double2*)part,
                           (const double2*)energy, chunks, JK, tiles, o.surface, b0, best);
        hipLaunchKernelGGL(k_cancel_pick, dim3((unsigned)nb), dim3(64), 0, st, (const CancelBest*)best, (const double2*)energy, chunks, tiles, K,
                           nu0, dnu, d_rates, job_nu, job_rate, b0, o.j, o.k, o.nu, o.rate, o.amp, o.qf2, o.es, o.er, o.resid);
    }
    CAF_HIP_TRY(hipGetLastError());
    return sc.finish();
}

}  // namespace

}  // namespace caf

using namespace caf;

int32_t caf_cancel_geometry(int32_t* max_len, int32_t* chunk, int32_t* samples_per_thread, int32_t* reseed_interval, int32_t* max_jobs,
                            int32_t* max_rates, int32_t* max_freqs) {
    if (max_len) *max_len = CS_MAXN;
    if (chunk) *chunk = CS_CHUNK;
    if (samples_per_thread) *samples_per_thread = CS_SPT;
    if (reseed_interval) *reseed_interval = CS_RESEED;
    if (max_jobs) *max_jobs = CS_MAXB;
    if (max_rates) *max_rates = CS_MAXJ;
    if (max_freqs) *max_freqs = CS_MAXK;
    return CAF_OK;
}

int32_t caf_cancel_search(const float* d_sigs, int32_t B, int32_t N, const float* d_rx, int64_t rx_len, const int32_t* d_idx, double nu0,
                          double dnu, int32_t K, const double* d_rates, int32_t J, int32_t* d_best_j, int32_t* d_best_k, double* d_nu,
                          double* d_rate, double* d_amp, double* d_qf2, double* d_es, double* d_er, double* d_resid, float* d_surface,
                          void* stream) {
    CAF_REQUIRE(N >= 1 && N <= CS_MAXN, "caf_cancel_search: 1 <= N <= 2^20");
    CAF_REQUIRE(B >= 1 && B <= CS_MAXB, "caf_cancel_search: 1 <= B <= 256");
    CAF_REQUIRE(J >= 1 && J <= CS_MAXJ, "caf_cancel_search: 1 <= J <= 64");
    CAF_REQUIRE(K >= 1 && K <= CS_MAXK, "caf_cancel_search: 1 <= K <= 1024");
    CAF_REQUIRE(rx_len >= N, "caf_cancel_search: rx is shorter than the template");
    CAF_REQUIRE(std::isfinite(nu0) && std::isfinite(dnu), "caf_cancel_search: nu0 and dnu must be finite");
    CAF_REQUIRE(d_sigs && d_rx && d_idx && d_rates, "caf_cancel_search: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = check_windows(d_idx, B, N, rx_len, st, "caf_cancel_search")) return rc;
    const SearchOut o{d_best_j, d_best_k, d_nu, d_rate, d_amp, d_qf2, d_es, d_er, d_resid, d_surface};
    return run_search((const float2*)d_sigs, B, N, (const float2*)d_rx, rx_len, d_idx, nu0, dnu, K, d_rates, J, nullptr, nullptr, o, st);
}

int32_t caf_cancel_estimate(const float* d_sigs, int32_t B, int32_t N, const float* d_rx, int64_t rx_len, const int32_t* d_idx,
                            const double* d_nu, const double* d_rate, double* d_amp, double* d_qf2, double* d_es, double* d_er,
                            double* d_resid, void* stream) {
    CAF_REQUIRE(N >= 1 && N <= CS_MAXN, "caf_cancel_estimate: 1 <= N <= 2^20");
    CAF_REQUIRE(B >= 1 && B <= CS_MAXB, "caf_cancel_estimate: 1 <= B <= 256");
    CAF_REQUIRE(rx_len >= N, "caf_cancel_estimate: rx is shorter than the template");
    CAF_REQUIRE(d_sigs && d_rx && d_idx && d_nu && d_rate, "caf_cancel_estimate: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = check_windows(d_idx, B, N, rx_len, st, "caf_cancel_estimate")) return rc;
    const SearchOut o{nullptr, nullptr, nullptr, nullptr, d_amp, d_qf2, d_es, d_er, d_resid, nullptr};
    return run_search((const float2*)d_sigs, B, N, (const float2*)d_rx, rx_len, d_idx, 0.0, 0.0, 1, d_rate, 1, d_nu, d_rate, o, st);
}

int32_t caf_cancel_subtract(const float* d_sigs, int32_t B, int32_t N, const float* d_rx, int64_t rx_len, const int32_t* d_idx,
                            const double* d_nu, const double* d_rate, const double* d_amp, float* d_out, void* stream) {
    CAF_REQUIRE(N >= 1 && N <= CS_MAXN, "caf_cancel_subtract: 1 <= N <= 2^20");
    CAF_REQUIRE(B >= 1 && B <= CS_MAXB, "caf_cancel_subtract: 1 <= B <= 256");
    CAF_REQUIRE(rx_len >= N && (rx_len + CS_THREADS - 1) / CS_THREADS <= 0x7fffffff, "caf_cancel_subtract: N <= rx_len < 2^39");
    CAF_REQUIRE(d_sigs && d_rx && d_idx && d_nu && d_rate && d_amp && d_out, "caf_cancel_subtract: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = check_windows(d_idx, B, N, rx_len, st, "caf_cancel_subtract")) return rc;
    hipLaunchKernelGGL(k_cancel_subtract, dim3(cdiv(rx_len, CS_THREADS)), dim3(CS_THREADS), 0, st, (const float2*)d_sigs, B, N, (const float2*)d_rx,
                       rx_len, d_idx, d_nu, d_rate, d_amp, (float2*)d_out);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}
