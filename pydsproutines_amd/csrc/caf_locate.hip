// TDOA / FDOA grid-search geolocation (localizationRoutines.py:510-748: gridSearchTDOA, gridSearchFDOA, gridSearchTDOA_direct,
// gridSearchTDFD_direct and the gridsearchtdoa_kernel of gridSearchTDOA_gpu).  Everything is float64.  For a grid point p and the
// measurement record k = (s1, s2, v1, v2, r, wr, d, wd):
//   rho1 = |p - s1|, rho2 = |p - s2|,   e = r - (rho2 - rho1),   f = d - ((p - s2).v2 / rho2 - (p - s1).v1 / rho1)
//   cost[p] = sum_k (wr e^2 + wd f^2)       in the order of k, the TD term before the FD term of the same k.
//
//   k_locate<TD, FD, SRC>  one workgroup per LOC_P = 1024 consecutive points (four per thread, 256 apart, all in registers, so the
//                          reciprocal-square-root chains of different points overlap) and per measurement set (blockIdx.y).  The
//                          records are staged in LDS LOC_C = 64 at a time -- read from global memory once per workgroup -- and read
//                          back as broadcasts, one record for the thread's four points.  A TD instantiation never reads a velocity.
//                          SRC: an (N, 3) matrix, or a separable mesh that is never materialised,
//                          p(i, j) = (A[i] C[j], A[i] S[j], Z[i]) or (XY) p(i, j) = (X[j], Y[i], z), flat index i nj + j.
//   k_grid_fold<false>     (caf_grid.h) the workgroups' (minimum, index) partials of each set -> one (value, index) per set.
// The point source, the sets, the stores and the arg min are the frame of caf_grid.h, shared with caf_crbmap.hip;
// this file holds the two record loops and their choice of kernel.
//
// One range costs: a = p - s (3 subtractions), d2 = a.a (one product and two fma), y = 1 / sqrt(d2) from v_rsq_f64 and ONE
// third-order correction y0 + y0 e (1/2 + 3/8 e), e = 1 - d2 y0^2 (the hardware estimate is good to about 2^-23, so the e^3 that is
// left is below 2^-65), and rho = d2 y.  The same y scales the dot product (p - s).v, so no division and no second root is taken.
// In units of eps = 2^-53 relative to rho: 1 (the subtractions: every component of a is off by at most eps, and so is its norm)
// + 1.5 (three roundings in d2, halved by the root) + 1.5 (the correction: e is known to eps absolute and enters with weight 1/2,
// and the closing fma rounds once) + 1 (the product d2 y) = 5; the difference rho2 - rho1 rounds once more, at most eps max(rho1,
// rho2).  tests/locate_ref.py therefore bounds the error of rho2 - rho1 by c1 eps (rho1 + rho2) with c1 = 6.  A projected velocity
// a.v y: 1 (a) + 3 (one product and two fma) relative to sum_i |a_i v_i|, 4 for y as above, 1 for the product with y, and the
// difference of the two rounds once: c2 = 10 relative to sum_i |a_i v1_i| / rho1 + sum_i |a_i v2_i| / rho2.
//
// A point ON a sensor has d2 = 0: its range is 0 (selected, not computed) and its unit vector is 0 / 0 = NaN as in the reference, so
// its TD cost is finite and its FD cost NaN.  A NaN cost is stored as NaN and never wins the arg min.
//
// Arg min, in a fixed order and without atomics: a thread visits its points in increasing index and keeps the first minimum (strict
// <); across lanes and the workgroup's four waves caf::block_argmin (the arg max of the negated cost: lower index wins a tie);
// the partials of a set, in increasing order of workgroup, by k_grid_fold in the same way.
// Floating-point contraction is off in this file: every product and sum is rounded where it is written, and each fma is spelled.
//
// One-bounce round trips (localizationRoutines.py:368-507 of the reference: gridSearchRTT, gridSearchBlindLinearRTT).  The record
// is (s1 = transmitter, s2 = receiver, g0, g1 in slots 6 and 7, r = the measured range sum in slot 12, w in slot 13); with
//   d_k = r_k - (rho1_k + rho2_k)
//   k_locate_rtt<Q, SRC>   Q = 0: cost[p] = sum_k w_k d_k^2, in the order of k.
//                          Q = 1, 2: the columns g_i are orthonormal under the weights of their set (sum_k w g_i g_j = delta_ij,
//                          the host's work), and the cost is what is left of d once its part in their span is taken out,
//                            pass 1  alpha = sum_k (w g0) d,  beta = sum_k (w g1) d       (beta for Q = 2 alone)
//                            pass 2  cost[p] = sum_k w (d - alpha g0 - beta g1)^2         = min over (a, b) of sum_k w (d - a t - b)^2
//                          each in the order of k.  The geometry, the staging and the arg min are k_locate's.
// Two passes are required: the one-pass form sum w d^2 - alpha^2 - beta^2 subtracts numbers that agree to six or more digits at the
// minimum (a turnaround of 128 us is 38 km of d against metres of residual) and was measured 1.0e-7 off in relative terms where
// the two passes are 2.4e-13 off, both in plain float64.  The price is each range twice.  As written, d costs 28 float64
// operations per point and record (per range 3 subtractions, 1 product and 2 fma for a.a, 6 for the reciprocal root, 1 product
// for rho = 13, twice; the sum and the difference from r), so Q = 0 costs 28 + 2 = 30, Q = 1 (28 + 1) + (28 + 3) = 60 and
// Q = 2 (28 + 2) + (28 + 4) = 62.  A set of at most LOC_C records is staged once and pass 2 reads it from LDS again; a longer
// set is read from global memory once per pass.  The range sum's error is c1 eps (rho1 + rho2) with the same c1 = 6: 5 per range
// and one rounding of the sum.  A point on a sensor has that range 0 (selected), so its cost is finite.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "caf_internal.h"
#include "caf_grid.h"
#include "caf_wave.h"

#pragma clang fp contract(off)

namespace caf {

namespace {

constexpr int LOC_T = 256;              // threads per workgroup
constexpr int LOC_PPT = 4;              // points per thread
constexpr int LOC_P = LOC_T * LOC_PPT;  // points per workgroup
constexpr int LOC_C = 64;               // records per LDS chunk (8 KiB)
constexpr int LOC_REC = 16;             // doubles per record: s1(3) s2(3) v1(3) v2(3) r wr d wd

// what every search kernel ends with: the thread's costs stored, and the workgroup's first minimum into the partials
__device__ __forceinline__ void put_costs(WaveSlots<LOC_T / 64, double, long long>& s_best, const double (&acc)[LOC_PPT], int64_t N,
                                          int64_t base, int tid, int set, void* __restrict__ cost, int cost_f32,
                                          double* __restrict__ part_v, int64_t* __restrict__ part_i) {
    const int64_t out0 = (int64_t)set * N;
    if (cost) {
#pragma unroll
        for (int j = 0; j < LOC_PPT; j++) {
            const int64_t at = base + tid + j * LOC_T;
            if (at < N) store_value(cost, cost_f32, out0 + at, acc[j]);
        }
    }
    if (part_v) {
        double bv;
        long long bi;
        thread_first_min<LOC_T, LOC_PPT>(acc, N, base, tid, bv, bi);
        block_argmin(s_best, bv, bi);
        if (tid == 0) {
            const int64_t o = (int64_t)set * gridDim.x + blockIdx.x;
            part_v[o] = bv;
            part_i[o] = (int64_t)bi;
        }
    }
}

template <bool TD, bool FD, int SRC>
__global__ __launch_bounds__(LOC_T) void k_locate(const LocSrc src, int64_t N, const double* __restrict__ rec, int64_t K,
                                                  const int64_t* __restrict__ set_starts, void* __restrict__ cost, int cost_f32,
                                                  double* __restrict__ part_v, int64_t* __restrict__ part_i) {
    __shared__ double s_rec[LOC_C * LOC_REC];
    __shared__ WaveSlots<LOC_T / 64, double, long long> s_best;
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * LOC_P;
    const int set = blockIdx.y;

    int64_t k0, k1;
    set_records(set_starts, set, K, k0, k1);

    double px[LOC_PPT], py[LOC_PPT], pz[LOC_PPT], acc[LOC_PPT];
    loc_points<SRC, LOC_T, LOC_PPT>(src, N, base, tid, px, py, pz);
#pragma unroll
    for (int j = 0; j < LOC_PPT; j++) acc[j] = 0.0;

    for (int64_t kc = k0; kc < k1; kc += LOC_C) {
        const int nrec = (int)std::min<int64_t>(LOC_C, k1 - kc);
        const double* g = rec + kc * LOC_REC;
        for (int q = tid; q < nrec * LOC_REC; q += LOC_T) s_rec[q] = g[q];
        __syncthreads();
        for (int k = 0; k < nrec; k++) {
            const double* r = s_rec + k * LOC_REC;  // the same address in every lane: broadcast reads
            const double s1x = r[0], s1y = r[1], s1z = r[2], s2x = r[3], s2y = r[4], s2z = r[5];
            double v1x = 0, v1y = 0, v1z = 0, v2x = 0, v2y = 0, v2z = 0, rr = 0, wr = 0, dd = 0, wd = 0;
            if constexpr (FD) {
                v1x = r[6], v1y = r[7], v1z = r[8], v2x = r[9], v2y = r[10], v2z = r[11];
                dd = r[14], wd = r[15];
            }
            if constexpr (TD) rr = r[12], wr = r[13];
#pragma unroll
            for (int j = 0; j < LOC_PPT; j++) {
                const double a1x = px[j] - s1x, a1y = py[j] - s1y, a1z = pz[j] - s1z;
                const double a2x = px[j] - s2x, a2y = py[j] - s2y, a2z = pz[j] - s2z;
                const double q1 = fma(a1z, a1z, fma(a1y, a1y, a1x * a1x));
                const double q2 = fma(a2z, a2z, fma(a2y, a2y, a2x * a2x));
                const double y1 = rsqrt_once(q1), y2 = rsqrt_once(q2);
                if constexpr (TD) {
                    const double rho1 = q1 == 0.0 ? 0.0 : q1 * y1;
                    const double rho2 = q2 == 0.0 ? 0.0 : q2 * y2;
                    const double e = rr - (rho2 - rho1);
                    acc[j] = fma(wr, e * e, acc[j]);
                }
                if constexpr (FD) {
                    const double u1 = fma(a1z, v1z, fma(a1y, v1y, a1x * v1x)) * y1;
                    const double u2 = fma(a2z, v2z, fma(a2y, v2y, a2x * v2x)) * y2;
                    const double f = dd - (u2 - u1);
                    acc[j] = fma(wd, f * f, acc[j]);
                }
            }
        }
        __syncthreads();  // the chunk is overwritten next
    }
    put_costs(s_best, acc, N, base, tid, set, cost, cost_f32, part_v, part_i);
}

// ---- one-bounce round trips ------------------------------------------------------------------------------------------------------
// the staged records against the thread's points: PASS 0 adds to alpha (and beta), PASS 1 adds the squared residual to acc
template <int Q, int PASS>
__device__ __forceinline__ void rtt_chunk(const double* s_rec, int nrec, const double (&px)[LOC_PPT], const double (&py)[LOC_PPT],
                                          const double (&pz)[LOC_PPT], double (&al)[LOC_PPT], double (&be)[LOC_PPT], double (&acc)[LOC_PPT]) {
    for (int k = 0; k < nrec; k++) {
        const double* r = s_rec + k * LOC_REC;  // the same address in every lane: broadcast reads
        const double s1x = r[0], s1y = r[1], s1z = r[2], s2x = r[3], s2y = r[4], s2z = r[5], rr = r[12], w = r[13];
        double g0 = 0, g1 = 0;
        if constexpr (Q >= 1) g0 = r[6];
        if constexpr (Q == 2) g1 = r[7];
        const double wg0 = w * g0, wg1 = w * g1;
#pragma unroll
        for (int j = 0; j < LOC_PPT; j++) {
            const double a1x = px[j] - s1x, a1y = py[j] - s1y, a1z = pz[j] - s1z;
            const double a2x = px[j] - s2x, a2y = py[j] - s2y, a2z = pz[j] - s2z;
            const double q1 = fma(a1z, a1z, fma(a1y, a1y, a1x * a1x));
            const double q2 = fma(a2z, a2z, fma(a2y, a2y, a2x * a2x));
            const double rho1 = q1 == 0.0 ? 0.0 : q1 * rsqrt_once(q1);
            const double rho2 = q2 == 0.0 ? 0.0 : q2 * rsqrt_once(q2);
            const double d = rr - (rho1 + rho2);
            if constexpr (PASS == 0) {
                al[j] = fma(wg0, d, al[j]);
                if constexpr (Q == 2) be[j] = fma(wg1, d, be[j]);
            } else {
                double e = d;
                if constexpr (Q >= 1) e = fma(-al[j], g0, e);
                if constexpr (Q == 2) e = fma(-be[j], g1, e);
                acc[j] = fma(w, e * e, acc[j]);
            }
        }
    }
}

template <int Q, int SRC>
__global__ __launch_bounds__(LOC_T) void k_locate_rtt(const LocSrc src, int64_t N, const double* __restrict__ rec, int64_t K,
                                                      const int64_t* __restrict__ set_starts, void* __restrict__ cost, int cost_f32,
                                                      double* __restrict__ part_v, int64_t* __restrict__ part_i) {
    __shared__ double s_rec[LOC_C * LOC_REC];
    __shared__ WaveSlots<LOC_T / 64, double, long long> s_best;
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * LOC_P;
    const int set = blockIdx.y;

    int64_t k0, k1;
    set_records(set_starts, set, K, k0, k1);
    const bool once = k1 - k0 <= LOC_C;  // the whole set is one chunk: pass 2 finds it in LDS

    double px[LOC_PPT], py[LOC_PPT], pz[LOC_PPT], al[LOC_PPT], be[LOC_PPT], acc[LOC_PPT];
    loc_points<SRC, LOC_T, LOC_PPT>(src, N, base, tid, px, py, pz);
#pragma unroll
    for (int j = 0; j < LOC_PPT; j++) al[j] = be[j] = acc[j] = 0.0;

    auto stage = [&](int64_t kc, int nrec) {
        const double* g = rec + kc * LOC_REC;
        for (int q = tid; q < nrec * LOC_REC; q += LOC_T) s_rec[q] = g[q];
        __syncthreads();
    };
    if constexpr (Q > 0) {
        for (int64_t kc = k0; kc < k1; kc += LOC_C) {
            const int nrec = (int)std::min<int64_t>(LOC_C, k1 - kc);
            stage(kc, nrec);
            rtt_chunk<Q, 0>(s_rec, nrec, px, py, pz, al, be, acc);
            if (!once) __syncthreads();  // the chunk is overwritten next
        }
    }
    for (int64_t kc = k0; kc < k1; kc += LOC_C) {
        const int nrec = (int)std::min<int64_t>(LOC_C, k1 - kc);
        if (Q == 0 || !once) stage(kc, nrec);
        rtt_chunk<Q, 1>(s_rec, nrec, px, py, pz, al, be, acc);
        if (!once) __syncthreads();
    }
    put_costs(s_best, acc, N, base, tid, set, cost, cost_f32, part_v, part_i);
}

// a search kernel, and what both entry points do once they have checked their own arguments: the shared checks, the launch of
// pick(source as a constant) over (workgroups, sets), and the fold of the partials when a minimum is asked for
using SearchKernel = void (*)(const LocSrc, int64_t, const double*, int64_t, const int64_t*, void*, int, double*, int64_t*);

template <class Pick>
int32_t grid_search(const char* entry, const caf_locate_desc* desc, const double* d_records, int64_t K, const int64_t* d_set_starts, int32_t B,
                    int per_set, Pick pick, void* d_cost, double* d_min_val, int64_t* d_min_idx, void* stream) {
    LocSrc src;
    int64_t N, tiles;
    int rc;
    if ((rc = grid_source(entry, desc, LOC_T, LOC_P, &src, &N, &tiles))) return rc;
    if ((rc = grid_sets_ok(entry, desc, d_records, K, d_set_starts, B, per_set))) return rc;
    const bool want_min = d_min_val != nullptr || d_min_idx != nullptr;
    if (!d_cost && !want_min) return CAF_OK;

    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    double* pv = nullptr;
    int64_t* pi = nullptr;
    if (want_min) {
        if ((rc = sc.get(&pv, (int64_t)B * tiles)) || (rc = sc.get(&pi, (int64_t)B * tiles))) return rc;
    }
    for_source(desc->source, [&](auto s) {
        const SearchKernel k = pick(s);
        hipLaunchKernelGGL(k, dim3((unsigned)tiles, (unsigned)B), dim3(LOC_T), 0, st, src, N, d_records, K, d_set_starts, d_cost,
                           desc->cost_f32, pv, pi);
    });
    CAF_HIP_TRY(hipGetLastError());
    if (want_min) {
        hipLaunchKernelGGL(k_grid_fold<false>, dim3((unsigned)B), dim3(GRID_FOLD_T), 0, st, GridParts{pv, pi, nullptr, nullptr}, tiles,
                           d_min_val, d_min_idx, (double*)nullptr, (int64_t*)nullptr);
        CAF_HIP_TRY(hipGetLastError());
    }
    return sc.finish();
}

}  // namespace

}  // namespace caf

using namespace caf;

int32_t caf_locate_geometry(int32_t* points_per_workgroup, int32_t* records_per_chunk) {
    if (points_per_workgroup) *points_per_workgroup = LOC_P;
    if (records_per_chunk) *records_per_chunk = LOC_C;
    return CAF_OK;
}

int32_t caf_locate_grid(const caf_locate_desc* desc, const double* d_records, int64_t K, const int64_t* d_set_starts, int32_t B,
                        void* d_cost, double* d_min_val, int64_t* d_min_idx, void* stream) {
    CAF_REQUIRE(desc != nullptr, "caf_locate_grid: NULL descriptor");
    CAF_REQUIRE(desc->mode == CAF_LOCATE_TD || desc->mode == CAF_LOCATE_FD || desc->mode == CAF_LOCATE_TDFD,
                "caf_locate_grid: mode must be CAF_LOCATE_TD, CAF_LOCATE_FD or CAF_LOCATE_TDFD");
    const int mode = desc->mode;
    const auto pick = [mode](auto s) -> SearchKernel {
        constexpr int SRC = decltype(s)::value;
        return mode == CAF_LOCATE_TD ? k_locate<true, false, SRC> : mode == CAF_LOCATE_FD ? k_locate<false, true, SRC> : k_locate<true, true, SRC>;
    };
    return grid_search("caf_locate_grid", desc, d_records, K, d_set_starts, B, 1, pick, d_cost, d_min_val, d_min_idx, stream);
}

int32_t caf_locate_rtt_geometry(int32_t* points_per_workgroup, int32_t* records_per_chunk) {
    return caf_locate_geometry(points_per_workgroup, records_per_chunk);  // (k_locate's frame)
}

int32_t caf_locate_rtt(const caf_locate_desc* desc, const double* d_records, int64_t K, const int64_t* d_set_starts, int32_t B,
                       int32_t nuisance, void* d_cost, double* d_min_val, int64_t* d_min_idx, void* stream) {
    CAF_REQUIRE(nuisance >= 0 && nuisance <= 2, "caf_locate_rtt: nuisance must be 0, 1 or 2");
    const auto pick = [nuisance](auto s) -> SearchKernel {
        constexpr int SRC = decltype(s)::value;
        return nuisance == 0 ? k_locate_rtt<0, SRC> : nuisance == 1 ? k_locate_rtt<1, SRC> : k_locate_rtt<2, SRC>;
    };
    return grid_search("caf_locate_rtt", desc, d_records, K, d_set_starts, B, nuisance + 1, pick, d_cost, d_min_val, d_min_idx, stream);
}
