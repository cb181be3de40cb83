// The frame of the entry points that visit every point of a candidate grid against a table of 16-double records, in sets
// (caf_locate.hip: caf_locate_grid, caf_locate_rtt; caf_crbmap.hip: caf_crb_map).  A member writes its record loop and what it
// makes of a point's sums; what stands around them is here, once:
//   host    grid_source (descriptor -> LocSrc, N, workgroups), grid_sets_ok (the table and its sets), for_source (the point source
//           as a compile-time constant)
//   device  loc_points and rsqrt_once; set_records (a set's records, clamped into the table); store_value (float32 or float64);
//           thread_first_min / thread_first_max (a thread's own extreme, first of equals); k_grid_fold (the workgroups' partials
//           -> one (value, index) per set, or (NaN, -1))
// The copy of a record chunk into LDS is three lines in each kernel: as an inlined helper it cost six of the 21 kernels two VGPRs.
// Each includer passes its own threads per workgroup and points per thread, so the index arithmetic is one text compiled for
// both geometries.  Everything is in the anonymous namespace: no device function crosses a translation unit.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <type_traits>

#include "caf_internal.h"
#include "caf_wave.h"

// No contraction from here on: the costs and the Fisher sums are rounded where they are written, and each fma is spelled.
#pragma clang fp contract(off)

namespace caf {

namespace {

constexpr long long NO_INDEX = INT64_MAX;  // no value yet: loses every tie, and what the fold turns into (NaN, -1)
constexpr int GRID_FOLD_T = 256;           // threads of k_grid_fold

struct LocSrc {
    const double* pts;                  // CAF_LOCATE_POINTS: (n, 3)
    const double *a, *z, *c, *s;        // meshes: a, z of ni entries (XY: a = Y), c, s of nj entries (XY: c = X)
    double z0;                          // XY: the constant height
    int32_t ni, nj;
    int32_t step_i, step_j;             // threads / nj and threads % nj: the mesh coordinates of a thread's next point
};

// where the workgroups' partials go (a search has no maxima)
struct GridParts {
    double* min_v;
    int64_t* min_i;
    double* max_v;
    int64_t* max_i;
};

// ---- host ------------------------------------------------------------------------------------------------------------------------

// the descriptor's point source for workgroups of `threads` threads and `points` points, or a refusal in the entry point's name
inline int32_t grid_source(const char* entry, const caf_locate_desc* desc, int threads, int points, LocSrc* src, int64_t* N, int64_t* tiles) {
    const auto why = [entry](const char* what) { return std::string(entry) + ": " + what; };  // (formed only for a refusal)
    CAF_REQUIRE(desc != nullptr, why("NULL descriptor"));
    *src = {};
    if (desc->source == CAF_LOCATE_POINTS) {
        *N = desc->n;
        CAF_REQUIRE(*N >= 1, why("the point matrix needs at least one row"));
        CAF_REQUIRE(desc->d_points != nullptr, why("NULL point matrix"));
        src->pts = desc->d_points;
    } else if (desc->source == CAF_LOCATE_MESH || desc->source == CAF_LOCATE_MESH_XY) {
        CAF_REQUIRE(desc->ni >= 1 && desc->nj >= 1, why("the mesh needs ni >= 1 and nj >= 1"));
        *N = (int64_t)desc->ni * desc->nj;
        CAF_REQUIRE(desc->d_a != nullptr && desc->d_c != nullptr, why("NULL mesh table"));
        if (desc->source == CAF_LOCATE_MESH) {
            CAF_REQUIRE(desc->d_z != nullptr && desc->d_s != nullptr, why("NULL mesh table"));
        }
        src->a = desc->d_a;
        src->z = desc->d_z;
        src->c = desc->d_c;
        src->s = desc->d_s;
        src->z0 = desc->z;
        src->ni = desc->ni;
        src->nj = desc->nj;
        src->step_i = threads / desc->nj;
        src->step_j = threads % desc->nj;
    } else {
        CAF_REQUIRE(false, why("unknown point source"));
    }
    *tiles = (*N + points - 1) / points;
    CAF_REQUIRE(*tiles <= 0x7fffffff, why("too many points for one launch"));
    return CAF_OK;
}

// the table, its sets (each needs `per_set` records) and the store's width
inline int32_t grid_sets_ok(const char* entry, const caf_locate_desc* desc, const double* d_records, int64_t K, const int64_t* d_set_starts,
                            int32_t B, int per_set) {
    const auto why = [entry](const char* what) { return std::string(entry) + ": " + what; };  // (formed only for a refusal)
    CAF_REQUIRE(desc->cost_f32 == 0 || desc->cost_f32 == 1, why("cost_f32 must be 0 or 1"));
    CAF_REQUIRE(K >= 1 && K <= ((int64_t)1 << 40), why("the table needs at least one record"));
    CAF_REQUIRE(B >= 1 && B <= 65535 && (d_set_starts != nullptr || B == 1), why("1 <= sets <= 65535, and more than one set needs set_starts"));
    CAF_REQUIRE((int64_t)B * per_set <= K,
                why(per_set == 1 ? "every set needs at least one record" : "every set needs more records than nuisance parameters"));
    CAF_REQUIRE(d_records != nullptr, why("NULL record table"));
    return CAF_OK;
}

// f(std::integral_constant<int, SRC>) for the (validated) source
template <class F>
void for_source(int source, F&& f) {
    if (source == CAF_LOCATE_POINTS) f(std::integral_constant<int, CAF_LOCATE_POINTS>{});
    else if (source == CAF_LOCATE_MESH) f(std::integral_constant<int, CAF_LOCATE_MESH>{});
    else f(std::integral_constant<int, CAF_LOCATE_MESH_XY>{});
}

// ---- device ----------------------------------------------------------------------------------------------------------------------

// 1 / sqrt(x), x > 0 finite: the hardware estimate and one third-order correction (see the head of caf_locate.hip)
__device__ __forceinline__ double rsqrt_once(double x) {
    const double y0 = __builtin_amdgcn_rsq(x);
    const double t = x * y0;
    const double e = fma(-t, y0, 1.0);
    return fma(y0 * e, fma(e, 0.375, 0.5), y0);
}

// the thread's points (one past the end repeats the last point and stores nothing)
template <int SRC, int LOC_T, int LOC_PPT>
__device__ __forceinline__ void loc_points(const LocSrc& src, int64_t N, int64_t base, int tid, double (&px)[LOC_PPT], double (&py)[LOC_PPT],
                                           double (&pz)[LOC_PPT]) {
    if constexpr (SRC == CAF_LOCATE_POINTS) {
#pragma unroll
        for (int j = 0; j < LOC_PPT; j++) {
            const int64_t at = std::min(base + tid + j * LOC_T, N - 1);
            px[j] = src.pts[3 * at];
            py[j] = src.pts[3 * at + 1];
            pz[j] = src.pts[3 * at + 2];
        }
    } else {
        const int64_t at = std::min(base + tid, N - 1);
        int32_t mi, mj;
        if (N <= (int64_t)UINT32_MAX) {
            mi = (int32_t)((uint32_t)at / (uint32_t)src.nj);
            mj = (int32_t)((uint32_t)at - (uint32_t)mi * (uint32_t)src.nj);
        } else {
            mi = (int32_t)(at / src.nj);
            mj = (int32_t)(at - (int64_t)mi * src.nj);
        }
#pragma unroll
        for (int j = 0; j < LOC_PPT; j++) {
            const int32_t ci = std::min(mi, src.ni - 1);
            if constexpr (SRC == CAF_LOCATE_MESH) {
                const double a = src.a[ci];
                px[j] = a * src.c[mj];
                py[j] = a * src.s[mj];
                pz[j] = src.z[ci];
            } else {
                px[j] = src.c[mj];
                py[j] = src.a[ci];
                pz[j] = src.z0;
            }
            mi += src.step_i;
            mj += src.step_j;
            if (mj >= src.nj) {
                mj -= src.nj;
                mi++;
            }
        }
    }
}

// the records [k0, k1) of a set, clamped into the table whatever the offsets say
__device__ __forceinline__ void set_records(const int64_t* set_starts, int set, int64_t K, int64_t& k0, int64_t& k1) {
    k0 = 0, k1 = K;
    if (set_starts) {
        k0 = std::min(std::max<int64_t>(set_starts[set], 0), K);
        k1 = std::min(std::max<int64_t>(set_starts[set + 1], k0), K);
    }
}

__device__ __forceinline__ void store_value(void* out, int f32, int64_t o, double v) {
    if (f32) ((float*)out)[o] = (float)v;
    else ((double*)out)[o] = v;
}

// the first minimum (maximum) of the thread's points base + tid + j T below N, visited in increasing index
template <int T, int PPT>
__device__ __forceinline__ void thread_first_min(const double (&v)[PPT], int64_t N, int64_t base, int tid, double& bv, long long& bi) {
    bv = INFINITY, bi = NO_INDEX;
#pragma unroll
    for (int j = 0; j < PPT; j++) {
        const int64_t at = base + tid + j * T;
        if (at < N && first_min(bv, bi, v[j], (long long)at)) bv = v[j], bi = at;
    }
}
template <int T, int PPT>
__device__ __forceinline__ void thread_first_max(const double (&v)[PPT], int64_t N, int64_t base, int tid, double& bv, long long& bi) {
    bv = -INFINITY, bi = NO_INDEX;
#pragma unroll
    for (int j = 0; j < PPT; j++) {
        const int64_t at = base + tid + j * T;
        if (at < N && first_max(bv, bi, v[j], (long long)at)) bv = v[j], bi = at;
    }
}

// the partials of set blockIdx.x (in increasing order of workgroup, so of index) -> the set's minimum, and with MAX its maximum;
// nothing but NaN: (NaN, -1)
template <bool MAX>
__global__ __launch_bounds__(GRID_FOLD_T) void k_grid_fold(const GridParts parts, int64_t nparts, double* __restrict__ min_val,
                                                           int64_t* __restrict__ min_idx, double* __restrict__ max_val,
                                                           int64_t* __restrict__ max_idx) {
    __shared__ WaveSlots<GRID_FOLD_T / 64, double, long long> s_lo;
    const int64_t o = (int64_t)blockIdx.x * nparts;
    double lo = INFINITY, hi = -INFINITY;
    long long li = NO_INDEX, hi_i = NO_INDEX;
    for (int64_t e = threadIdx.x; e < nparts; e += GRID_FOLD_T) {
        const double a = parts.min_v[o + e];
        const long long ai = (long long)parts.min_i[o + e];
        if (first_min(lo, li, a, ai)) lo = a, li = ai;
        if constexpr (MAX) {
            const double b = parts.max_v[o + e];
            const long long bi = (long long)parts.max_i[o + e];
            if (first_max(hi, hi_i, b, bi)) hi = b, hi_i = bi;
        }
    }
    block_argmin(s_lo, lo, li);
    if constexpr (MAX) {
        __shared__ WaveSlots<GRID_FOLD_T / 64, double, long long> s_hi;
        block_argmax(s_hi, hi, hi_i);
    }
    if (threadIdx.x == 0) {
        const bool no_lo = li == NO_INDEX;
        if (min_val) min_val[blockIdx.x] = no_lo ? (double)NAN : lo;
        if (min_idx) min_idx[blockIdx.x] = no_lo ? (int64_t)-1 : (int64_t)li;
        if constexpr (MAX) {
            const bool no_hi = hi_i == NO_INDEX;
            if (max_val) max_val[blockIdx.x] = no_hi ? (double)NAN : hi;
            if (max_idx) max_idx[blockIdx.x] = no_hi ? (int64_t)-1 : (int64_t)hi_i;
        }
    }
}

}  // namespace

}  // namespace caf
