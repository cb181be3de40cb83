// What the kernels that visit a grid of candidate positions share (caf_locate.hip: k_locate; caf_crbmap.hip: k_crb_map): the point
// source, the reciprocal square root and the loop that forms a thread's points.  Device code only; each includer passes its own
// threads per workgroup and points per thread, so the index arithmetic is one text compiled for both geometries.
#pragma once

#include <algorithm>
#include <cstdint>

#include "caf_internal.h"

namespace caf {

namespace {

struct LocSrc {
    const double* pts;                  // CAF_LOCATE_POINTS: (n, 3)
    const double *a, *z, *c, *s;        // meshes: a, z of ni entries (XY: a = Y), c, s of nj entries (XY: c = X)
    double z0;                          // XY: the constant height
    int32_t ni, nj;
    int32_t step_i, step_j;             // LOC_T / nj and LOC_T % nj: the mesh coordinates of a thread's next point
};

// 1 / sqrt(x), x > 0 finite: the hardware estimate and one third-order correction (see the head of the file)
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

}  // namespace

}  // namespace caf
