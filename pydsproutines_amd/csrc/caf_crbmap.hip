// CRB accuracy maps (crbRoutines.py: CRBMap): the Cramer-Rao bound of a position fix at every point of a grid, in float64.  For a
// grid point p and the record k = (s1, s2, v1, v2, w, kind, 0, 0), with a = p - s, rho = |a|, u = a / rho, the record adds
// w J J^T to the point's 3 x 3 Fisher matrix F (six running sums xx xy xz yy yz zz, in the order of k):
//   kind 1 (RANGE)      J = u1                                       kind 2 (RANGE_SUM)  J = u1 + u2
//   kind 3 (RANGE_DIFF) J = u2 - u1                                  kind 4 (RATE_DIFF)  J = g2 - g1, g = (v - u (u.v)) / rho
//   kind 5 (AOA3D)      two rows about s1, with h = ax^2 + ay^2:     (-ay, ax, 0) / (sqrt(h) rho)     [cos(theta) dphi]
//                                                                    (-az ax, -az ay, h) / (rho^2 sqrt(h))   [dtheta]
//   any other kind: F is NaN, so every point of that set is NaN.
// Then, with a normal n (FIXED: the caller's; RADIAL: p; WGS84: (px / a^2, py / a^2, pz / b^2)), e = z^ x n = (-ny, nx, 0), or x^
// where that vanishes, east = e / |e|, north = n^ x east, U = [east north]:
//   G = U^T F U,  C2 = G^-1,  CRB = U C2 U^T,  rms = sqrt(C2_11 + C2_22)  (the trace of CRB: U has orthonormal columns),
//   ellipse = (sqrt(lmax), sqrt(lmin), angle), lmax = (c11 + c22) / 2 + sqrt(((c11 - c22) / 2)^2 + c12^2), lmin = 1 / (det G lmax),
//   angle = atan2(2 c12, c11 - c22) / 2 in (-pi/2, pi/2], from east toward north.
// FREE: C = F^-1 through L D L^T, rms = sqrt(Cxx + Cyy + Czz).  A point is unobservable, NaN in every output, when a pivot of the
// L D L^T of G (or F) is not above CRB_SINGULAR = 2^-40 times its diagonal entry: below that more than 40 of the 53 bits of the
// Fisher matrix are lost to cancellation and the inverse is rounding noise.  det G = G11 G22 - G12^2 is a difference of products
// with an fma for the residual (its error is relative to det G itself), and the second pivot is det G / G11.
//
//   k_crb_map<SRC>   one workgroup per CRB_P = 512 consecutive points (two per thread, 256 apart: 6 sums per point) and per set
//                    (blockIdx.y); records staged in LDS CRB_C = 64 at a time and read back as broadcasts; the kind of a record
//                    is one value for the whole wave (v_readfirstlane), so the switch on it is a scalar branch and a table of
//                    range differences never reads a velocity.  After the records every thread finishes its own points.
//   k_grid_fold<true>  (caf_grid.h) the workgroups' (min, index) and (max, index) partials of each set -> one pair each per set.
// The point source, the sets, the stores and the extremes are the frame of caf_grid.h, shared with caf_locate.hip.
// Arg min and arg max of rms as in caf_locate.hip: first of equal values, NaN never wins, through block_argmax and block_argmin of
// caf_wave.h, partials in pooled scratch, folded in increasing order of workgroup; no atomics.
//
// The error count, in units of eps = 2^-53 (tests/crb_ref.py repeats it and forms the bound from it):
//   u = a y, y = 1 / sqrt(a.a) by rsqrt_once: a is off by 1 per component relative to rho; y by 4 relative (1 from a, 1.5 from the
//   three roundings of a.a halved by the root, 1.5 from the correction, as counted in caf_locate.hip); the product rounds: 6 absolute.
//   kinds 1: c_J = 6; kinds 2, 3: 12 and the sum's rounding (|J| <= 2): c_J = 14; scale s = 1.
//   kind 4, V = sum_i |v_i|: u.v is off by 6 V (u) + 3 V (one product, two fma) = 9 V; t_i = v_i - u_i (u.v), |t_i| <= 2 V, by
//   6 V + 9 V + 2 V = 17 V; g_i = t_i y by 17 + 4 * 2 + 2 = 27 V / rho; the difference rounds once (2): c_J = 29, s = V1 / rho1 + V2 / rho2.
//   kind 5, |J| <= 1 / rho: the first row is a (1) times yh y (4 + 4 + 1) and one product: 11; the second row: az ax (3) or h (4),
//   y y yh (4 + 4 + 4 + 2) and one product: c_J = 19, s = 1 / rho1.
//   F_ij += (w J_i) J_j by one product and one fma: dF_ij = eps [c_J sum_k w s (|J_i| + |J_j|) + c_F sum_k w |J_i J_j|], c_F = 1 + T,
//   T the number of terms added (one rounding of w J_i, and each of the T fma rounds at most eps sum_k w |J_i J_j|).
//   U: n exact (WGS84: 2, the rounding of b^2 and the division); |e|^-1: 1 + 1.5 (+ 2); east: + 1 (+ 2) <= 7.5; n^ <= 8; north is
//   products and one difference of products of the two, 8 + 7.5 + 1 each and one rounding: c_U = 18 absolute per entry.
//   G = U^T (F U): dG = |U|^T dF |U| + c_G eps sum_ij |F_ij|, c_G = 2 c_U + 6 (three roundings in F U, three in U^T (F U)).
//   C2 = adj G / det G: dC2 = |C2| dG |C2| + c_I eps |C2|, c_I = 3 (det G within 2 eps of itself, one division).
//   CRB = U C2 U^T: dCRB = |U| dC2 |U|^T + (2 c_U + 6) eps sum_ab |C2_ab|.
//   FREE: dC = |C| dF |C| + c_L eps |C| D |C|, D_ij = sqrt(F_ii F_jj) >= (|L| |D| |L^T|)_ij, c_L = 16 (4 in the factors, 3 in L^-1,
//   9 in the three-term entries of L^-T D^-1 L^-1).
//   rms: (the diagonal's bounds) / (2 rms) + 3 eps rms (two sums at most, and the root).  lmax, lmin: sum_ab dC2_ab + c_E eps lmax, c_E = 16 (the mean,
//   the half difference, the root of an fma, the sum: 5; lmin from det G lmax and a division: 5; the roots and atan2: the rest).
// Floating-point contraction is off in this file: every product and sum is rounded where it is written, and each fma is spelled.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "caf_internal.h"
#include "caf_grid.h"
#include "caf_wave.h"

#pragma clang fp contract(off)

namespace caf {

namespace {

constexpr int CRB_T = 256;              // threads per workgroup
constexpr int CRB_PPT = 2;              // points per thread
constexpr int CRB_P = CRB_T * CRB_PPT;  // points per workgroup
constexpr int CRB_C = 64;               // records per LDS chunk (8 KiB)
constexpr int CRB_REC = 16;             // doubles per record: s1(3) s2(3) v1(3) v2(3) w kind 0 0
constexpr double CRB_SINGULAR = 0x1p-40;
constexpr double WGS84_A = 6378137.0, WGS84_INV_F = 298.257223563;

struct CrbNormal {
    double nx, ny, nz;  // CAF_CRB_FIXED
    double a2, b2;      // CAF_CRB_WGS84: the squared semi-axes
};

// F += w J J^T
__device__ __forceinline__ void add_outer(double (&f)[6], double w, double jx, double jy, double jz) {
    const double wx = w * jx, wy = w * jy, wz = w * jz;
    f[0] = fma(wx, jx, f[0]);
    f[1] = fma(wx, jy, f[1]);
    f[2] = fma(wx, jz, f[2]);
    f[3] = fma(wy, jy, f[3]);
    f[4] = fma(wy, jz, f[4]);
    f[5] = fma(wz, jz, f[5]);
}

// a b - c d with the residual of c d taken by an fma: within 2 eps of the exact difference
__device__ __forceinline__ double diff_of_products(double a, double b, double c, double d) {
    const double w = c * d;
    const double e = fma(-c, d, w);
    const double f = fma(a, b, -w);
    return f + e;
}

template <int SRC>
__global__ __launch_bounds__(CRB_T) void k_crb_map(const LocSrc src, int64_t N, const double* __restrict__ rec, int64_t K,
                                                   const int64_t* __restrict__ set_starts, int constraint, const CrbNormal nrm,
                                                   double* __restrict__ crb, double* __restrict__ ell, void* __restrict__ rms,
                                                   int rms_f32, const GridParts parts) {  // (all four partials or none)
    __shared__ double s_rec[CRB_C * CRB_REC];
    __shared__ WaveSlots<CRB_T / 64, double, long long> s_lo, s_hi;
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * CRB_P;
    const int set = blockIdx.y;

    int64_t k0, k1;
    set_records(set_starts, set, K, k0, k1);

    double px[CRB_PPT], py[CRB_PPT], pz[CRB_PPT], f[CRB_PPT][6];
    loc_points<SRC, CRB_T, CRB_PPT>(src, N, base, tid, px, py, pz);
#pragma unroll
    for (int j = 0; j < CRB_PPT; j++)
#pragma unroll
        for (int q = 0; q < 6; q++) f[j][q] = 0.0;

    for (int64_t kc = k0; kc < k1; kc += CRB_C) {
        const int nrec = (int)std::min<int64_t>(CRB_C, k1 - kc);
        const double* g = rec + kc * CRB_REC;
        for (int q = tid; q < nrec * CRB_REC; q += CRB_T) s_rec[q] = g[q];
        __syncthreads();
        for (int k = 0; k < nrec; k++) {
            const double* r = s_rec + k * CRB_REC;  // the same address in every lane: broadcast reads
            const double s1x = r[0], s1y = r[1], s1z = r[2], w = r[12], kd = r[13];
            // the kind as one scalar for the wave; a value that is no small integer (NaN included) falls to the default
            const int kind = __builtin_amdgcn_readfirstlane(kd >= 1.0 && kd <= 5.0 && kd == (double)(int)kd ? (int)kd : 0);
            switch (kind) {
                case CAF_CRB_RANGE: {
#pragma unroll
                    for (int j = 0; j < CRB_PPT; j++) {
                        const double ax = px[j] - s1x, ay = py[j] - s1y, az = pz[j] - s1z;
                        const double y = rsqrt_once(fma(az, az, fma(ay, ay, ax * ax)));
                        add_outer(f[j], w, ax * y, ay * y, az * y);
                    }
                    break;
                }
                case CAF_CRB_RANGE_SUM:
                case CAF_CRB_RANGE_DIFF: {
                    const double s2x = r[3], s2y = r[4], s2z = r[5];
                    const double sign = kind == CAF_CRB_RANGE_SUM ? 1.0 : -1.0;  // (u2 + u1 or u2 - u1: a product by 1 is exact)
#pragma unroll
                    for (int j = 0; j < CRB_PPT; j++) {
                        const double ax = px[j] - s1x, ay = py[j] - s1y, az = pz[j] - s1z;
                        const double bx = px[j] - s2x, by = py[j] - s2y, bz = pz[j] - s2z;
                        const double y1 = sign * rsqrt_once(fma(az, az, fma(ay, ay, ax * ax)));
                        const double y2 = rsqrt_once(fma(bz, bz, fma(by, by, bx * bx)));
                        add_outer(f[j], w, bx * y2 + ax * y1, by * y2 + ay * y1, bz * y2 + az * y1);
                    }
                    break;
                }
                case CAF_CRB_RATE_DIFF: {
                    const double s2x = r[3], s2y = r[4], s2z = r[5];
                    const double v1x = r[6], v1y = r[7], v1z = r[8], v2x = r[9], v2y = r[10], v2z = r[11];
#pragma unroll
                    for (int j = 0; j < CRB_PPT; j++) {
                        const double ax = px[j] - s1x, ay = py[j] - s1y, az = pz[j] - s1z;
                        const double bx = px[j] - s2x, by = py[j] - s2y, bz = pz[j] - s2z;
                        const double y1 = rsqrt_once(fma(az, az, fma(ay, ay, ax * ax)));
                        const double y2 = rsqrt_once(fma(bz, bz, fma(by, by, bx * bx)));
                        const double u1x = ax * y1, u1y = ay * y1, u1z = az * y1;
                        const double u2x = bx * y2, u2y = by * y2, u2z = bz * y2;
                        const double d1 = fma(u1z, v1z, fma(u1y, v1y, u1x * v1x));
                        const double d2 = fma(u2z, v2z, fma(u2y, v2y, u2x * v2x));
                        const double jx = fma(-u2x, d2, v2x) * y2 - fma(-u1x, d1, v1x) * y1;
                        const double jy = fma(-u2y, d2, v2y) * y2 - fma(-u1y, d1, v1y) * y1;
                        const double jz = fma(-u2z, d2, v2z) * y2 - fma(-u1z, d1, v1z) * y1;
                        add_outer(f[j], w, jx, jy, jz);
                    }
                    break;
                }
                case CAF_CRB_AOA3D: {
#pragma unroll
                    for (int j = 0; j < CRB_PPT; j++) {
                        const double ax = px[j] - s1x, ay = py[j] - s1y, az = pz[j] - s1z;
                        const double h = fma(ay, ay, ax * ax);
                        const double yh = rsqrt_once(h), y = rsqrt_once(fma(az, az, h));
                        const double c1 = yh * y;
                        add_outer(f[j], w, -ay * c1, ax * c1, 0.0);
                        const double c2 = (y * y) * yh;
                        const double naz = -az;
                        add_outer(f[j], w, (naz * ax) * c2, (naz * ay) * c2, h * c2);
                    }
                    break;
                }
                default: {
#pragma unroll
                    for (int j = 0; j < CRB_PPT; j++) f[j][0] = NAN;
                    break;
                }
            }
        }
        __syncthreads();  // the chunk is overwritten next
    }

    // every thread finishes its own points
    const double qnan = NAN;
    double val[CRB_PPT];
    const int64_t out0 = (int64_t)set * N;
#pragma unroll
    for (int j = 0; j < CRB_PPT; j++) {
        const int64_t at = base + tid + j * CRB_T;
        const double fxx = f[j][0], fxy = f[j][1], fxz = f[j][2], fyy = f[j][3], fyz = f[j][4], fzz = f[j][5];
        double c[6], e3[3] = {qnan, qnan, qnan}, tr;
        bool ok;
        if (constraint == CAF_CRB_FREE) {
            // F = L D L^T, C = L^-T D^-1 L^-1
            const double d1 = fxx;
            const double l21 = fxy / d1, l31 = fxz / d1;
            const double d2 = fma(-l21, fxy, fyy);
            const double t32 = fma(-l31, fxy, fyz);
            const double l32 = t32 / d2;
            const double d3 = fma(-l32, t32, fma(-l31, fxz, fzz));
            ok = d1 > CRB_SINGULAR * fxx && d2 > CRB_SINGULAR * fyy && d3 > CRB_SINGULAR * fzz;
            const double m31 = fma(l21, l32, -l31);  // L^-1 = [1 0 0; -l21 1 0; m31 -l32 1]
            const double i1 = 1.0 / d1, i2 = 1.0 / d2, i3 = 1.0 / d3;
            const double m31i = m31 * i3, l32i = l32 * i3;
            c[5] = i3;
            c[4] = -l32i;
            c[3] = fma(l32, l32i, i2);
            c[2] = m31i;
            c[1] = fma(-m31, l32i, -l21 * i2);
            c[0] = fma(m31, m31i, fma(l21, l21 * i2, i1));
            tr = (c[0] + c[3]) + c[5];
        } else {
            double nx = nrm.nx, ny = nrm.ny, nz = nrm.nz;
            if (constraint == CAF_CRB_RADIAL) nx = px[j], ny = py[j], nz = pz[j];
            if (constraint == CAF_CRB_WGS84) nx = px[j] / nrm.a2, ny = py[j] / nrm.a2, nz = pz[j] / nrm.b2;
            const double he = fma(ny, ny, nx * nx);
            const bool pole = he == 0.0;  // n along z: east is x^
            const double ye = rsqrt_once(pole ? 1.0 : he);
            const double ex = pole ? 1.0 : -ny * ye, ey = pole ? 0.0 : nx * ye;
            const double yn = rsqrt_once(fma(nz, nz, he));
            const double ux = nx * yn, uy = ny * yn, uz = nz * yn;
            const double qx = -uz * ey, qy = uz * ex, qz = diff_of_products(ux, ey, uy, ex);  // north = n^ x east
            // G = U^T (F U)
            const double fex = fma(fxy, ey, fxx * ex), fey = fma(fyy, ey, fxy * ex);
            const double fnx = fma(fxz, qz, fma(fxy, qy, fxx * qx)), fny = fma(fyz, qz, fma(fyy, qy, fxy * qx)),
                         fnz = fma(fzz, qz, fma(fyz, qy, fxz * qx));
            const double g11 = fma(ey, fey, ex * fex);
            const double g12 = fma(ey, fny, ex * fnx);
            const double g22 = fma(qz, fnz, fma(qy, fny, qx * fnx));
            const double det = diff_of_products(g11, g22, g12, g12);
            ok = g11 > CRB_SINGULAR * g11 && det / g11 > CRB_SINGULAR * g22;
            const double c11 = g22 / det, c12 = -g12 / det, c22 = g11 / det;
            tr = c11 + c22;
            // CRB = U C2 U^T (east has no z)
            const double ax = c11 * ex + c12 * qx, ay = c11 * ey + c12 * qy, az = c12 * qz;  // U C2, first column
            const double bx = c12 * ex + c22 * qx, by = c12 * ey + c22 * qy, bz = c22 * qz;  // second column
            c[0] = fma(bx, qx, ax * ex);
            c[1] = fma(bx, qy, ax * ey);
            c[2] = bx * qz;
            c[3] = fma(by, qy, ay * ey);
            c[4] = by * qz;
            c[5] = bz * qz;
            if (ell) {
                const double m = 0.5 * (c11 + c22), dd = 0.5 * (c11 - c22);
                const double lmax = m + sqrt(fma(dd, dd, c12 * c12));
                const double lmin = 1.0 / (det * lmax);
                double ang = 0.5 * atan2(2.0 * c12, c11 - c22);
                if (ang <= -0.5 * M_PI) ang = 0.5 * M_PI;
                e3[0] = sqrt(lmax), e3[1] = sqrt(lmin), e3[2] = ang;
            }
        }
        // (a NaN anywhere in F fails the comparisons above)
        const double v = ok ? sqrt(tr) : qnan;
        val[j] = v;
        if (at < N) {
            const int64_t o = out0 + at;
            if (crb) {
#pragma unroll
                for (int q = 0; q < 6; q++) crb[6 * o + q] = ok ? c[q] : qnan;
            }
            if (ell) {
#pragma unroll
                for (int q = 0; q < 3; q++) ell[3 * o + q] = ok ? e3[q] : qnan;
            }
            if (rms) store_value(rms, rms_f32, o, v);
        }
    }

    if (parts.min_v) {
        double lo, hi;
        long long li, hi_i;
        thread_first_min<CRB_T, CRB_PPT>(val, N, base, tid, lo, li);
        thread_first_max<CRB_T, CRB_PPT>(val, N, base, tid, hi, hi_i);
        block_argmin(s_lo, lo, li);
        block_argmax(s_hi, hi, hi_i);
        if (tid == 0) {
            const int64_t o = (int64_t)set * gridDim.x + blockIdx.x;
            parts.min_v[o] = lo, parts.min_i[o] = (int64_t)li;
            parts.max_v[o] = hi, parts.max_i[o] = (int64_t)hi_i;
        }
    }
}

}  // namespace

}  // namespace caf

using namespace caf;

int32_t caf_crb_map_geometry(int32_t* points_per_workgroup, int32_t* records_per_chunk, double* singular_threshold) {
    if (points_per_workgroup) *points_per_workgroup = CRB_P;
    if (records_per_chunk) *records_per_chunk = CRB_C;
    if (singular_threshold) *singular_threshold = CRB_SINGULAR;
    return CAF_OK;
}

int32_t caf_crb_map(const caf_locate_desc* desc, const double* d_records, int64_t K, const int64_t* d_set_starts, int32_t B,
                    int32_t constraint, const double* normal, double* d_crb, double* d_ellipse, void* d_rms, double* d_min_val,
                    int64_t* d_min_idx, double* d_max_val, int64_t* d_max_idx, void* stream) {
    LocSrc src;
    int64_t N, tiles;
    int rc;
    if ((rc = grid_source("caf_crb_map", desc, CRB_T, CRB_P, &src, &N, &tiles))) return rc;
    if ((rc = grid_sets_ok("caf_crb_map", desc, d_records, K, d_set_starts, B, 1))) return rc;
    CAF_REQUIRE(constraint == CAF_CRB_FREE || constraint == CAF_CRB_FIXED || constraint == CAF_CRB_RADIAL || constraint == CAF_CRB_WGS84,
                "caf_crb_map: constraint must be CAF_CRB_FREE, CAF_CRB_FIXED, CAF_CRB_RADIAL or CAF_CRB_WGS84");
    CrbNormal nrm = {0.0, 0.0, 0.0, WGS84_A * WGS84_A, 0.0};
    const double wgs_b = WGS84_A * (1.0 - 1.0 / WGS84_INV_F);
    nrm.b2 = wgs_b * wgs_b;
    if (constraint == CAF_CRB_FIXED) {
        CAF_REQUIRE(normal != nullptr, "caf_crb_map: CAF_CRB_FIXED needs a normal");
        CAF_REQUIRE(std::isfinite(normal[0]) && std::isfinite(normal[1]) && std::isfinite(normal[2]) &&
                        (normal[0] != 0.0 || normal[1] != 0.0 || normal[2] != 0.0),
                    "caf_crb_map: the fixed normal must be finite and not zero");
        nrm.nx = normal[0], nrm.ny = normal[1], nrm.nz = normal[2];
    }
    CAF_REQUIRE(!(constraint == CAF_CRB_FREE && d_ellipse != nullptr), "caf_crb_map: no ellipse of an unconstrained 3 x 3 (CAF_CRB_FREE)");
    CAF_REQUIRE(d_min_idx == nullptr || d_min_val != nullptr, "caf_crb_map: d_min_idx needs d_min_val");
    CAF_REQUIRE(d_max_idx == nullptr || d_max_val != nullptr, "caf_crb_map: d_max_idx needs d_max_val");
    const bool want_fold = d_min_val != nullptr || d_max_val != nullptr;
    if (!d_crb && !d_ellipse && !d_rms && !want_fold) return CAF_OK;

    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    GridParts parts = {};
    if (want_fold) {
        const int64_t np = (int64_t)B * tiles;
        if ((rc = sc.get(&parts.min_v, np)) || (rc = sc.get(&parts.min_i, np)) || (rc = sc.get(&parts.max_v, np)) ||
            (rc = sc.get(&parts.max_i, np)))
            return rc;
    }
    const dim3 grid((unsigned)tiles, (unsigned)B);
    for_source(desc->source, [&](auto s) {
        hipLaunchKernelGGL(k_crb_map<decltype(s)::value>, grid, dim3(CRB_T), 0, st, src, N, d_records, K, d_set_starts, constraint, nrm, d_crb,
                           d_ellipse, d_rms, desc->cost_f32, parts);
    });
    CAF_HIP_TRY(hipGetLastError());
    if (want_fold) {
        hipLaunchKernelGGL(k_grid_fold<true>, dim3((unsigned)B), dim3(GRID_FOLD_T), 0, st, parts, tiles, d_min_val, d_min_idx, d_max_val,
                           d_max_idx);
        CAF_HIP_TRY(hipGetLastError());
    }
    return sc.finish();
}
