// Lines of position on an oblate spheroid (hyperboloidRoutines.py, sphereRoutines.py, localizationRoutines.py: linesOfPosition,
// rangeCircles): the curve on the Earth where one measured range difference, or one measured range, is satisfied, in float64.
// A job (mu, e0, e1, e2, a, c, p_min, p_max) is a one-parameter family of circles q(phi) = C(p) + A(p) cos phi + B(p) sin phi,
//   hyperboloid sheet: C = mu - c cosh p e2, A = a sinh p e0, B = a sinh p e1;      sphere: C = mu + c cos p e2, A = a sin p e0, B = a sin p e1,
// and with the circle's vectors divided through by the semi-axes (x and y by omega, z by lambda: every k is of order 1)
//   g(phi) = E(q(phi)) = k0 + k1 cos phi + k2 sin phi + k3 cos 2 phi + k4 sin 2 phi
//   k0 = C.C + (A.A + B.B) / 2 - 1, k1 = 2 C.A, k2 = 2 C.B, k3 = (A.A - B.B) / 2, k4 = A.B.
//
// The zeros of g at p (lop_zeros, the one device function both kernels call: a parameter that k_lop_range reports has a zero in
// k_lop_points too, bit for bit):
//   1. g is sampled at the 16 angles j pi / 8; the angle of the largest |g| becomes the pole of the substitution
//      t = tan((phi - phi0) / 2), phi0 = pole - pi.  The 16 squares sum to 16 (k0^2 + (k1^2 + ... + k4^2) / 2), so that |g| is at
//      least a third of sum |k| while |g'| <= 2 sum |k|: no zero lies within 0.15 rad of the pole and every root has |t| < 14.
//   2. (1 + t^2)^2 g = a4 t^4 + ... + a0 with a4 = g(pole); divided by a4 it is monic, P, and all its roots lie in |t| <= T, T = 1 + max |b_i|.
//   3. P'' is a quadratic (closed form); its roots cut [-T, T] into at most three pieces on each of which P' is monotone: a sign change
//      of P' over a piece is bisected LOP_N1 times -> the stationary points of P (an error e there moves P by P'' e^2 / 2 only).
//   4. The stationary points cut [-T, T] into at most four pieces on each of which P is monotone: a sign change of P over a piece
//      is one zero, bisected LOP_N2 times.  The count is decided by the signs of P at its stationary points and at +-T alone.
//   5. phi = phi0 + 2 atan t, then LOP_NEWTON Newton steps on g itself in phi (a step above LOP_STEP is not taken), wrapped into
//      (-pi, pi] and sorted.
// Every loop has a trip count fixed at compile time.  "x < 0" is the only sign test: a NaN anywhere has no sign change and ends
// with count 0; a job that is not finite, or has A = B = 0 at p, is given count 0 before any of it.
//
//   k_lop_points   one thread per (job, sample), LOP_S = 256 samples per workgroup, samples of consecutive jobs packed together.
//   k_lop_range    one wave per job, LOP_W = 4 jobs per workgroup: LOP_ROUNDS = 4 rounds of 64 parameters, one per lane, folded by
//                  one ballot each; the lower end's three refinements, then the upper end's.
// Floating-point contraction is off in this file: every product and sum is rounded where it is written, and each fma is spelled.
#include <cmath>
#include <cstdint>

#include "caf_internal.h"

#pragma clang fp contract(off)

namespace caf {

namespace {

constexpr int LOP_S = 256;      // threads, and samples, per workgroup of k_lop_points
constexpr int LOP_W = 4;        // jobs (waves) per workgroup of k_lop_range
constexpr int LOP_ROUNDS = 4;   // search rounds of k_lop_range
constexpr int LOP_WIDTH = 64;   // parameters per round: one per lane
constexpr int LOP_REC = 16;     // doubles per job
constexpr int LOP_N1 = 30;      // bisections of a stationary point of P
constexpr int LOP_N2 = 40;      // bisections of a zero of P
constexpr int LOP_NEWTON = 3;   // Newton steps on g
constexpr double LOP_STEP = 1e-3;  // the largest Newton step taken (rad)
constexpr double LOP_DEG = 180.0 / M_PI;

struct LopJob {
    double mu[3], e0[3], e1[3], e2[3], a, c, p_min, p_max;
};

struct LopCircle {
    double C[3], A[3], B[3];
};

__device__ __forceinline__ LopJob lop_load(const double* __restrict__ jobs, int64_t b) {
    const double* r = jobs + b * LOP_REC;
    LopJob j;
#pragma unroll
    for (int i = 0; i < 3; i++) j.mu[i] = r[i], j.e0[i] = r[3 + i], j.e1[i] = r[6 + i], j.e2[i] = r[9 + i];
    j.a = r[12], j.c = r[13], j.p_min = r[14], j.p_max = r[15];
    return j;
}

__device__ __forceinline__ double dot3(const double (&x)[3], const double (&y)[3]) { return fma(x[2], y[2], fma(x[1], y[1], x[0] * y[0])); }

// the circle of the job at p, and k0..k4 of its g
template <int KIND>
__device__ __forceinline__ void lop_circle(const LopJob& j, double p, double omega, double lambda, LopCircle& q, double (&k)[5]) {
    double sa, sc;
    if (KIND == CAF_LOP_HYPERBOLOID) {
        sa = j.a * sinh(p);
        sc = -(j.c * cosh(p));
    } else {
        sa = j.a * sin(p);
        sc = j.c * cos(p);
    }
    double ch[3], ah[3], bh[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double s = i < 2 ? omega : lambda;
        q.C[i] = fma(sc, j.e2[i], j.mu[i]);
        q.A[i] = sa * j.e0[i];
        q.B[i] = sa * j.e1[i];
        ch[i] = q.C[i] / s, ah[i] = q.A[i] / s, bh[i] = q.B[i] / s;
    }
    const double cc = dot3(ch, ch), aa = dot3(ah, ah), bb = dot3(bh, bh);
    k[0] = (cc + 0.5 * (aa + bb)) - 1.0;
    k[1] = 2.0 * dot3(ch, ah);
    k[2] = 2.0 * dot3(ch, bh);
    k[3] = 0.5 * (aa - bb);
    k[4] = dot3(ah, bh);
}

// g from the cosine and sine of phi: cos 2 phi = (c - s)(c + s), sin 2 phi = 2 s c
__device__ __forceinline__ double lop_g(const double (&k)[5], double c, double s) {
    const double c2 = (c - s) * (c + s), s2 = 2.0 * (s * c);
    return fma(k[4], s2, fma(k[3], c2, fma(k[2], s, fma(k[1], c, k[0]))));
}

__device__ __forceinline__ double lop_dg(const double (&k)[5], double c, double s) {
    const double c2 = (c - s) * (c + s), s2 = 2.0 * (s * c);
    return fma(2.0 * k[4], c2, fma(-2.0 * k[3], s2, fma(k[2], c, -k[1] * s)));
}

__device__ __forceinline__ double lop_wrap(double phi) {
    if (phi <= -M_PI) phi += 2.0 * M_PI;
    if (phi > M_PI) phi -= 2.0 * M_PI;
    return phi;
}

// the zeros of g in (-pi, pi], ascending, NaN behind them; their number
__device__ int lop_zeros(const double (&k)[5], double (&phi)[4]) {
    const double qnan = NAN;
#pragma unroll
    for (int i = 0; i < 4; i++) phi[i] = qnan;
    const double sum = fabs(k[0]) + fabs(k[1]) + fabs(k[2]) + fabs(k[3]) + fabs(k[4]);
    if (!(sum < INFINITY)) return 0;                                          // NaN or infinite
    if (k[1] == 0.0 && k[2] == 0.0 && k[3] == 0.0 && k[4] == 0.0) return 0;  // A = B = 0: no circle

    // 1. the pole: the first of the 16 angles j pi / 8 with the largest |g|
    constexpr double CS[5] = {1.0, 0.92387953251128674, 0.70710678118654752, 0.38268343236508977, 0.0};  // cos(j pi / 8), j = 0..4
    double best = -1.0, pc = 1.0, ps = 0.0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const int m = j & 7;  // cos(j pi / 8) = +-cos(m pi / 8) = +-CS[m] or -+CS[8 - m]
        const double c8 = m <= 4 ? CS[m] : -CS[8 - m], s8 = m <= 4 ? CS[4 - m] : CS[m - 4];
        const double c = j < 8 ? c8 : -c8, s = j < 8 ? s8 : -s8;
        const double v = fabs(lop_g(k, c, s));
        if (v > best) best = v, pc = c, ps = s;
    }
    // phi0 = pole - pi
    const double c0 = -pc, s0 = -ps;
    const double c20 = (c0 - s0) * (c0 + s0), s20 = 2.0 * (s0 * c0);
    const double phi0 = atan2(s0, c0);

    // 2. g(phi0 + psi) = k0 + r1 cos psi + r2 sin psi + r3 cos 2 psi + r4 sin 2 psi -> the monic quartic in t = tan(psi / 2)
    const double r1 = fma(k[2], s0, k[1] * c0), r2 = fma(-k[1], s0, k[2] * c0);
    const double r3 = fma(k[4], s20, k[3] * c20), r4 = fma(-k[3], s20, k[4] * c20);
    const double a4 = (k[0] - r1) + r3;
    const double b0 = ((k[0] + r1) + r3) / a4, b1 = fma(4.0, r4, 2.0 * r2) / a4, b2 = fma(-6.0, r3, 2.0 * k[0]) / a4,
                 b3 = fma(-4.0, r4, 2.0 * r2) / a4;
    const double T = 1.0 + fmax(fmax(fabs(b0), fabs(b1)), fmax(fabs(b2), fabs(b3)));
    if (!(T < INFINITY)) return 0;
    auto P = [&](double t) { return fma(fma(fma(t + b3, t, b2), t, b1), t, b0); };
    auto dP = [&](double t) { return fma(fma(fma(4.0, t, 3.0 * b3), t, 2.0 * b2), t, b1); };

    // 3. the stationary points of P between the roots of P'' = 2 (6 t^2 + 3 b3 t + b2)
    const double disc = fma(9.0 * b3, b3, -24.0 * b2);
    double cut[4] = {-T, 0.0, 0.0, T};
    if (disc > 0.0) {
        const double rt = sqrt(disc);
        cut[1] = fmin(fmax((-3.0 * b3 - rt) / 12.0, -T), T);
        cut[2] = fmin(fmax((-3.0 * b3 + rt) / 12.0, -T), T);
    }
    double stat[4] = {qnan, qnan, qnan, T};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double lo = cut[i], hi = cut[i + 1];
        const bool nlo = dP(lo) < 0.0;
        if (nlo != (dP(hi) < 0.0)) {
            for (int it = 0; it < LOP_N1; it++) {
                const double mid = 0.5 * (lo + hi);
                if ((dP(mid) < 0.0) == nlo) lo = mid;
                else hi = mid;
            }
            stat[i] = 0.5 * (lo + hi);
        }
    }

    // 4. one zero of P in every piece between stationary points over which it changes sign; 5. polished on g
    double prev = -T;
    int n = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (!(stat[i] == stat[i])) continue;  // no stationary point in that piece of step 3
        double lo = prev, hi = stat[i];
        prev = hi;
        const bool nlo = P(lo) < 0.0;
        if (nlo == (P(hi) < 0.0)) continue;
        for (int it = 0; it < LOP_N2; it++) {
            const double mid = 0.5 * (lo + hi);
            if ((P(mid) < 0.0) == nlo) lo = mid;
            else hi = mid;
        }
        double f = lop_wrap(phi0 + 2.0 * atan(0.5 * (lo + hi)));
        for (int it = 0; it < LOP_NEWTON; it++) {
            double s, c;
            sincos(f, &s, &c);
            const double step = lop_g(k, c, s) / lop_dg(k, c, s);
            if (fabs(step) <= LOP_STEP) f -= step;
        }
        phi[i] = lop_wrap(f);
        n++;
    }
    // ascending, NaN last: a network of five exchanges on the keys (NaN counts as +inf)
    auto exch = [&](int a, int b) {
        const double ka = phi[a] == phi[a] ? phi[a] : INFINITY, kb = phi[b] == phi[b] ? phi[b] : INFINITY;
        if (ka > kb) {
            const double t = phi[a];
            phi[a] = phi[b], phi[b] = t;
        }
    };
    exch(0, 1), exch(2, 3), exch(0, 2), exch(1, 3), exch(1, 2);
    return n;
}

struct LopOut {
    int32_t* count;
    double *phi, *xyz, *latlon, *p_out;
};

template <int KIND>
__global__ __launch_bounds__(LOP_S) void k_lop_points(const double* __restrict__ jobs, int64_t B, int32_t P, int spacing,
                                                      const double* __restrict__ plist, const double* __restrict__ range,
                                                      double omega, double lambda, const LopOut out) {
    const int64_t at = (int64_t)blockIdx.x * LOP_S + threadIdx.x;
    if (at >= B * (int64_t)P) return;
    const int64_t b = at / P;
    const int32_t j = (int32_t)(at - b * P);
    double p;
    if (spacing == CAF_LOP_LIST) {
        p = plist[j];
    } else {
        const double lo = range[2 * b], hi = range[2 * b + 1];
        if (spacing == CAF_LOP_LINSPACE) p = j == 0 ? lo : (j == P - 1 ? hi : lo + (double)j * ((hi - lo) / (double)(P - 1)));
        else p = lo + (hi - lo) * (0.5 * (1.0 - cos(M_PI * ((double)j + 0.5) / (double)P)));
    }
    const LopJob job = lop_load(jobs, b);
    LopCircle q;
    double k[5], phi[4];
    lop_circle<KIND>(job, p, omega, lambda, q, k);
    const int n = lop_zeros(k, phi);
    if (out.count) out.count[at] = n;
    if (out.p_out) out.p_out[at] = p;
    const double w2 = omega * omega, l2 = lambda * lambda;
#pragma unroll
    for (int z = 0; z < 4; z++) {
        const int64_t o = 4 * at + z;
        const double f = phi[z];  // NaN behind the zeros: everything below is NaN with it
        double s, c;
        sincos(f, &s, &c);
        double x[3];
#pragma unroll
        for (int i = 0; i < 3; i++) x[i] = fma(q.B[i], s, fma(q.A[i], c, q.C[i]));
        if (out.phi) out.phi[o] = f;
        if (out.xyz) {
#pragma unroll
            for (int i = 0; i < 3; i++) out.xyz[3 * o + i] = x[i];
        }
        if (out.latlon) {
            out.latlon[2 * o] = atan2(x[2] / l2, hypot(x[0], x[1]) / w2) * LOP_DEG;
            out.latlon[2 * o + 1] = atan2(x[1], x[0]) * LOP_DEG;
        }
    }
}

template <int KIND>
__global__ __launch_bounds__(LOP_W * 64) void k_lop_range(const double* __restrict__ jobs, int64_t B, double omega, double lambda,
                                                          double* __restrict__ range, int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * LOP_W + (threadIdx.x >> 6);
    if (b >= B) return;  // (the whole wave)
    const LopJob job = lop_load(jobs, b);
    auto hit = [&](double p) {
        LopCircle q;
        double k[5], phi[4];
        lop_circle<KIND>(job, p, omega, lambda, q, k);
        return lop_zeros(k, phi) > 0;
    };
    // round 0: p_min + i (p_max - p_min) / 63, the last one p_max itself
    const double h0 = (job.p_max - job.p_min) / (double)(LOP_WIDTH - 1);
    auto p0 = [&](int i) { return i == LOP_WIDTH - 1 ? job.p_max : job.p_min + (double)i * h0; };
    const uint64_t m0 = __ballot(hit(p0(lane)));
    double lo = NAN, hi = NAN;
    if (m0 != 0) {
        const int first = __ffsll((unsigned long long)m0) - 1, last = 63 - __clzll((long long)m0);
        lo = p0(first);
        if (first > 0) {
            double a = p0(first - 1);  // a has no zero, lo has
            for (int r = 1; r < LOP_ROUNDS; r++) {
                const double h = (lo - a) / (double)(LOP_WIDTH + 1);
                const uint64_t m = __ballot(hit(a + (double)(lane + 1) * h));
                const int f = m != 0 ? __ffsll((unsigned long long)m) - 1 : LOP_WIDTH;  // (none: the bracket's last piece)
                if (f < LOP_WIDTH) lo = a + (double)(f + 1) * h;
                if (f > 0) a = a + (double)f * h;
            }
        }
        hi = p0(last);
        if (last < LOP_WIDTH - 1) {
            double z = p0(last + 1);  // hi has a zero, z has none
            for (int r = 1; r < LOP_ROUNDS; r++) {
                const double h = (z - hi) / (double)(LOP_WIDTH + 1);
                const double base = hi;
                const uint64_t m = __ballot(hit(base + (double)(lane + 1) * h));
                const int l = m != 0 ? 63 - __clzll((long long)m) : -1;  // (none: the bracket's first piece)
                if (l < LOP_WIDTH - 1) z = base + (double)(l + 2) * h;
                if (l >= 0) hi = base + (double)(l + 1) * h;
            }
        }
    }
    if (lane == 0) {
        if (range) range[2 * b] = lo, range[2 * b + 1] = hi;
        if (status) status[b] = m0 != 0 ? CAF_LOP_FOUND : CAF_LOP_NO_CURVE;
    }
}

int check_desc(const caf_lop_desc* desc, const double* d_jobs, int64_t B, const char* who) {
    const std::string w(who);
    if (desc == nullptr) return set_error(w + ": NULL descriptor"), CAF_ERR_INVALID;
    if (desc->kind != CAF_LOP_HYPERBOLOID && desc->kind != CAF_LOP_SPHERE)
        return set_error(w + ": kind must be CAF_LOP_HYPERBOLOID or CAF_LOP_SPHERE"), CAF_ERR_INVALID;
    if (!(desc->omega > 0.0 && desc->omega < INFINITY && desc->lambda > 0.0 && desc->lambda < INFINITY))
        return set_error(w + ": the semi-axes omega and lambda must be finite and positive"), CAF_ERR_INVALID;
    if (B < 1 || B > ((int64_t)1 << 40)) return set_error(w + ": needs at least one job"), CAF_ERR_INVALID;
    if (d_jobs == nullptr) return set_error(w + ": NULL job table"), CAF_ERR_INVALID;
    return CAF_OK;
}

}  // namespace

}  // namespace caf

using namespace caf;

int32_t caf_lop_geometry(int32_t* samples_per_workgroup, int32_t* jobs_per_workgroup, int32_t* rounds, int32_t* width) {
    if (samples_per_workgroup) *samples_per_workgroup = LOP_S;
    if (jobs_per_workgroup) *jobs_per_workgroup = LOP_W;
    if (rounds) *rounds = LOP_ROUNDS;
    if (width) *width = LOP_WIDTH;
    return CAF_OK;
}

int32_t caf_lop_points(const caf_lop_desc* desc, const double* d_jobs, int64_t B, const double* d_range, int32_t* d_count,
                       double* d_phi, double* d_xyz, double* d_latlon, double* d_p_out, void* stream) {
    if (int rc = check_desc(desc, d_jobs, B, "caf_lop_points")) return rc;
    CAF_REQUIRE(desc->P >= 1, "caf_lop_points: needs at least one sample per job (P >= 1)");
    CAF_REQUIRE(desc->spacing == CAF_LOP_LIST || desc->spacing == CAF_LOP_LINSPACE || desc->spacing == CAF_LOP_CHEBYSHEV,
                "caf_lop_points: spacing must be CAF_LOP_LIST, CAF_LOP_LINSPACE or CAF_LOP_CHEBYSHEV");
    CAF_REQUIRE(desc->spacing != CAF_LOP_LIST || desc->d_p != nullptr, "caf_lop_points: CAF_LOP_LIST needs the parameter list d_p");
    CAF_REQUIRE(desc->spacing == CAF_LOP_LIST || d_range != nullptr, "caf_lop_points: CAF_LOP_LINSPACE and CAF_LOP_CHEBYSHEV need d_range");
    const int64_t blocks = (B * (int64_t)desc->P + LOP_S - 1) / LOP_S;
    CAF_REQUIRE(blocks <= 0x7fffffff, "caf_lop_points: too many samples for one launch");
    if (!d_count && !d_phi && !d_xyz && !d_latlon && !d_p_out) return CAF_OK;
    const LopOut out = {d_count, d_phi, d_xyz, d_latlon, d_p_out};
    hipStream_t st = (hipStream_t)stream;
    if (desc->kind == CAF_LOP_HYPERBOLOID)
        hipLaunchKernelGGL((k_lop_points<CAF_LOP_HYPERBOLOID>), dim3((unsigned)blocks), dim3(LOP_S), 0, st, d_jobs, B, desc->P, desc->spacing,
                           desc->d_p, d_range, desc->omega, desc->lambda, out);
    else
        hipLaunchKernelGGL((k_lop_points<CAF_LOP_SPHERE>), dim3((unsigned)blocks), dim3(LOP_S), 0, st, d_jobs, B, desc->P, desc->spacing,
                           desc->d_p, d_range, desc->omega, desc->lambda, out);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_lop_range(const caf_lop_desc* desc, const double* d_jobs, int64_t B, double* d_range, int32_t* d_status, void* stream) {
    if (int rc = check_desc(desc, d_jobs, B, "caf_lop_range")) return rc;
    const int64_t blocks = (B + LOP_W - 1) / LOP_W;
    CAF_REQUIRE(blocks <= 0x7fffffff, "caf_lop_range: too many jobs for one launch");
    if (!d_range && !d_status) return CAF_OK;
    hipStream_t st = (hipStream_t)stream;
    if (desc->kind == CAF_LOP_HYPERBOLOID)
        hipLaunchKernelGGL((k_lop_range<CAF_LOP_HYPERBOLOID>), dim3((unsigned)blocks), dim3(LOP_W * 64), 0, st, d_jobs, B, desc->omega,
                           desc->lambda, d_range, d_status);
    else
        hipLaunchKernelGGL((k_lop_range<CAF_LOP_SPHERE>), dim3((unsigned)blocks), dim3(LOP_W * 64), 0, st, d_jobs, B, desc->omega,
                           desc->lambda, d_range, d_status);
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}
