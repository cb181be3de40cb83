// Moving-platform scenarios (trajectoryRoutines.py: Trajectory.to / frm; cython_ext/PySampledLinearInterpolator: ConstAmpSigLerp,
// ConstAmpSigLerpBursty, ConstAmpSigLerpBurstyMulti).  With p(t) the position of a trajectory, c the speed of light:
//
//   caf_traj_tau         tau[r][n] solves c tau = |p_self(t[n]) - p_other_r(t[n] + sg tau)|, sg = +1 (to) or -1 (frm)
//   caf_lerp_propagate   out[n] = sum_e sum_b amp exp(j (lerp(phase_b)(u) - 2 pi fc (tau[n] + tJump) + phi)),
//                        u = t[n] - tau[n] - tJump - timevec[0], a term present iff 0 <= u < span
//   caf_scene_propagate  the same sum for every receiver r with t[n] = t0 + n dt and tau = rx_r.frm(tx_e, t[n]) solved per term
//
// One thread per (row, output sample), float64 throughout, nothing atomic and nothing shared between rows: a row is bitwise the
// same whatever the number of rows, and a sum of one emitter is that emitter's term (0 + x = x).
//
// Light time.  A stationary other side: |D| / c.  A constant-velocity other side: D = p_self(t) - p_other(t), a = c^2 - |v|^2,
// b = -2 D.v, disc = b^2 + 4 a |D|^2, tau = (sqrt(disc) +- b) / (2 a): sqrt(disc) ~ 2 c |D| dominates b by c / |v|, no
// cancellation.  Anything else: tau <- |p_self(t) - p_other(t + sg tau)| / c, 5 times from 0 (the contraction factor is |v| / c
// < 1e-4).  A knot table is searched by bisection; a step first tries the segment the previous step ended in.
//
// Active burst.  An emitter's windows are sorted and disjoint in emission time s = t - tau, so the last burst with u >= 0 is the
// only candidate: a bisection on u itself, the value the window test and the lerp then use.  In the fused form s increases
// with n (speeds are below c): the first and the last live thread of a workgroup bisect the emitter's whole list, and the other
// threads only the bursts between those two.
//
// Phase.  lerp: q = u / T, i = floor(q), fma(q - i, y[i + 1] - y[i], y[i]); in turns it is reduced mod 1, the carrier turns
// fc tau and fc tJump are exact products reduced before anything is rounded (mul_split), then one float64 sincospi.
#include <cmath>
#include <cstdint>
#include <vector>

#include "caf_internal.h"
#include "caf_phase.h"

#pragma clang fp contract(off)

namespace caf {

namespace {

constexpr int SC_THREADS = 256;  // threads and outputs per workgroup
constexpr int SC_MAX_EMITTERS = 64;
constexpr int SC_MAX_RECEIVERS = 64;
constexpr int SC_MAX_BURSTS = 4096;  // per emitter
constexpr int64_t SC_MAX_KNOTS = ((int64_t)1 << 31) - 1;
constexpr int SC_STEPS = 5;
constexpr double SC_C = 299792458.0;
constexpr double SC_MAX_BETA = 1e-4;
constexpr double SC_INV_2PI = 0.15915494309189535;

struct Traj {
    double x0[3];
    double v[3];
    const double* tp;  // this trajectory's knots
    const double* xp;
    int32_t knots;
    int32_t kind;
};

struct Burst {
    double start, span, T, amp, fc, phi, tjump;
    const double* phase;
    int32_t knots;
    int32_t pad;
};

// p(t); *seg: the segment of the last call on this trajectory (tried first), -1 for none
__device__ __forceinline__ void traj_at(const Traj& tr, double t, int32_t* seg, double p[3]) {
    if (tr.kind == CAF_TRAJ_STATIONARY) {
        p[0] = tr.x0[0], p[1] = tr.x0[1], p[2] = tr.x0[2];
        return;
    }
    if (tr.kind == CAF_TRAJ_CONSTANT_VELOCITY) {
#pragma unroll
        for (int i = 0; i < 3; i++) p[i] = fma(t, tr.v[i], tr.x0[i]);
        return;
    }
    const int32_t last = tr.knots - 1;
    if (!(t > tr.tp[0])) {  // (a NaN lands here)
        p[0] = tr.xp[0], p[1] = tr.xp[1], p[2] = tr.xp[2];
        return;
    }
    if (t >= tr.tp[last]) {
        p[0] = tr.xp[3 * (int64_t)last], p[1] = tr.xp[3 * (int64_t)last + 1], p[2] = tr.xp[3 * (int64_t)last + 2];
        return;
    }
    int32_t k = *seg;
    if (k < 0 || k >= last || !(tr.tp[k] <= t && t < tr.tp[k + 1])) {
        int32_t lo = 0, hi = last;  // tp[lo] <= t < tp[hi]
        while (hi - lo > 1) {
            const int32_t mid = lo + ((hi - lo) >> 1);
            if (tr.tp[mid] <= t) lo = mid;
            else hi = mid;
        }
        k = lo;
        *seg = k;
    }
    const double ta = tr.tp[k], tb = tr.tp[k + 1];
    const double w = (t - ta) / (tb - ta);
    const double* a = tr.xp + 3 * (int64_t)k;
#pragma unroll
    for (int i = 0; i < 3; i++) p[i] = fma(w, a[3 + i] - a[i], a[i]);
}

__device__ __forceinline__ double dist3(const double a[3], const double b[3], double d[3]) {
    d[0] = a[0] - b[0], d[1] = a[1] - b[1], d[2] = a[2] - b[2];
    return sqrt(fma(d[0], d[0], fma(d[1], d[1], d[2] * d[2])));
}

// sg = +1: the photon leaves self at t; -1: it arrives at self at t
__device__ __forceinline__ double light_time(const Traj& self, const Traj& other, double t, double sg, bool chase) {
    double ps[3], po[3], d[3];
    int32_t seg = -1;
    traj_at(self, t, &seg, ps);
    if (other.kind == CAF_TRAJ_STATIONARY) return dist3(ps, other.x0, d) / SC_C;
    if (other.kind == CAF_TRAJ_CONSTANT_VELOCITY && !chase && self.kind != CAF_TRAJ_INTERPOLATED) {
        seg = -1;
        traj_at(other, t, &seg, po);
        const double dd = dist3(ps, po, d);
        const double* v = other.v;
        const double a = SC_C * SC_C - fma(v[0], v[0], fma(v[1], v[1], v[2] * v[2]));
        const double b = -2.0 * fma(d[0], v[0], fma(d[1], v[1], d[2] * v[2]));
        const double disc = fma(b, b, 4.0 * a * (dd * dd));
        return fma(sg, b, sqrt(disc)) / (2.0 * a);
    }
    double tau = 0.0;
    seg = -1;
    for (int k = 0; k < SC_STEPS; k++) {
        traj_at(other, fma(sg, tau, t), &seg, po);
        tau = dist3(ps, po, d) / SC_C;
    }
    return tau;
}

__device__ __forceinline__ double burst_u(const Burst& b, double s) { return (s - b.tjump) - b.start; }

// the last burst of [lo, hi) with u >= 0, or -1
__device__ __forceinline__ int32_t find_burst(const Burst* __restrict__ bursts, int32_t lo, int32_t hi, double s) {
    if (lo >= hi || !(burst_u(bursts[lo], s) >= 0.0)) return -1;
    while (hi - lo > 1) {  // u(lo) >= 0; u(hi) < 0 or hi is the end
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (burst_u(bursts[mid], s) >= 0.0) lo = mid;
        else hi = mid;
    }
    return lo;
}

// adds the term of burst b at emission time s = t - tau (nothing outside its window)
__device__ __forceinline__ void add_term(const Burst& b, double s, double tau, double* re, double* im) {
    const double u = burst_u(b, s);
    if (!(u >= 0.0 && u < b.span)) return;
    const double q = u / b.T;
    int32_t i = (int32_t)fmin(floor(q), (double)(b.knots - 2));
    const double fr = q - (double)i;
    const double y0 = b.phase[i], y1 = b.phase[i + 1];
    const double lp = fma(fr, y1 - y0, y0);
    double whole, r1, r2;
    mul_split(b.fc, tau, &whole, &r1);
    mul_split(b.fc, b.tjump, &whole, &r2);
    const double turns = ((frac_turn(lp * SC_INV_2PI) - r1) - r2) + frac_turn(b.phi * SC_INV_2PI);
    double sn, cs;
    sincospi(2.0 * turns, &sn, &cs);
    *re += b.amp * cs;
    *im += b.amp * sn;
}

template <bool C128>
__device__ __forceinline__ void store_out(void* out, int64_t at, double re, double im) {
    if (C128) ((double2*)out)[at] = make_double2(re, im);
    else ((float2*)out)[at] = make_float2((float)re, (float)im);
}

__global__ __launch_bounds__(SC_THREADS) void k_traj_tau(const Traj* __restrict__ self, const Traj* __restrict__ others,
                                                        const double* __restrict__ t, int64_t n, int32_t tiles, double sg, int32_t chase,
                                                        double* __restrict__ tau) {
    const int32_t row = (int32_t)blockIdx.x / tiles;
    const int64_t at = (int64_t)((int32_t)blockIdx.x - row * tiles) * SC_THREADS + threadIdx.x;
    if (at >= n) return;
    tau[(int64_t)row * n + at] = light_time(self[0], others[row], t[at], sg, chase != 0);
}

template <bool C128>
__global__ __launch_bounds__(SC_THREADS) void k_lerp_propagate(const Burst* __restrict__ bursts, const int32_t* __restrict__ burst_off,
                                                              int32_t emitters, const double* __restrict__ t,
                                                              const double* __restrict__ tau, int64_t n, int64_t start_idx,
                                                              void* __restrict__ out) {
    const int64_t at = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    if (at >= n) return;
    double re = 0.0, im = 0.0;
    if (at >= start_idx) {
        const double ta = tau[at];
        const double s = t[at] - ta;
        for (int32_t e = 0; e < emitters; e++) {
            const int32_t b = find_burst(bursts, burst_off[e], burst_off[e + 1], s);
            if (b >= 0) add_term(bursts[b], s, ta, &re, &im);
        }
    }
    store_out<C128>(out, at, re, im);
}

template <bool C128>
__global__ __launch_bounds__(SC_THREADS) void k_scene(const Traj* __restrict__ tx, const Traj* __restrict__ rx,
                                                     const Burst* __restrict__ bursts, const int32_t* __restrict__ burst_off,
                                                     int32_t emitters, double t0, double dt, int64_t n, int32_t tiles,
                                                     void* __restrict__ out) {
    __shared__ int32_t s_edge[SC_MAX_EMITTERS][2];
    const int32_t row = (int32_t)blockIdx.x / tiles;
    const int64_t base = (int64_t)((int32_t)blockIdx.x - row * tiles) * SC_THREADS;
    const int64_t at = base + threadIdx.x;
    const bool live = at < n;
    const int32_t last_live = (int32_t)((n - base < SC_THREADS ? n - base : (int64_t)SC_THREADS) - 1);
    const int64_t nn = live ? at : n - 1;  // a thread past the row repeats the last sample and stores nothing
    const double t = t0 + (double)nn * dt;
    const Traj& me = rx[row];
    double re = 0.0, im = 0.0;
    for (int32_t e = 0; e < emitters; e++) {  // (uniform: every thread reaches the barrier)
        const double ta = light_time(me, tx[e], t, -1.0, false);
        const double s = t - ta;
        const int32_t b0 = burst_off[e], b1 = burst_off[e + 1];
        int32_t b = -1;
        const bool edge = threadIdx.x == 0 || (int32_t)threadIdx.x == last_live;
        if (edge) {
            b = find_burst(bursts, b0, b1, s);
            if (threadIdx.x == 0) s_edge[e][0] = b;
            if ((int32_t)threadIdx.x == last_live) s_edge[e][1] = b;
        }
        __syncthreads();
        if (!edge) {
            const int32_t first = s_edge[e][0], last = s_edge[e][1];
            b = find_burst(bursts, first < 0 ? b0 : first, last + 1, s);  // (last < 0: an empty range)
        }
        if (b >= 0) add_term(bursts[b], s, ta, &re, &im);
    }
    if (live) store_out<C128>(out, (int64_t)row * n + at, re, im);
}

// checks a trajectory table and lays it out for the kernels
int build_trajs(const caf_traj_table* tb, int32_t max_count, const char* what, std::vector<Traj>* out) {
    CAF_REQUIRE(tb && tb->count >= 1 && tb->count <= max_count, std::string(what) + ": the number of trajectories is out of range");
    CAF_REQUIRE(tb->h_kind && tb->h_x0v && tb->h_knot_off, std::string(what) + ": NULL table");
    CAF_REQUIRE(tb->h_knot_off[0] == 0, std::string(what) + ": the knot offsets start at 0");
    out->resize(tb->count);
    for (int32_t i = 0; i < tb->count; i++) {
        Traj& tr = (*out)[i];
        tr = Traj{};
        tr.kind = tb->h_kind[i];
        CAF_REQUIRE(tr.kind >= CAF_TRAJ_STATIONARY && tr.kind <= CAF_TRAJ_INTERPOLATED, std::string(what) + ": unknown trajectory kind");
        const int64_t k0 = tb->h_knot_off[i], k1 = tb->h_knot_off[i + 1];
        CAF_REQUIRE(k1 >= k0 && k1 <= SC_MAX_KNOTS, std::string(what) + ": the knot offsets must ascend and stay below 2^31");
        if (tr.kind == CAF_TRAJ_INTERPOLATED) {
            CAF_REQUIRE(k1 - k0 >= 2, std::string(what) + ": an interpolated trajectory needs at least 2 knots");
            CAF_REQUIRE(tb->d_tp && tb->d_xp, std::string(what) + ": NULL knot arrays");
            tr.tp = tb->d_tp + k0;
            tr.xp = tb->d_xp + 3 * k0;
            tr.knots = (int32_t)(k1 - k0);
        } else {
            CAF_REQUIRE(k1 == k0, std::string(what) + ": only an interpolated trajectory has knots");
            double v2 = 0.0;
            for (int j = 0; j < 3; j++) {
                tr.x0[j] = tb->h_x0v[6 * i + j];
                tr.v[j] = tr.kind == CAF_TRAJ_CONSTANT_VELOCITY ? tb->h_x0v[6 * i + 3 + j] : 0.0;
                CAF_REQUIRE(std::isfinite(tr.x0[j]) && std::isfinite(tr.v[j]), std::string(what) + ": x0 and v must be finite");
                v2 += tr.v[j] * tr.v[j];
            }
            CAF_REQUIRE(std::sqrt(v2) < SC_MAX_BETA * SC_C, std::string(what) + ": speeds of 1e-4 c or more are not supported");
        }
    }
    return CAF_OK;
}

int build_bursts(const caf_burst_table* tb, std::vector<Burst>* out) {
    CAF_REQUIRE(tb && tb->count >= 1 && tb->count <= SC_MAX_EMITTERS, "caf_scene: the number of emitters is out of range");
    CAF_REQUIRE(tb->h_burst_off && tb->h_burst && tb->h_phase_off && tb->d_phase, "caf_scene: NULL burst table");
    CAF_REQUIRE(tb->h_burst_off[0] == 0 && tb->h_phase_off[0] == 0, "caf_scene: the burst and phase offsets start at 0");
    for (int32_t e = 0; e < tb->count; e++) {
        const int32_t nb = tb->h_burst_off[e + 1] - tb->h_burst_off[e];
        CAF_REQUIRE(nb >= 1 && nb <= SC_MAX_BURSTS, "caf_scene: the number of bursts of an emitter is out of range");
    }
    out->resize(tb->h_burst_off[tb->count]);
    for (int32_t e = 0; e < tb->count; e++) {
        for (int32_t i = tb->h_burst_off[e]; i < tb->h_burst_off[e + 1]; i++) {
            Burst& b = (*out)[i];
            const double* h = tb->h_burst + 7 * (int64_t)i;
            b = Burst{h[0], h[1], h[2], h[3], h[4], h[5], h[6], nullptr, 0, 0};
            for (int j = 0; j < 7; j++) CAF_REQUIRE(std::isfinite(h[j]), "caf_scene: the burst parameters must be finite");
            const int64_t p0 = tb->h_phase_off[i], p1 = tb->h_phase_off[i + 1];
            CAF_REQUIRE(p1 - p0 >= 2 && p1 - p0 <= SC_MAX_KNOTS, "caf_scene: a burst needs at least 2 phase knots (and fewer than 2^31)");
            b.phase = tb->d_phase + p0;
            b.knots = (int32_t)(p1 - p0);
            CAF_REQUIRE(b.T > 0.0 && b.span > 0.0, "caf_scene: T and timevec[-1] - timevec[0] must be positive");
            CAF_REQUIRE(b.span <= ((double)(b.knots - 1) + 1e-3) * b.T, "caf_scene: the window is longer than the phase table");
            if (i > tb->h_burst_off[e]) {
                const Burst& a = (*out)[i - 1];
                CAF_REQUIRE((a.start + a.tjump) + a.span <= b.start + b.tjump,
                            "caf_scene: the bursts of an emitter must be in ascending order and disjoint in emission time");
            }
        }
    }
    return CAF_OK;
}

// a host table on its way to the device; the caller waits once (uploads_done) before its host tables go away
template <typename T>
int upload(Scratch& sc, const T* h, int64_t count, hipStream_t st, T** d) {
    if (const int rc = sc.get(d, count)) return rc;
    CAF_HIP_TRY(hipMemcpyAsync(*d, h, (size_t)count * sizeof(T), hipMemcpyHostToDevice, st));
    return CAF_OK;
}

int uploads_done(hipStream_t st) {
    CAF_HIP_TRY(hipStreamSynchronize(st));
    return CAF_OK;
}

inline bool tiles_ok(int64_t n, int32_t rows, int32_t* tiles) {
    const int64_t t = (n + SC_THREADS - 1) / SC_THREADS;
    *tiles = (int32_t)t;
    return t * rows <= 0x7fffffff;
}

}  // namespace

}  // namespace caf

using namespace caf;

int32_t caf_scene_geometry(int32_t* max_emitters, int32_t* max_receivers, int32_t* max_bursts, int64_t* max_knots,
                           int32_t* threads_per_workgroup, int32_t* outputs_per_workgroup) {
    if (max_emitters) *max_emitters = SC_MAX_EMITTERS;
    if (max_receivers) *max_receivers = SC_MAX_RECEIVERS;
    if (max_bursts) *max_bursts = SC_MAX_BURSTS;
    if (max_knots) *max_knots = SC_MAX_KNOTS;
    if (threads_per_workgroup) *threads_per_workgroup = SC_THREADS;
    if (outputs_per_workgroup) *outputs_per_workgroup = SC_THREADS;
    return CAF_OK;
}

int32_t caf_traj_tau(const caf_traj_table* self, const caf_traj_table* others, const double* d_t, int64_t n, int32_t direction,
                     int32_t method, double* d_tau, void* stream) {
    std::vector<Traj> me, them;
    if (const int rc = build_trajs(self, 1, "caf_traj_tau (self)", &me)) return rc;
    if (const int rc = build_trajs(others, SC_MAX_RECEIVERS, "caf_traj_tau (others)", &them)) return rc;
    CAF_REQUIRE(direction == 0 || direction == 1, "caf_traj_tau: direction is 0 (to) or 1 (frm)");
    CAF_REQUIRE(method == 0 || method == 1, "caf_traj_tau: method is 0 (closed form where there is one) or 1 (iteration)");
    int32_t tiles = 0;
    CAF_REQUIRE(n >= 1 && tiles_ok(n, others->count, &tiles), "caf_traj_tau: n must be positive and fit one launch");
    CAF_REQUIRE(d_t && d_tau, "caf_traj_tau: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    Traj *d_me = nullptr, *d_them = nullptr;
    if (const int rc = upload(sc, me.data(), 1, st, &d_me)) return rc;
    if (const int rc = upload(sc, them.data(), (int64_t)them.size(), st, &d_them)) return rc;
    if (const int rc = uploads_done(st)) return rc;
    hipLaunchKernelGGL(k_traj_tau, dim3((unsigned)(tiles * others->count)), dim3(SC_THREADS), 0, st, (const Traj*)d_me, (const Traj*)d_them,
                       d_t, n, tiles, direction == 0 ? 1.0 : -1.0, method, d_tau);
    CAF_HIP_TRY(hipGetLastError());
    return sc.finish();
}

int32_t caf_lerp_propagate(const caf_burst_table* bursts, const double* d_t, const double* d_tau, int64_t n, int64_t start_idx,
                           int32_t c128, void* d_out, void* stream) {
    std::vector<Burst> tb;
    if (const int rc = build_bursts(bursts, &tb)) return rc;
    int32_t tiles = 0;
    CAF_REQUIRE(n >= 1 && tiles_ok(n, 1, &tiles), "caf_lerp_propagate: n must be positive and fit one launch");
    CAF_REQUIRE(c128 == 0 || c128 == 1, "caf_lerp_propagate: c128 must be 0 or 1");
    CAF_REQUIRE(d_t && d_tau && d_out, "caf_lerp_propagate: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    Burst* d_b = nullptr;
    int32_t* d_off = nullptr;
    if (const int rc = upload(sc, tb.data(), (int64_t)tb.size(), st, &d_b)) return rc;
    if (const int rc = upload(sc, bursts->h_burst_off, (int64_t)bursts->count + 1, st, &d_off)) return rc;
    if (const int rc = uploads_done(st)) return rc;
    if (c128)
        hipLaunchKernelGGL(k_lerp_propagate<true>, dim3((unsigned)tiles), dim3(SC_THREADS), 0, st, (const Burst*)d_b, (const int32_t*)d_off,
                           bursts->count, d_t, d_tau, n, start_idx, d_out);
    else
        hipLaunchKernelGGL(k_lerp_propagate<false>, dim3((unsigned)tiles), dim3(SC_THREADS), 0, st, (const Burst*)d_b, (const int32_t*)d_off,
                           bursts->count, d_t, d_tau, n, start_idx, d_out);
    CAF_HIP_TRY(hipGetLastError());
    return sc.finish();
}

int32_t caf_scene_propagate(const caf_traj_table* emitters, const caf_traj_table* receivers, const caf_burst_table* bursts, double t0,
                            double dt, int64_t n, int32_t c128, void* d_out, void* stream) {
    std::vector<Traj> tx, rx;
    std::vector<Burst> tb;
    if (const int rc = build_trajs(emitters, SC_MAX_EMITTERS, "caf_scene_propagate (emitters)", &tx)) return rc;
    if (const int rc = build_trajs(receivers, SC_MAX_RECEIVERS, "caf_scene_propagate (receivers)", &rx)) return rc;
    if (const int rc = build_bursts(bursts, &tb)) return rc;
    CAF_REQUIRE(bursts->count == emitters->count, "caf_scene_propagate: one burst list per emitter");
    CAF_REQUIRE(std::isfinite(t0) && std::isfinite(dt) && dt > 0.0, "caf_scene_propagate: t0 must be finite, dt positive and finite");
    int32_t tiles = 0;
    CAF_REQUIRE(n >= 1 && tiles_ok(n, receivers->count, &tiles), "caf_scene_propagate: n must be positive and fit one launch");
    CAF_REQUIRE(c128 == 0 || c128 == 1, "caf_scene_propagate: c128 must be 0 or 1");
    CAF_REQUIRE(d_out, "caf_scene_propagate: NULL output");
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    Traj *d_tx = nullptr, *d_rx = nullptr;
    Burst* d_b = nullptr;
    int32_t* d_off = nullptr;
    if (const int rc = upload(sc, tx.data(), (int64_t)tx.size(), st, &d_tx)) return rc;
    if (const int rc = upload(sc, rx.data(), (int64_t)rx.size(), st, &d_rx)) return rc;
    if (const int rc = upload(sc, tb.data(), (int64_t)tb.size(), st, &d_b)) return rc;
    if (const int rc = upload(sc, bursts->h_burst_off, (int64_t)bursts->count + 1, st, &d_off)) return rc;
    if (const int rc = uploads_done(st)) return rc;
    const unsigned grid = (unsigned)(tiles * receivers->count);
    if (c128)
        hipLaunchKernelGGL(k_scene<true>, dim3(grid), dim3(SC_THREADS), 0, st, (const Traj*)d_tx, (const Traj*)d_rx, (const Burst*)d_b,
                           (const int32_t*)d_off, bursts->count, t0, dt, n, tiles, d_out);
    else
        hipLaunchKernelGGL(k_scene<false>, dim3(grid), dim3(SC_THREADS), 0, st, (const Traj*)d_tx, (const Traj*)d_rx, (const Burst*)d_b,
                           (const int32_t*)d_off, bursts->count, t0, dt, n, tiles, d_out);
    CAF_HIP_TRY(hipGetLastError());
    return sc.finish();
}
