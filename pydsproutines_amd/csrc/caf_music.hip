// Subspace spectra (musicRoutines.py: MUSIC, CAPON, ESPRIT, musicAlg; xcorrRoutines.py: musicXcorr), batched.  Everything is
// float64: the noise subspace of a covariance lives 2^-53-relative under its largest eigenvalue and float32 destroys it.
//
//   k_music_cov          Rx[i, j] = scale sum_segments sum_c x[c jump + i] conj(x[c jump + j]), a segment being (offset, element
//                        stride, length) into one buffer of complex64 or complex128 and giving (length - rows) / jump + 1 snapshots
//                        (the reshape form of the reference is jump = rows).  One workgroup per 32 x 32 tile of the upper triangle and
//                        batch entry, a thread owns 2 x 2 outputs; 32 snapshots of the two 32-sample windows are staged in LDS at a
//                        time.  Direct sums: the four real products of a term go to four accumulators, each one fused multiply-add
//                        chain over the terms in order (segment by segment, snapshot by snapshot), so a term passes through at most
//                        C roundings, C the number of terms; then one addition and the scale.  The lower triangle is the mirror.
//   k_music_cov_post     forward-backward averaging 0.5 (Rx + J Rx^T J) and averaging of every diagonal (Toeplitz), one workgroup
//                        per matrix, when either is asked for.
//   k_music_eig          Hermitian eigendecomposition by one-sided (Hestenes) Jacobi on the columns of G = Rx with an accumulated
//                        V: one workgroup of 16 waves per matrix, round-robin ordering (rows / 2 disjoint pairs per step, a bye when
//                        rows is odd), one wave per pair: the three column dots through wave_sum, then the rotation of the two
//                        columns of G and of V.  G and V are column-major in pooled scratch.  A pair is rotated when
//                        |g_p^H g_q|^2 > rows 2^-106 |g_p|^2 |g_q|^2; a sweep without a rotation ends the solve.  The sweep loop is
//                        bounded (EIG_SWEEPS); running out writes status -1, never spins.  s = the column norms of G, descending
//                        (ties by column index); u = the columns of V in that order, normalised; vh = u^H.
//   k_music_spectrum     g_k(f) = |sum_m exp(-j 2 pi f m) u[m, k]|^2 for every k at once: the steering rows of a block of
//                        frequencies are formed in float64 from the exact product f m (rounded product plus its fma residual)
//                        reduced to a fraction of a turn before sincospi, staged in LDS and reused over all k; then per frequency
//                        and p: denom = sum_{k >= p} g_k, num = sum_{k < p} g_k / s_k (mode 2, Capon: denom = sum_k g_k / s_k).
//   k_music_xcorr_front  out[b, n] = sum_t taps[t] rx[s_b + n - t] conj(cutout[n - t]) over n - t >= 0 (lfilter(ftap, 1, product)),
//                        direct form, for every shift s_b.
//
// Nothing is atomic, every sum has one order that depends on the problem's own shape alone, and batch entries never meet: entry b
// is bitwise what the same problem gives alone.  Every loop bound is an argument the host has validated.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "caf_internal.h"
#include "caf_wave.h"

namespace caf {

namespace {

constexpr int MUSIC_MIN_ROWS = 2;
constexpr int MUSIC_MAX_ROWS = 256;   // a column is at most 4 elements per lane of a wave
constexpr int MUSIC_MAX_BATCH = 65535;  // (the batch is a grid's y extent)
constexpr int COV_TILE = 32;          // outputs per side of a tile
constexpr int COV_CH = 32;            // snapshots staged at a time
constexpr int EIG_THREADS = 1024;
constexpr int EIG_WAVES = EIG_THREADS / 64;
constexpr int EIG_PER_LANE = MUSIC_MAX_ROWS / 64;
constexpr int EIG_SWEEPS = 60;
constexpr int SP_THREADS = 256;
constexpr int SP_FPT = 8;             // frequencies per thread
constexpr int SP_SLOTS = SP_THREADS * SP_FPT;  // LDS entries of the steering rows and of g

struct CovSeg {
    int64_t offset, stride, ncols;
};

__device__ __forceinline__ double2 load_x(const void* x, int c128, int64_t at) {
    if (c128) return ((const double2*)x)[at];
    const float2 v = ((const float2*)x)[at];
    return make_double2((double)v.x, (double)v.y);
}

// tile (ti, tj), ti <= tj, of the upper triangle from its running number
__device__ __forceinline__ void tile_of(int t, int nt, int& ti, int& tj) {
    ti = 0;
    while (t >= nt - ti) {
        t -= nt - ti;
        ti++;
    }
    tj = ti + t;
}

__global__ __launch_bounds__(256) void k_music_cov(const void* __restrict__ x, int c128, const CovSeg* __restrict__ segs, int nseg,
                                                   const double* __restrict__ scales, int rows, int64_t jump, int nt,
                                                   double2* __restrict__ out) {
    __shared__ double2 s_a[COV_CH][COV_TILE], s_b[COV_CH][COV_TILE];
    const int b = blockIdx.y, tid = threadIdx.x;
    int ti, tj;
    tile_of(blockIdx.x, nt, ti, tj);
    const int i0 = ti * COV_TILE, j0 = tj * COV_TILE;
    const int li = tid & 15, lj = tid >> 4;
    // [a][b][part]: a = which of the thread's two rows, b = which of its two columns; parts rr, ii, ir, ri
    double acc[2][2][4] = {};
    for (int sg = 0; sg < nseg; sg++) {
        const CovSeg s = segs[(int64_t)b * nseg + sg];
        for (int64_t c0 = 0; c0 < s.ncols; c0 += COV_CH) {
            __syncthreads();
            for (int e = tid; e < COV_CH * COV_TILE; e += 256) {
                const int cc = e / COV_TILE, k = e - cc * COV_TILE;
                const int64_t c = c0 + cc;
                double2 va = make_double2(0.0, 0.0), vb = va;
                if (c < s.ncols) {
                    if (i0 + k < rows) va = load_x(x, c128, s.offset + (c * jump + i0 + k) * s.stride);
                    if (j0 + k < rows) vb = load_x(x, c128, s.offset + (c * jump + j0 + k) * s.stride);
                }
                s_a[cc][k] = va;
                s_b[cc][k] = vb;
            }
            __syncthreads();
#pragma unroll 4
            for (int cc = 0; cc < COV_CH; cc++) {
                const double2 a[2] = {s_a[cc][li], s_a[cc][li + 16]};
                const double2 bb[2] = {s_b[cc][lj], s_b[cc][lj + 16]};
#pragma unroll
                for (int p = 0; p < 2; p++)
#pragma unroll
                    for (int q = 0; q < 2; q++) {
                        acc[p][q][0] = fma(a[p].x, bb[q].x, acc[p][q][0]);
                        acc[p][q][1] = fma(a[p].y, bb[q].y, acc[p][q][1]);
                        acc[p][q][2] = fma(a[p].y, bb[q].x, acc[p][q][2]);
                        acc[p][q][3] = fma(a[p].x, bb[q].y, acc[p][q][3]);
                    }
            }
        }
    }
    const double scale = scales[b];
    double2* o = out + (int64_t)b * rows * rows;
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int i = i0 + li + 16 * p, j = j0 + lj + 16 * q;
            if (i >= rows || j >= rows || i > j) continue;
            const double re = (acc[p][q][0] + acc[p][q][1]) * scale, im = (acc[p][q][2] - acc[p][q][3]) * scale;
            o[(int64_t)i * rows + j] = make_double2(re, im);
            if (i != j) o[(int64_t)j * rows + i] = make_double2(re, -im);
        }
}

__global__ __launch_bounds__(256) void k_music_cov_post(const double2* __restrict__ raw_all, int rows, int fwd_bwd, int toeplitz,
                                                        double2* __restrict__ out_all) {
    __shared__ double2 s_diag[2 * MUSIC_MAX_ROWS];
    const int n = rows, tid = threadIdx.x;
    const double2* raw = raw_all + (int64_t)blockIdx.x * n * n;
    double2* out = out_all + (int64_t)blockIdx.x * n * n;
    for (int e = tid; e < n * n; e += 256) {
        const int i = e / n, j = e - i * n;
        double2 v = raw[e];
        if (fwd_bwd) {  // (J Rx^T J)[i, j] = Rx[n - 1 - j, n - 1 - i]
            const double2 w = raw[(n - 1 - j) * n + (n - 1 - i)];
            v = make_double2(0.5 * (v.x + w.x), 0.5 * (v.y + w.y));
        }
        out[e] = v;
    }
    if (!toeplitz) return;
    __syncthreads();
    for (int d = tid; d < 2 * n - 1; d += 256) {  // diagonal k = d - (n - 1): the mean of out[i, i + k]
        const int k = d - (n - 1), i_lo = k < 0 ? -k : 0, cnt = n - (k < 0 ? -k : k);
        double sr = 0.0, si = 0.0;
        for (int t = 0; t < cnt; t++) {
            const double2 v = out[(i_lo + t) * n + (i_lo + t + k)];
            sr += v.x;
            si += v.y;
        }
        s_diag[d] = make_double2(sr / cnt, si / cnt);
    }
    __syncthreads();
    for (int e = tid; e < n * n; e += 256) {
        const int i = e / n, j = e - i * n;
        out[e] = s_diag[j - i + n - 1];
    }
}

__global__ __launch_bounds__(EIG_THREADS) void k_music_eig(const double2* __restrict__ rx_all, int n, double2* __restrict__ g_all,
                                                           double2* __restrict__ v_all, double* __restrict__ s_all,
                                                           double2* __restrict__ u_all, double2* __restrict__ vh_all,
                                                           int32_t* __restrict__ status) {
    __shared__ double s_norm2[MUSIC_MAX_ROWS], s_vinv[MUSIC_MAX_ROWS];
    __shared__ int s_col_of[MUSIC_MAX_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * n * n;
    const double2* rx = rx_all + base;
    double2* G = g_all + base;
    double2* V = v_all + base;
    for (int e = tid; e < n * n; e += EIG_THREADS) {  // column-major: column k at k n
        const int k = e / n, m = e - k * n;
        G[e] = rx[m * n + k];
        V[e] = make_double2(m == k ? 1.0 : 0.0, 0.0);
    }
    __syncthreads();

    const int mm = n + (n & 1);                  // players of the round robin: a phantom when n is odd
    const double tol2 = (double)n * 0x1p-106;    // (sqrt(n) 2^-53)^2
    int sweeps = -1;
    for (int sweep = 0; sweep < EIG_SWEEPS; sweep++) {
        int rotated = 0;
        for (int r = 0; r < mm - 1; r++) {
            for (int pi = wave; pi < mm / 2; pi += EIG_WAVES) {
                int p, q;
                if (pi == 0) {
                    p = mm - 1;
                    q = r;
                } else {
                    p = (r + pi) % (mm - 1);
                    q = (r - pi + mm - 1) % (mm - 1);
                }
                if (p > q) {
                    const int t = p;
                    p = q;
                    q = t;
                }
                if (q >= n) continue;  // the bye (the same for the whole wave)
                double2* gp = G + p * n;
                double2* gq = G + q * n;
                double2 xp[EIG_PER_LANE], xq[EIG_PER_LANE];
                double a = 0.0, bq = 0.0, cr = 0.0, ci = 0.0;
#pragma unroll
                for (int j = 0; j < EIG_PER_LANE; j++) {
                    const int m = lane + 64 * j;
                    xp[j] = xq[j] = make_double2(0.0, 0.0);
                    if (m < n) {
                        xp[j] = gp[m];
                        xq[j] = gq[m];
                    }
                    a = fma(xp[j].x, xp[j].x, fma(xp[j].y, xp[j].y, a));
                    bq = fma(xq[j].x, xq[j].x, fma(xq[j].y, xq[j].y, bq));
                    cr = fma(xp[j].x, xq[j].x, fma(xp[j].y, xq[j].y, cr));  // c = g_p^H g_q
                    ci = fma(xp[j].x, xq[j].y, fma(-xp[j].y, xq[j].x, ci));
                }
                a = wave_sum(a);
                bq = wave_sum(bq);
                cr = wave_sum(cr);
                ci = wave_sum(ci);
                const double c2 = cr * cr + ci * ci;
                if (!(c2 > tol2 * a * bq)) continue;  // orthogonal already (or a zero column, or not a number): wave-uniform
                rotated = 1;
                const double cabs = sqrt(c2);
                const double er = cr / cabs, ei = ci / cabs;
                const double zeta = (bq - a) / (2.0 * cabs);
                const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                // h = g_q conj(e) makes g_p^H h = |c| real; then a real rotation of (g_p, h)
#pragma unroll
                for (int j = 0; j < EIG_PER_LANE; j++) {
                    const int m = lane + 64 * j;
                    if (m < n) {
                        const double hx = xq[j].x * er + xq[j].y * ei, hy = xq[j].y * er - xq[j].x * ei;
                        gp[m] = make_double2(cs * xp[j].x - sn * hx, cs * xp[j].y - sn * hy);
                        gq[m] = make_double2(sn * xp[j].x + cs * hx, sn * xp[j].y + cs * hy);
                    }
                }
                // (V's columns are read only when the pair is rotated: asking for them together with G's was measured and did not pay)
                double2* vp = V + p * n;
                double2* vq = V + q * n;
#pragma unroll
                for (int j = 0; j < EIG_PER_LANE; j++) {
                    const int m = lane + 64 * j;
                    if (m < n) {
                        const double2 yp = vp[m], yq = vq[m];
                        const double hx = yq.x * er + yq.y * ei, hy = yq.y * er - yq.x * ei;
                        vp[m] = make_double2(cs * yp.x - sn * hx, cs * yp.y - sn * hy);
                        vq[m] = make_double2(sn * yp.x + cs * hx, sn * yp.y + cs * hy);
                    }
                }
            }
            __syncthreads();  // the pairs of a step are disjoint; the next step reads what this one wrote
        }
        // workgroup-uniform before anything depends on it
        if (!__syncthreads_or(rotated)) {
            sweeps = sweep + 1;
            break;
        }
    }
    if (tid == 0) status[blockIdx.x] = sweeps;  // -1: the sweep limit ran out

    // eigenvalues = the column norms of G; the norms of V's columns for the final normalisation
    for (int k = wave; k < n; k += EIG_WAVES) {
        double a = 0.0, v2 = 0.0;
#pragma unroll
        for (int j = 0; j < EIG_PER_LANE; j++) {
            const int m = lane + 64 * j;
            if (m < n) {
                const double2 g = G[k * n + m], v = V[k * n + m];
                a = fma(g.x, g.x, fma(g.y, g.y, a));
                v2 = fma(v.x, v.x, fma(v.y, v.y, v2));
            }
        }
        a = wave_sum(a);
        v2 = wave_sum(v2);
        if (lane == 0) {
            s_norm2[k] = a;
            s_vinv[k] = 1.0 / sqrt(v2);
        }
    }
    __syncthreads();
    if (tid < n) {  // descending, equal values by column index: a place of its own for every column
        // (what is not a number, from an input that held none, goes after every number: still one place per column)
        const double mine = s_norm2[tid];
        const bool mnan = mine != mine;
        int rank = 0;
        for (int j = 0; j < n; j++) {
            const double o = s_norm2[j];
            const bool onan = o != o;
            const bool ahead = mnan ? (!onan || j < tid) : (!onan && first_max(mine, tid, o, j));
            rank += ahead ? 1 : 0;
        }
        s_col_of[rank] = tid;
        s_all[(int64_t)blockIdx.x * n + rank] = sqrt(mine);
    }
    __syncthreads();
    for (int e = tid; e < n * n; e += EIG_THREADS) {
        const int m = e / n, kr = e - m * n;
        const int k = s_col_of[kr];
        const double2 v = V[k * n + m];
        const double w = s_vinv[k];
        const double2 uv = make_double2(v.x * w, v.y * w);
        u_all[base + e] = uv;
        if (vh_all) vh_all[base + (int64_t)kr * n + m] = make_double2(uv.x, -uv.y);
    }
}

__global__ __launch_bounds__(SP_THREADS) void k_music_spectrum(const double2* __restrict__ u_all, const double* __restrict__ s_all,
                                                               const double* __restrict__ freqs, int nfreq,
                                                               const int32_t* __restrict__ plist, int np, int mode, int n, int kt,
                                                               double* __restrict__ f_out, double* __restrict__ denom_out,
                                                               double* __restrict__ num_out) {
    __shared__ double2 s_e[SP_SLOTS];  // [slot][m]
    __shared__ double s_g[SP_SLOTS];   // [slot][k]
    __shared__ double s_s[MUSIC_MAX_ROWS];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int slots = (SP_THREADS / kt) * SP_FPT;  // frequencies of this workgroup; slots n <= SP_SLOTS because kt >= n
    const int f0 = blockIdx.x * slots;
    const double2* u = u_all + (int64_t)b * n * n;
    for (int e = tid; e < slots * n; e += SP_THREADS) {
        const int slot = e / n, m = e - slot * n;
        double2 v = make_double2(0.0, 0.0);
        if (f0 + slot < nfreq) {
            const double f = freqs[f0 + slot], dm = (double)m;
            const double t = f * dm, err = fma(f, dm, -t);  // f m = t + err exactly
            const double turn = (t - rint(t)) + err;
            double sn, cs;
            sincospi(2.0 * turn, &sn, &cs);
            v = make_double2(cs, -sn);
        }
        s_e[e] = v;
    }
    if (tid < n) s_s[tid] = s_all[(int64_t)b * n + tid];
    __syncthreads();
    const int kk = tid % kt, fsub = tid / kt;
    if (kk < n) {
        double ar[SP_FPT] = {}, ai[SP_FPT] = {};
        const double2* e0 = s_e + fsub * SP_FPT * n;
        for (int m = 0; m < n; m++) {
            const double2 uv = u[m * n + kk];
#pragma unroll
            for (int j = 0; j < SP_FPT; j++) {
                const double2 ev = e0[j * n + m];
                ar[j] = fma(ev.x, uv.x, fma(-ev.y, uv.y, ar[j]));
                ai[j] = fma(ev.x, uv.y, fma(ev.y, uv.x, ai[j]));
            }
        }
#pragma unroll
        for (int j = 0; j < SP_FPT; j++) s_g[(fsub * SP_FPT + j) * n + kk] = ar[j] * ar[j] + ai[j] * ai[j];
    }
    __syncthreads();
    for (int e = tid; e < slots * np; e += SP_THREADS) {
        const int slot = e / np, pi = e - slot * np;
        if (f0 + slot >= nfreq) continue;
        const double* g = s_g + slot * n;
        double denom = 0.0, num = 0.0;
        if (mode == 2) {
            for (int k = n - 1; k >= 0; k--) denom += g[k] / s_s[k];
        } else {
            const int p = plist[pi];
            for (int k = n - 1; k >= p; k--) denom += g[k];
            if (mode == 1 || num_out)
                for (int k = p - 1; k >= 0; k--) num += g[k] / s_s[k];
        }
        const int64_t at = ((int64_t)b * np + pi) * nfreq + f0 + slot;
        f_out[at] = (mode == 1 ? num : 1.0) / denom;
        if (denom_out) denom_out[at] = denom;
        if (num_out) num_out[at] = num;
    }
}

__global__ __launch_bounds__(256) void k_music_xcorr_front(const double2* __restrict__ rx, const double2* __restrict__ cutout,
                                                           const double2* __restrict__ taps, int ntaps,
                                                           const int64_t* __restrict__ shifts, int64_t len, double2* __restrict__ out) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= len) return;
    const int b = blockIdx.y;
    const double2* r = rx + shifts[b];
    const int tmax = (int)std::min<int64_t>(ntaps - 1, n);
    double ar = 0.0, ai = 0.0;
    for (int t = 0; t <= tmax; t++) {
        const double2 rv = r[n - t], cv = cutout[n - t], h = taps[t];
        const double pr = rv.x * cv.x + rv.y * cv.y, pim = rv.y * cv.x - rv.x * cv.y;  // rx conj(cutout)
        ar += h.x * pr - h.y * pim;
        ai += h.x * pim + h.y * pr;
    }
    out[(int64_t)b * len + n] = make_double2(ar, ai);
}

}  // namespace

}  // namespace caf

using namespace caf;

int32_t caf_music_geometry(int32_t* min_rows, int32_t* max_rows, int32_t* max_sweeps, int32_t* cov_tile, int32_t* max_batch) {
    if (min_rows) *min_rows = MUSIC_MIN_ROWS;
    if (max_rows) *max_rows = MUSIC_MAX_ROWS;
    if (max_sweeps) *max_sweeps = EIG_SWEEPS;
    if (cov_tile) *cov_tile = COV_TILE;
    if (max_batch) *max_batch = MUSIC_MAX_BATCH;
    return CAF_OK;
}

#define CAF_MUSIC_SHAPE(what)                                                                                       \
    CAF_REQUIRE(rows >= MUSIC_MIN_ROWS && rows <= MUSIC_MAX_ROWS, what ": 2 <= rows <= 256");                       \
    CAF_REQUIRE(batch >= 1 && batch <= MUSIC_MAX_BATCH, what ": 1 <= batch <= 65535")

int32_t caf_music_cov(const void* d_x, int32_t x_c128, int64_t x_len, const int64_t* h_segs, int32_t nseg, int32_t batch, int32_t rows,
                      int64_t jump, const double* h_scale, int32_t fwd_bwd, int32_t toeplitz, double* d_rx, void* stream) {
    CAF_MUSIC_SHAPE("caf_music_cov");
    CAF_REQUIRE(x_c128 == 0 || x_c128 == 1, "caf_music_cov: x_c128 must be 0 or 1");
    CAF_REQUIRE(nseg >= 1 && (int64_t)nseg * batch <= ((int64_t)1 << 24), "caf_music_cov: 1 <= segments, segments * batch <= 2^24");
    CAF_REQUIRE(jump >= 1 && jump <= ((int64_t)1 << 31), "caf_music_cov: 1 <= jump <= 2^31");
    CAF_REQUIRE(d_x && h_segs && h_scale && d_rx && x_len >= 1, "caf_music_cov: NULL argument");
    std::vector<CovSeg> segs((size_t)nseg * batch);
    for (size_t e = 0; e < segs.size(); e++) {
        const int64_t off = h_segs[3 * e], stride = h_segs[3 * e + 1], len = h_segs[3 * e + 2];
        CAF_REQUIRE(off >= 0 && stride >= 1 && len >= rows, "caf_music_cov: a segment needs offset >= 0, stride >= 1 and length >= rows");
        CAF_REQUIRE(len <= x_len && stride <= x_len && off < x_len && (len - 1) <= (x_len - 1 - off) / stride,
                    "caf_music_cov: a segment reaches past the end of x");
        segs[e].offset = off;
        segs[e].stride = stride;
        segs[e].ncols = (len - rows) / jump + 1;  // the last snapshot ends at (ncols - 1) jump + rows <= len
    }
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    CovSeg* d_segs = nullptr;
    double* d_scale = nullptr;
    double2* raw = nullptr;
    if (const int rc = sc.get(&d_segs, (int64_t)segs.size())) return rc;
    if (const int rc = sc.get(&d_scale, batch)) return rc;
    const bool post = fwd_bwd || toeplitz;
    if (post)
        if (const int rc = sc.get(&raw, (int64_t)batch * rows * rows)) return rc;
    CAF_H2D(d_segs, segs.data(), segs.size() * sizeof(CovSeg));
    CAF_H2D(d_scale, h_scale, (size_t)batch * sizeof(double));
    const int nt = (rows + COV_TILE - 1) / COV_TILE;
    hipLaunchKernelGGL(k_music_cov, dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)batch), dim3(256), 0, st, d_x, x_c128, d_segs, nseg,
                       d_scale, rows, jump, nt, post ? raw : (double2*)d_rx);
    CAF_HIP_TRY(hipGetLastError());
    if (post) {
        hipLaunchKernelGGL(k_music_cov_post, dim3((unsigned)batch), dim3(256), 0, st, raw, rows, fwd_bwd ? 1 : 0, toeplitz ? 1 : 0,
                           (double2*)d_rx);
        CAF_HIP_TRY(hipGetLastError());
    }
    return sc.finish();
}

int32_t caf_music_eig(const double* d_rx, int32_t batch, int32_t rows, double* d_s, double* d_u, double* d_vh, int32_t* d_status,
                      void* stream) {
    CAF_REQUIRE(rows >= MUSIC_MIN_ROWS && rows <= MUSIC_MAX_ROWS, "caf_music_eig: 2 <= rows <= 256");
    CAF_REQUIRE(batch >= 1, "caf_music_eig: batch >= 1");
    CAF_REQUIRE(d_rx && d_s && d_u && d_status, "caf_music_eig: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    double2 *g = nullptr, *v = nullptr;
    if (const int rc = sc.get(&g, (int64_t)batch * rows * rows)) return rc;
    if (const int rc = sc.get(&v, (int64_t)batch * rows * rows)) return rc;
    hipLaunchKernelGGL(k_music_eig, dim3((unsigned)batch), dim3(EIG_THREADS), 0, st, (const double2*)d_rx, rows, g, v, d_s, (double2*)d_u,
                       (double2*)d_vh, d_status);
    CAF_HIP_TRY(hipGetLastError());
    return sc.finish();
}

int32_t caf_music_spectrum(const double* d_u, const double* d_s, int32_t batch, int32_t rows, const double* d_freqs, int32_t nfreq,
                           const int32_t* h_plist, int32_t np, int32_t mode, double* d_f, double* d_denom, double* d_num, void* stream) {
    CAF_MUSIC_SHAPE("caf_music_spectrum");
    CAF_REQUIRE(mode >= 0 && mode <= 2, "caf_music_spectrum: mode 0 (1 / denom), 1 (num / denom) or 2 (Capon)");
    CAF_REQUIRE(nfreq >= 1, "caf_music_spectrum: nfreq >= 1");
    CAF_REQUIRE(d_u && d_s && d_freqs && d_f, "caf_music_spectrum: NULL argument");
    CAF_REQUIRE(mode == 2 ? np == 1 : (np >= 1 && np <= 4096 && h_plist != nullptr), "caf_music_spectrum: 1 <= len(plist) <= 4096 (Capon: 1)");
    std::vector<int32_t> pl((size_t)np, 0);
    if (mode != 2)
        for (int i = 0; i < np; i++) {
            CAF_REQUIRE(h_plist[i] >= 0 && h_plist[i] < rows, "caf_music_spectrum: 0 <= p < rows");
            pl[i] = h_plist[i];
        }
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    int32_t* d_pl = nullptr;
    if (const int rc = sc.get(&d_pl, np)) return rc;
    CAF_H2D(d_pl, pl.data(), pl.size() * sizeof(int32_t));
    int kt = 1;
    while (kt < rows) kt <<= 1;
    const int slots = (SP_THREADS / kt) * SP_FPT;
    hipLaunchKernelGGL(k_music_spectrum, dim3((unsigned)((nfreq + slots - 1) / slots), (unsigned)batch), dim3(SP_THREADS), 0, st,
                       (const double2*)d_u, d_s, d_freqs, nfreq, d_pl, np, mode, rows, kt, d_f, d_denom, d_num);
    CAF_HIP_TRY(hipGetLastError());
    return sc.finish();
}

int32_t caf_music_xcorr_front(const double* d_rx, int64_t rx_len, const double* d_cutout, int64_t len, const double* d_taps, int32_t ntaps,
                              const int64_t* h_shifts, int32_t batch, double* d_out, void* stream) {
    CAF_REQUIRE(batch >= 1 && batch <= MUSIC_MAX_BATCH, "caf_music_xcorr_front: 1 <= batch <= 65535");
    CAF_REQUIRE(len >= 1 && len <= rx_len && (len + 255) / 256 <= 0x7fffffff, "caf_music_xcorr_front: 1 <= len <= rx_len");
    CAF_REQUIRE(ntaps >= 1, "caf_music_xcorr_front: ntaps >= 1");
    CAF_REQUIRE(d_rx && d_cutout && d_taps && h_shifts && d_out, "caf_music_xcorr_front: NULL argument");
    for (int b = 0; b < batch; b++)
        CAF_REQUIRE(h_shifts[b] >= 0 && h_shifts[b] <= rx_len - len, "caf_music_xcorr_front: a shift reaches outside rx");
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    int64_t* d_shifts = nullptr;
    if (const int rc = sc.get(&d_shifts, batch)) return rc;
    CAF_H2D(d_shifts, h_shifts, (size_t)batch * sizeof(int64_t));
    hipLaunchKernelGGL(k_music_xcorr_front, dim3((unsigned)((len + 255) / 256), (unsigned)batch), dim3(256), 0, st, (const double2*)d_rx,
                       (const double2*)d_cutout, (const double2*)d_taps, ntaps, d_shifts, len, (double2*)d_out);
    CAF_HIP_TRY(hipGetLastError());
    return sc.finish();
}
