// Batched k-means and cluster scores (clusterRoutines.py: ClusterEngine, ClusterEngine2D, AngularClusterEngine run KMeans for
// every guess of k and score each fit, inside a loop that removes the smallest cluster and starts again).  Everything is
// float64.  P problems of up to `pitch` points in D <= 4 dimensions, ragged (lengths) and thinned (mask) in place; a JOB is
// one (problem, k) pair, a restart is one more job.
//   * caf_kmeans_seed   k-means++ from the caller's variates: one workgroup per job, D^2 of every point in pooled scratch,
//                       its running sum by a tiled workgroup scan in index order.
//   * caf_kmeans_lloyd  one workgroup per job, the whole iteration on the device.  Centres in LDS; the points in LDS too
//                       where pitch * D * 8 bytes fit KM_STAGE_BYTES (form 1), else read through L2 every pass (form 2).
//                       Both forms run the same arithmetic in the same order: they give the same bits.
//   * caf_cluster_scores  from labels alone: a workgroup per job forms counts, centroids, Davies-Bouldin and
//                       Calinski-Harabasz; the silhouette runs on a grid over (job, tile of 256 points i), every workgroup
//                       walking all points j tile by tile through LDS with one LDS COLUMN of k running sums per thread (no
//                       array indexed by a label in registers, so nothing in scratch memory); per-tile sums of s(i) go to
//                       pooled scratch and a last kernel adds them in increasing tile order.
// Orders of summation: the points in use are numbered in index order (their rank; with a mask a list rank -> index is made
// first), a thread visits the ranks r = t, t + 256, ... in increasing order, threads are folded by caf_wave.h (xor
// butterfly, waves in increasing order), clusters and tiles in increasing order.  No atomics.  A job's outputs depend on
// its own points in use, k and centres alone: not on the pitch, on what the mask leaves out, or on the other jobs.
#include "caf_internal.h"
#include "caf_wave.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <string>

namespace caf {

namespace {

constexpr int KM_THREADS = 256;  // threads per workgroup of every kernel here, and the points per tile T
constexpr int KM_WAVES = KM_THREADS / 64;
constexpr int KM_MAX_D = 4;
constexpr int KM_MAX_K = 32;
constexpr int64_t KM_MAX_PITCH = (int64_t)1 << 17;
constexpr int64_t KM_STAGE_BYTES = 128 * 1024;           // LDS for the staged points of a Lloyd job
constexpr int64_t KM_SEED_SCRATCH = (int64_t)1 << 25;    // doubles of D^2 scratch per chunk of seeding jobs

struct KmArgs {
    const double* x;
    const int32_t* lengths;
    const uint8_t* mask;
    const int32_t* idx;    // (P, pitch): the index of a problem's used point number r, or NULL (no mask: r itself)
    const int32_t* nused;  // (P) with idx
    const int32_t* job_problem;
    const int32_t* job_k;
    int64_t pitch;
    int32_t kmax;
};

using SumSlots = WaveSlots<KM_WAVES, double, double, double, double, int>;

__device__ __forceinline__ int km_length(const KmArgs& a, int p) {
    int L = a.lengths ? a.lengths[p] : (int)a.pitch;
    L = L < 0 ? 0 : L;
    return L > (int)a.pitch ? (int)a.pitch : L;
}

template <int D, typename X, typename C>
__device__ __forceinline__ double km_dist2(const X* x, const C* c) {
    double s = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const double e = x[d] - c[d];
        s += e * e;
    }
    return s;
}

// inclusive scan of one tile of 256 values in index order, on top of `carry`; the tile's total is added to the carry.
// Two barriers; `lds` and `tot` are free again on return.
template <typename T>
__device__ __forceinline__ T km_tile_scan(T v, T& carry, T (&lds)[KM_WAVES], T& tot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T incl = wave_scan_inclusive(v, lane);
    const T blk = block_carry(incl, incl, lane, wave, lds, [](T a, T b) { return a + b; });
    const T p = carry + blk;
    if (threadIdx.x == KM_THREADS - 1) tot = p;
    __syncthreads();
    carry = tot;
    return p;
}

// the smallest of the threads' values (INT_MAX: none), in every thread
__device__ __forceinline__ int km_block_min(int v, int (&lds)[KM_WAVES], int& out) {
    const int m = block_max<KM_WAVES>(INT_MAX - v, lds);
    if (threadIdx.x == 0) out = INT_MAX - m;
    __syncthreads();
    const int r = out;
    __syncthreads();
    return r;
}

// ---- rank lists ---------------------------------------------------------------------------------------------------------
// Every sum below runs over the points that count, numbered in index order (their RANK), so that a problem thinned by a mask
// gives the bits of the same problem with those points taken out.  idx[r] = the index of point number r; *n = how many.
template <typename F>
__device__ __forceinline__ void km_rank_row(int L, F flag, int32_t* __restrict__ idx, int32_t* __restrict__ n, int (&lds)[KM_WAVES],
                                            int& tot) {
    int carry = 0;
    for (int base = 0; base < L; base += KM_THREADS) {
        const int i = base + threadIdx.x;
        const int f = i < L && flag(i) ? 1 : 0;
        const int rank = km_tile_scan(f, carry, lds, tot);  // inclusive: this point is number rank - 1
        if (f) idx[rank - 1] = i;
    }
    if (threadIdx.x == 0) *n = carry;
}

// one workgroup per problem: the points its mask leaves in use
__global__ __launch_bounds__(KM_THREADS) void k_km_rank(const KmArgs a, int32_t* __restrict__ idx, int32_t* __restrict__ nused) {
    __shared__ int s_i[KM_WAVES];
    __shared__ int s_tot;
    const int p = blockIdx.x;
    const uint8_t* m = a.mask + (int64_t)p * a.pitch;
    km_rank_row(km_length(a, p), [&](int i) { return m[i] != 0; }, idx + (int64_t)p * a.pitch, nused + p, s_i, s_tot);
}

__device__ __forceinline__ int km_used(const KmArgs& a, int p, int L) { return a.idx ? a.nused[p] : L; }

// ---- seeding ------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(KM_THREADS) void k_km_seed(const KmArgs a, int64_t job0, const double* __restrict__ u,
                                                        double* __restrict__ d2all, int32_t* __restrict__ index,
                                                        double* __restrict__ centres) {
    __shared__ int s_i[KM_WAVES];
    __shared__ double s_d[KM_WAVES];
    __shared__ int s_pick;
    __shared__ double s_dtot;
    const int tid = threadIdx.x;
    const int64_t job = job0 + blockIdx.x;
    const int p = a.job_problem[job], k = a.job_k[job];
    const int n = km_used(a, p, km_length(a, p));
    const double* x = a.x + (int64_t)p * a.pitch * D;
    const int32_t* ix = a.idx ? a.idx + (int64_t)p * a.pitch : nullptr;
    double* d2 = d2all + (int64_t)blockIdx.x * a.pitch;  // by rank
    int32_t* out = index + job * a.kmax;
    double* cen = centres + job * a.kmax * D;
    const double* uj = u + job * a.kmax;
    auto point = [&](int r) { return ix ? ix[r] : r; };

    if (n < k) {  // (uniform)
        if (tid < k) out[tid] = -1;
        return;
    }
    // the first centre: used point number floor(u0 n) in index order
    int r = (int)(uj[0] * (double)n);
    r = r < 0 ? 0 : r > n - 1 ? n - 1 : r;
    int chosen = point(r);
    for (int j = 0;; ++j) {
        if (tid == 0) out[j] = chosen;
        double c[D];
#pragma unroll
        for (int d = 0; d < D; ++d) c[d] = x[(int64_t)chosen * D + d];
        if (tid < D) cen[j * D + tid] = x[(int64_t)chosen * D + tid];
        if (j + 1 == k) break;
        // D^2 to the nearest chosen centre, and its sum over the used points
        double total = 0.0;
        for (int base = 0; base < n; base += KM_THREADS) {
            const int q = base + tid;
            double v = 0.0;
            if (q < n) {
                const double e = km_dist2<D>(x + (int64_t)point(q) * D, c);
                v = j == 0 ? e : fmin(d2[q], e);
                d2[q] = v;  // (read back by this thread alone)
            }
            (void)km_tile_scan(v, total, s_d, s_dtot);
        }
        // the first used point with P > t and D^2 > 0; where rounding leaves none, the last point with D^2 > 0, and where every
        // used point coincides with a centre, the last used point
        const double t = uj[j + 1] * total;
        double run = 0.0;
        int first = INT_MAX, lastpos = -1;
        for (int base = 0; base < n; base += KM_THREADS) {
            const int q = base + tid;
            const double v = q < n ? d2[q] : 0.0;
            const double P = km_tile_scan(v, run, s_d, s_dtot);
            if (v > 0.0) {
                lastpos = q;
                if (P > t && first == INT_MAX) first = q;
            }
        }
        first = km_block_min(first, s_i, s_pick);
        if (first == INT_MAX) {  // (uniform)
            const int lp = km_block_min(lastpos < 0 ? INT_MAX : INT_MAX - 1 - lastpos, s_i, s_pick);
            first = lp != INT_MAX ? INT_MAX - 1 - lp : n - 1;
        }
        chosen = point(first > n - 1 ? n - 1 : first);  // (first < n by construction; kept inside the row whatever happens)
    }
}

// ---- Lloyd --------------------------------------------------------------------------------------------------------------
struct LloydOut {
    double* centres;  // (J, kmax, D), in and out
    int32_t* labels;
    int32_t* counts;
    double* inertia;
    int32_t* n_iter;
    int32_t* status;
    int32_t max_iter;
};

template <int D, bool STAGED>
__global__ __launch_bounds__(KM_THREADS) void k_km_lloyd(const KmArgs a, const LloydOut o) {
    extern __shared__ __attribute__((aligned(16))) double s_pts[];  // STAGED: the used points by rank
    __shared__ double s_c[KM_MAX_K * D];
    __shared__ SumSlots s_red;
    __shared__ int s_i[KM_WAVES];
    __shared__ double s_d[KM_WAVES];
    const int tid = threadIdx.x;
    const int64_t job = blockIdx.x;
    const int p = a.job_problem[job], k = a.job_k[job];
    const int L = km_length(a, p);
    const int n = km_used(a, p, L);
    const double* x = a.x + (int64_t)p * a.pitch * D;
    const int32_t* ix = a.idx ? a.idx + (int64_t)p * a.pitch : nullptr;
    int32_t* lab = o.labels + job * a.pitch;
    double* cen = o.centres + job * a.kmax * D;
    auto point = [&](int r) { return ix ? ix[r] : r; };

    if (ix || n < k)
        for (int i = tid; i < L; i += KM_THREADS) lab[i] = -1;
    if (n < k) {  // (uniform)
        if (tid == 0) o.status[job] = 1;
        return;
    }
    if (tid < k * D) s_c[tid] = cen[tid];
    if constexpr (STAGED)
        for (int r = tid; r < n; r += KM_THREADS) {
            const int i = point(r);
#pragma unroll
            for (int d = 0; d < D; ++d) s_pts[r * D + d] = x[(int64_t)i * D + d];
        }
    __syncthreads();  // (and the -1 labels are in place before another thread writes a label)
    // point number r: its coordinates and its label (thread r mod 256 alone reads and writes the labels of point r)
    auto coords = [&](int r) { return STAGED ? s_pts + r * D : x + (int64_t)point(r) * D; };

    int n_iter = 0, status = 0;
    for (int it = 0;; ++it) {
        // assignment: the nearest centre, the lower index of equal distances
        int changed = 0;
        for (int r = tid; r < n; r += KM_THREADS) {
            const double* xr = coords(r);
            double best = km_dist2<D>(xr, s_c);
            int l = 0;
            for (int c = 1; c < k; ++c) {
                const double e = km_dist2<D>(xr, s_c + c * D);
                if (e < best) best = e, l = c;
            }
            const int i = point(r);
            if (it == 0 || lab[i] != l) changed = 1, lab[i] = l;
        }
        changed = __syncthreads_or(changed);
        if (it > 0 && !changed) break;
        if (it == o.max_iter) {
            status = 3;
            break;
        }
        // update: the mean of each cluster's members; an empty cluster keeps its centre
        for (int c = 0; c < k; ++c) {
            double s[KM_MAX_D] = {0.0, 0.0, 0.0, 0.0};
            int m = 0;
            for (int r = tid; r < n; r += KM_THREADS)
                if (lab[point(r)] == c) {
                    const double* xr = coords(r);
#pragma unroll
                    for (int d = 0; d < D; ++d) s[d] += xr[d];
                    ++m;
                }
            block_sum_all<KM_WAVES>(s_red, s[0], s[1], s[2], s[3], m);
            if (tid == 0 && m > 0) {
#pragma unroll
                for (int d = 0; d < D; ++d) s_c[c * D + d] = s[d] / (double)m;
            }
        }
        __syncthreads();
        ++n_iter;
    }
    // the labels are the assignment to the centres in s_c on either exit
    double in = 0.0;
    for (int r = tid; r < n; r += KM_THREADS) in += km_dist2<D>(coords(r), s_c + lab[point(r)] * D);
    in = block_sum_all<KM_WAVES>(in, s_d);
    int empty = 0;
    for (int c = 0; c < k; ++c) {
        int m = 0;
        for (int r = tid; r < n; r += KM_THREADS) m += lab[point(r)] == c ? 1 : 0;
        m = block_sum_all<KM_WAVES>(m, s_i);
        if (tid == 0) o.counts[job * a.kmax + c] = m;
        empty |= m == 0;
    }
    if (tid < k * D) cen[tid] = s_c[tid];
    if (tid == 0) {
        o.inertia[job] = in;
        o.n_iter[job] = n_iter;
        o.status[job] = status == 3 ? 3 : empty ? 2 : 0;
    }
}

// ---- scores -------------------------------------------------------------------------------------------------------------
struct ScoreArgs {
    const int32_t* labels;  // (rows, pitch)
    const int32_t* rows;    // the row of a job's labels, or NULL: row = job
    int32_t* idx;           // scratch (J, pitch): the points that count, by rank
    int32_t* nu;            // scratch (J): how many
    int32_t* cnt;           // scratch (J, kmax)
    double* partial;        // scratch (J, tiles)
    int32_t tiles;
    uint32_t which;
    double *sil, *db, *ch, *sil_points;
};

__device__ __forceinline__ const int32_t* cs_labels(const KmArgs& a, const ScoreArgs& o, int64_t job) {
    return o.labels + (o.rows ? (int64_t)o.rows[job] : job) * a.pitch;
}

// one workgroup per job: the points whose label counts, and NaN for the others' per-point value
__global__ __launch_bounds__(KM_THREADS) void k_cs_rank(const KmArgs a, const ScoreArgs o) {
    __shared__ int s_i[KM_WAVES];
    __shared__ int s_tot;
    const int64_t job = blockIdx.x;
    const int k = a.job_k[job];
    const int L = km_length(a, a.job_problem[job]);
    const int32_t* lab = cs_labels(a, o, job);
    km_rank_row(L, [&](int i) { return lab[i] >= 0 && lab[i] < k; }, o.idx + job * a.pitch, o.nu + job, s_i, s_tot);
    if (o.sil_points)
        for (int i = threadIdx.x; i < L; i += KM_THREADS)
            if (!(lab[i] >= 0 && lab[i] < k)) o.sil_points[job * a.pitch + i] = __longlong_as_double(0x7ff8000000000000LL);
}

// counts (always), and Davies-Bouldin / Calinski-Harabasz where asked for: one workgroup per job
template <int D>
__global__ __launch_bounds__(KM_THREADS) void k_cs_prep(const KmArgs a, const ScoreArgs o) {
    __shared__ double s_c[KM_MAX_K * D], s_S[KM_MAX_K], s_W[KM_MAX_K], s_g[KM_MAX_D];
    __shared__ int s_n[KM_MAX_K];
    __shared__ SumSlots s_red;
    const int tid = threadIdx.x;
    const int64_t job = blockIdx.x;
    const int p = a.job_problem[job], k = a.job_k[job];
    const int n = o.nu[job];
    const int32_t* ix = o.idx + job * a.pitch;
    const double* x = a.x + (int64_t)p * a.pitch * D;
    const int32_t* lab = cs_labels(a, o, job);
    const bool full = (o.which & 6u) != 0;
    for (int c = 0; c < k; ++c) {
        double s[KM_MAX_D] = {0.0, 0.0, 0.0, 0.0};
        int m = 0;
        for (int r = tid; r < n; r += KM_THREADS) {
            const int i = ix[r];
            if (lab[i] == c) {
#pragma unroll
                for (int d = 0; d < D; ++d) s[d] += x[(int64_t)i * D + d];
                ++m;
            }
        }
        block_sum_all<KM_WAVES>(s_red, s[0], s[1], s[2], s[3], m);
        if (tid == 0) {
            s_n[c] = m;
            o.cnt[job * a.kmax + c] = m;
#pragma unroll
            for (int d = 0; d < D; ++d) s_c[c * D + d] = m > 0 ? s[d] / (double)m : 0.0;
        }
    }
    if (!full) return;
    {  // the mean of all points that count
        double s[KM_MAX_D] = {0.0, 0.0, 0.0, 0.0};
        int m = 0;
        for (int r = tid; r < n; r += KM_THREADS) {
            const int i = ix[r];
#pragma unroll
            for (int d = 0; d < D; ++d) s[d] += x[(int64_t)i * D + d];
            ++m;
        }
        block_sum_all<KM_WAVES>(s_red, s[0], s[1], s[2], s[3], m);
        if (tid == 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) s_g[d] = m > 0 ? s[d] / (double)m : 0.0;
        }
    }
    __syncthreads();  // s_c complete
    for (int c = 0; c < k; ++c) {  // per cluster: the sum of distances to its centroid and of their squares
        double sd = 0.0, sq = 0.0, z0 = 0.0, z1 = 0.0;
        int m = 0;
        for (int r = tid; r < n; r += KM_THREADS) {
            const int i = ix[r];
            if (lab[i] == c) {
                const double e = km_dist2<D>(x + (int64_t)i * D, s_c + c * D);
                sd += sqrt(e), sq += e;
            }
        }
        block_sum_all<KM_WAVES>(s_red, sd, sq, z0, z1, m);
        if (tid == 0) s_S[c] = s_n[c] > 0 ? sd / (double)s_n[c] : 0.0, s_W[c] = sq;
    }
    if (tid != 0) return;
    int kk = 0, nu = 0;
    for (int c = 0; c < k; ++c) kk += s_n[c] > 0, nu += s_n[c];
    const bool none = kk < 2 || kk >= nu;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (o.which & 2u) {
        double sum = 0.0;
        for (int i = 0; i < k; ++i) {
            if (s_n[i] == 0) continue;
            double worst = 0.0;
            for (int j = 0; j < k; ++j) {
                if (j == i || s_n[j] == 0) continue;
                const double md = sqrt(km_dist2<D>(s_c + i * D, s_c + j * D));
                const double r = md > 0.0 ? (s_S[i] + s_S[j]) / md : 0.0;
                worst = r > worst ? r : worst;
            }
            sum += worst;
        }
        o.db[job] = none ? nan : sum / (double)kk;
    }
    if (o.which & 4u) {
        double W = 0.0, B = 0.0;
        for (int c = 0; c < k; ++c)
            if (s_n[c] > 0) W += s_W[c], B += (double)s_n[c] * km_dist2<D>(s_c + c * D, s_g);
        o.ch[job] = none ? nan : W == 0.0 ? 1.0 : B * (double)(nu - kk) / (W * (double)(kk - 1));
    }
}

// silhouette of one tile of 256 points (by rank) of one job; dynamic LDS: k columns of 256 running sums, then a tile of points j
template <int D>
__global__ __launch_bounds__(KM_THREADS) void k_cs_sil(const KmArgs a, const ScoreArgs o) {
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    __shared__ int s_lab[KM_THREADS];
    __shared__ int s_n[KM_MAX_K];
    __shared__ double s_d[KM_WAVES];
    const int tid = threadIdx.x;
    const int64_t job = blockIdx.x / o.tiles;
    const int tile = (int)(blockIdx.x - job * o.tiles);
    const int p = a.job_problem[job], k = a.job_k[job];
    const int n = o.nu[job];
    double* acc = s_dyn;                   // acc[c * 256 + tid]
    double* s_x = s_dyn + k * KM_THREADS;  // (256, D)
    if (tile * KM_THREADS >= n) {  // (uniform) a tile behind the last point
        if (tid == 0) o.partial[job * o.tiles + tile] = 0.0;
        return;
    }
    const double* x = a.x + (int64_t)p * a.pitch * D;
    const int32_t* ix = o.idx + job * a.pitch;
    const int32_t* lab = cs_labels(a, o, job);
    if (tid < k) s_n[tid] = o.cnt[job * a.kmax + tid];
    const int r = tile * KM_THREADS + tid;
    const int i = r < n ? ix[r] : -1;
    const int li = i >= 0 ? lab[i] : -1;  // (within 0 .. k - 1 for every listed point)
    double xi[D];
#pragma unroll
    for (int d = 0; d < D; ++d) xi[d] = i >= 0 ? x[(int64_t)i * D + d] : 0.0;
    for (int c = 0; c < k; ++c) acc[c * KM_THREADS + tid] = 0.0;
    for (int base = 0; base < n; base += KM_THREADS) {
        __syncthreads();  // the tile before has been read
        const int q = base + tid;
        const int j = q < n ? ix[q] : -1;
        s_lab[tid] = j >= 0 ? lab[j] : -1;
#pragma unroll
        for (int d = 0; d < D; ++d) s_x[tid * D + d] = j >= 0 ? x[(int64_t)j * D + d] : 0.0;
        __syncthreads();
        const int nj = n - base < KM_THREADS ? n - base : KM_THREADS;
        if (i >= 0)
            for (int jj = 0; jj < nj; ++jj) acc[s_lab[jj] * KM_THREADS + tid] += sqrt(km_dist2<D>(xi, s_x + jj * D));
    }
    double s = 0.0;
    if (i >= 0 && s_n[li] > 1) {
        const double av = acc[li * KM_THREADS + tid] / (double)(s_n[li] - 1);
        double bv = __longlong_as_double(0x7ff0000000000000LL);
        for (int c = 0; c < k; ++c)
            if (c != li && s_n[c] > 0) {
                const double e = acc[c * KM_THREADS + tid] / (double)s_n[c];
                bv = e < bv ? e : bv;
            }
        const double mx = av > bv ? av : bv;
        s = mx > 0.0 && mx <= 1.7976931348623157e308 ? (bv - av) / mx : 0.0;
    }
    if (o.sil_points && i >= 0) o.sil_points[job * a.pitch + i] = s;
    s = block_sum<KM_WAVES>(s, s_d);
    if (tid == 0) o.partial[job * o.tiles + tile] = s;
}

// the tiles' sums in increasing tile order: one thread per job
__global__ __launch_bounds__(64) void k_cs_fold(const KmArgs a, const ScoreArgs o, int64_t J) {
    const int64_t job = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (job >= J) return;
    const int k = a.job_k[job];
    int kk = 0, nu = 0;
    for (int c = 0; c < k; ++c) {
        const int n = o.cnt[job * a.kmax + c];
        kk += n > 0, nu += n;
    }
    double s = 0.0;
    for (int t = 0; t < o.tiles; ++t) s += o.partial[job * o.tiles + t];
    o.sil[job] = kk < 2 || kk >= nu ? __longlong_as_double(0x7ff8000000000000LL) : s / (double)nu;
}

// ---- host ---------------------------------------------------------------------------------------------------------------
bool km_staged(int64_t pitch, int D) { return pitch * D * 8 <= KM_STAGE_BYTES; }
int64_t km_sil_lds(int D, int kmax) { return (int64_t)KM_THREADS * 8 * (kmax + D); }

// the checks that every entry point shares, before anything touches a device
int km_check(const char* who, const void* d_x, int64_t P, int64_t pitch, int32_t D, const int32_t* job_problem, const int32_t* job_k,
             int64_t J, int32_t kmax) {
    const std::string w(who);
    if (!d_x || !job_problem || !job_k) return set_error(w + ": NULL argument"), CAF_ERR_INVALID;
    if (D < 1 || D > KM_MAX_D) return set_error(w + ": 1 <= D <= 4"), CAF_ERR_INVALID;
    if (kmax < 1 || kmax > KM_MAX_K) return set_error(w + ": 1 <= kmax <= 32"), CAF_ERR_INVALID;
    if (pitch < 1 || pitch > KM_MAX_PITCH) return set_error(w + ": 1 <= pitch <= 2^17"), CAF_ERR_INVALID;
    if (P < 1 || P >= ((int64_t)1 << 31)) return set_error(w + ": 1 <= P < 2^31"), CAF_ERR_INVALID;
    if (J < 1 || J * KM_MAX_PITCH / KM_THREADS >= ((int64_t)1 << 31)) return set_error(w + ": 1 <= J < 2^22"), CAF_ERR_INVALID;
    for (int64_t j = 0; j < J; ++j) {
        if (job_k[j] < 1 || job_k[j] > kmax)
            return set_error(w + ": 1 <= k <= kmax (job " + std::to_string(j) + " has k = " + std::to_string(job_k[j]) + ")"), CAF_ERR_INVALID;
        if (job_problem[j] < 0 || job_problem[j] >= P)
            return set_error(w + ": a job's problem must lie within 0 .. P - 1 (job " + std::to_string(j) + ")"), CAF_ERR_INVALID;
    }
    return CAF_OK;
}

// the job lists on the device
int km_jobs(Scratch& sc, KmArgs& a, const int32_t* job_problem, const int32_t* job_k, int64_t J) {
    int32_t *dp = nullptr, *dk = nullptr;
    if (const int rc = sc.get(&dp, J)) return rc;
    if (const int rc = sc.get(&dk, J)) return rc;
    CAF_H2D(dp, job_problem, J * 4);
    CAF_H2D(dk, job_k, J * 4);
    a.job_problem = dp, a.job_k = dk;
    return CAF_OK;
}

// the rank lists of the problems' used points, where there is a mask
int km_ranks(Scratch& sc, KmArgs& a, int64_t P, hipStream_t st) {
    if (!a.mask) return CAF_OK;
    int32_t *idx = nullptr, *n = nullptr;
    if (const int rc = sc.get(&idx, P * a.pitch)) return rc;
    if (const int rc = sc.get(&n, P)) return rc;
    hipLaunchKernelGGL(k_km_rank, dim3((unsigned)P), dim3(KM_THREADS), 0, st, a, idx, n);
    a.idx = idx, a.nused = n;
    return CAF_OK;
}

template <int D>
int km_seed_launch(const KmArgs& a, int64_t j0, unsigned nj, const double* u, double* d2, int32_t* index, double* centres, hipStream_t st) {
    hipLaunchKernelGGL(k_km_seed<D>, dim3(nj), dim3(KM_THREADS), 0, st, a, j0, u, d2, index, centres);
    return CAF_OK;
}

template <int D>
int km_lloyd_launch(const KmArgs& a, const LloydOut& o, int64_t J, hipStream_t st) {
    if (km_staged(a.pitch, D)) {
        const size_t lds = (size_t)a.pitch * D * 8;
        if (const int rc = allow_dynamic_lds(reinterpret_cast<const void*>(k_km_lloyd<D, true>), lds)) return rc;
        hipLaunchKernelGGL((k_km_lloyd<D, true>), dim3((unsigned)J), dim3(KM_THREADS), lds, st, a, o);
    } else {
        hipLaunchKernelGGL((k_km_lloyd<D, false>), dim3((unsigned)J), dim3(KM_THREADS), 0, st, a, o);
    }
    return CAF_OK;
}

template <int D>
int km_scores_launch(const KmArgs& a, const ScoreArgs& o, int64_t J, hipStream_t st) {
    hipLaunchKernelGGL(k_cs_rank, dim3((unsigned)J), dim3(KM_THREADS), 0, st, a, o);
    hipLaunchKernelGGL(k_cs_prep<D>, dim3((unsigned)J), dim3(KM_THREADS), 0, st, a, o);
    if (o.which & 1u) {
        const size_t lds = (size_t)km_sil_lds(D, a.kmax);
        if (const int rc = allow_dynamic_lds(reinterpret_cast<const void*>(k_cs_sil<D>), lds)) return rc;
        hipLaunchKernelGGL(k_cs_sil<D>, dim3((unsigned)(J * o.tiles)), dim3(KM_THREADS), lds, st, a, o);
        hipLaunchKernelGGL(k_cs_fold, dim3((unsigned)((J + 63) / 64)), dim3(64), 0, st, a, o, J);
    }
    return CAF_OK;
}

#define KM_DISPATCH_D(D, CALL) \
    switch (D) {               \
        case 1: rc = CALL(1); break; \
        case 2: rc = CALL(2); break; \
        case 3: rc = CALL(3); break; \
        default: rc = CALL(4); break; \
    }

}  // namespace

}  // namespace caf

using namespace caf;

int32_t caf_cluster_geometry(int64_t pitch, int32_t D, int32_t kmax, int32_t* form, int32_t* threads, int32_t* tile,
                             int64_t* lloyd_lds_bytes, int64_t* sil_lds_bytes, int64_t* scratch_bytes) {
    const bool ok = pitch >= 1 && pitch <= KM_MAX_PITCH && D >= 1 && D <= KM_MAX_D && kmax >= 1 && kmax <= KM_MAX_K;
    const bool staged = ok && km_staged(pitch, D);
    const int64_t tiles = ok ? (pitch + KM_THREADS - 1) / KM_THREADS : 0;
    if (form) *form = !ok ? 0 : staged ? 1 : 2;
    if (threads) *threads = ok ? KM_THREADS : 0;
    if (tile) *tile = ok ? KM_THREADS : 0;
    if (lloyd_lds_bytes) *lloyd_lds_bytes = staged ? pitch * D * 8 : 0;
    if (sil_lds_bytes) *sil_lds_bytes = ok ? km_sil_lds(D, kmax) : 0;
    // per job: D^2 of every point while seeding; the rank list, the counts and the per-tile sums while scoring; the two job
    // lists always (a mask adds pitch * 4 + 4 bytes per PROBLEM)
    if (scratch_bytes) *scratch_bytes = ok ? std::max<int64_t>(pitch * 8, pitch * 4 + 4 + (int64_t)kmax * 4 + tiles * 8) + 8 : 0;
    return CAF_OK;
}

int32_t caf_kmeans_seed(const double* d_x, int64_t P, int64_t pitch, int32_t D, const int32_t* d_lengths, const uint8_t* d_mask,
                        const int32_t* job_problem, const int32_t* job_k, int64_t J, int32_t kmax, const double* d_u,
                        int32_t* d_index, double* d_centres, void* stream) {
    if (const int rc = km_check("caf_kmeans_seed", d_x, P, pitch, D, job_problem, job_k, J, kmax)) return rc;
    CAF_REQUIRE(d_u && d_index && d_centres, "caf_kmeans_seed: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    KmArgs a{};
    a.x = d_x, a.lengths = d_lengths, a.mask = d_mask, a.pitch = pitch, a.kmax = kmax;
    if (const int rc = km_jobs(sc, a, job_problem, job_k, J)) return rc;
    if (const int rc = km_ranks(sc, a, P, st)) return rc;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(J, KM_SEED_SCRATCH / pitch));
    double* d2 = nullptr;
    if (const int rc = sc.get(&d2, chunk * pitch)) return rc;
    for (int64_t j0 = 0; j0 < J; j0 += chunk) {
        const unsigned nj = (unsigned)std::min(chunk, J - j0);
#define KM_SEED(DD) km_seed_launch<DD>(a, j0, nj, d_u, d2, d_index, d_centres, st)
        int rc = CAF_OK;
        KM_DISPATCH_D(D, KM_SEED)
#undef KM_SEED
        if (rc) return rc;
    }
    CAF_HIP_TRY(hipGetLastError());
    return sc.finish();
}

int32_t caf_kmeans_lloyd(const double* d_x, int64_t P, int64_t pitch, int32_t D, const int32_t* d_lengths, const uint8_t* d_mask,
                         const int32_t* job_problem, const int32_t* job_k, int64_t J, int32_t kmax, int32_t max_iter,
                         double* d_centres, int32_t* d_labels, int32_t* d_counts, double* d_inertia, int32_t* d_n_iter,
                         int32_t* d_status, void* stream) {
    if (const int rc = km_check("caf_kmeans_lloyd", d_x, P, pitch, D, job_problem, job_k, J, kmax)) return rc;
    CAF_REQUIRE(d_centres && d_labels && d_counts && d_inertia && d_n_iter && d_status, "caf_kmeans_lloyd: NULL argument");
    CAF_REQUIRE(max_iter >= 1, "caf_kmeans_lloyd: max_iter >= 1");
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    KmArgs a{};
    a.x = d_x, a.lengths = d_lengths, a.mask = d_mask, a.pitch = pitch, a.kmax = kmax;
    if (const int rc = km_jobs(sc, a, job_problem, job_k, J)) return rc;
    if (const int rc = km_ranks(sc, a, P, st)) return rc;
    LloydOut o{d_centres, d_labels, d_counts, d_inertia, d_n_iter, d_status, max_iter};
    int rc = CAF_OK;
#define KM_LLOYD(DD) km_lloyd_launch<DD>(a, o, J, st)
    KM_DISPATCH_D(D, KM_LLOYD)
#undef KM_LLOYD
    if (rc) return rc;
    CAF_HIP_TRY(hipGetLastError());
    return sc.finish();
}

int32_t caf_cluster_scores(const double* d_x, int64_t P, int64_t pitch, int32_t D, const int32_t* d_lengths,
                           const int32_t* job_problem, const int32_t* job_k, int64_t J, int32_t kmax, const int32_t* d_labels,
                           const int32_t* job_rows, int64_t label_rows, uint32_t which, double* d_sil, double* d_db, double* d_ch, double* d_sil_points, void* stream) {
    if (const int rc = km_check("caf_cluster_scores", d_x, P, pitch, D, job_problem, job_k, J, kmax)) return rc;
    CAF_REQUIRE(d_labels, "caf_cluster_scores: NULL argument");
    if (job_rows)
        for (int64_t j = 0; j < J; ++j)
            CAF_REQUIRE(job_rows[j] >= 0 && job_rows[j] < label_rows, "caf_cluster_scores: a job's label row must lie within 0 .. label_rows - 1");
    CAF_REQUIRE(which >= 1 && which <= 7, "caf_cluster_scores: which is a mask of 1 (silhouette), 2 (Davies-Bouldin), 4 (Calinski-Harabasz)");
    CAF_REQUIRE((!(which & 1u) || d_sil) && (!(which & 2u) || d_db) && (!(which & 4u) || d_ch),
                "caf_cluster_scores: a selected score has a NULL output");
    CAF_REQUIRE(!d_sil_points || (which & 1u), "caf_cluster_scores: per-point values come with the silhouette");
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    KmArgs a{};
    a.x = d_x, a.lengths = d_lengths, a.pitch = pitch, a.kmax = kmax;
    if (const int rc = km_jobs(sc, a, job_problem, job_k, J)) return rc;
    ScoreArgs o{};
    o.labels = d_labels, o.tiles = (int32_t)((pitch + KM_THREADS - 1) / KM_THREADS), o.which = which;
    o.sil = d_sil, o.db = d_db, o.ch = d_ch, o.sil_points = d_sil_points;
    if (job_rows) {
        int32_t* dr = nullptr;
        if (const int rc = sc.get(&dr, J)) return rc;
        CAF_H2D(dr, job_rows, J * 4);
        o.rows = dr;
    }
    if (const int rc = sc.get(&o.idx, J * pitch)) return rc;
    if (const int rc = sc.get(&o.nu, J)) return rc;
    if (const int rc = sc.get(&o.cnt, J * kmax)) return rc;
    if (const int rc = sc.get(&o.partial, J * o.tiles)) return rc;
    int rc = CAF_OK;
#define KM_SCORES(DD) km_scores_launch<DD>(a, o, J, st)
    KM_DISPATCH_D(D, KM_SCORES)
#undef KM_SCORES
    if (rc) return rc;
    CAF_HIP_TRY(hipGetLastError());
    return sc.finish();
}
