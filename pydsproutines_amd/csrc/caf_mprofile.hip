// The matrix profile of one record (matrixProfileRoutines.py: MatrixProfile, CupyMatrixProfile).  For x[0 .. N), a window W and
// M = N - W + 1 window positions, diagonal k (1 <= k < M) holds the M - k values
//
//   v(i, k) = |sum_{t < W} x[i + t] conj(x[i + k + t])|^2 / (E[i] E[i + k]),   E[n] = sum_{t < W} |x[n + t]|^2.
//
//   k_mp_energy    E[n] for every n, float64, a plain sum in increasing t (once per call; W additions per window).
//   k_mp<MODE, T>  A work item (one workgroup of T = 256 threads; 512 for W > 1024, where the LDS leaves room for one item per CU
//                  and its waves are all the CU runs) owns the segment of MP_S positions i0 = seg MP_S ... and a chunk of
//                  MP_KC consecutive diagonals (one diagonal when the diagonals come as a list).  It loads the left slice
//                  x[i0 .. i0 + S + W - 1) and the one right window x[i0 + k .. i0 + k + KC + S + W - 2) of the chunk into LDS once,
//                  and then, per diagonal, runs mp_prefix and hands every value to the mode:
//                    mp_prefix    the products p[t] = x[i0 + t] conj(x[i0 + k + t]) are formed in float64 (a product of two float32
//                                 is exact there: one rounding per component).  Thread j owns the `epb` consecutive products from
//                                 j epb (epb odd: its 8-byte LDS reads then fall on different banks), adds them up, the totals go
//                                 through wave_scan_inclusive and block_carry of caf_wave.h, and the thread writes the running
//                                 prefix P[t + 1] = P[t] + p[t] of its products to LDS.  The window sum of position i0 + t is
//                                 P[t + W] - P[t]: nothing but the halo (S + W - 1) / S grows with W.
//                    value        (float) (|P[t + W] - P[t]|^2 / (E[i] E[i + k])), the quotient in float64, rounded once; NaN where an
//                                 energy is zero (numpy's 0 / 0).  A value is a function of x, W, k and i alone -- segments start at
//                                 multiples of MP_S whatever the call's first diagonal is -- so every mode sees the same bits and a
//                                 call on [k0, k1) is bitwise a slice of the call on all diagonals.
//                  MP_RAW      writes the value to its place in the packed output (int64 offsets relative to k0).
//                  MP_COUNT    counts the runs of v > threshold inside the (diagonal, segment), MP_FILL computes the same flags again
//                              and writes (k, start, end) of every run at its place: k_mp_rowscan turns a diagonal's counts into
//                              offsets within the diagonal, launch_scan_exclusive the diagonals' totals into offsets of the list, so
//                              the list is sorted by (k, start), nothing is atomic and no capacity is guessed.  Runs that meet at a
//                              segment boundary are joined by the caller (vectorised, matrixProfileRoutines.py), who then applies
//                              minChainLength.
//                  MP_PROFILE  keeps, per window position p, the maximum over its partners q = p +- k as a packed 64-bit key: the
//                              value's bits in the high word (non-negative floats order as integers), ~(2 k + (q > p)) in the low
//                              word, so of equal values the smallest k wins and of equal k the left partner.  A thread folds the
//                              chunk's diagonals in registers for the positions i it owns and in LDS for the positions i + k (one
//                              owner per address and diagonal: no LDS atomics), then the item sends at most 2 S + KC 64-bit integer
//                              maxima to global memory; an integer maximum does not depend on the order of arrival.  k_mp_unpack
//                              turns the keys into (value, partner); a key of 0 -- no partner in range, or NaN for all of them --
//                              gives (0, -1).
//
// Upstream's CUDA kernels (custom_kernels/matrixProfile.cu) are not the model: they read past their workspace, ignore the list of
// diagonals and minChainLength and index in 32 bits; the semantics here are those of upstream's Python class.
// Floating-point contraction is off in this file; the fused multiply-adds are written out, so the rounding model of
// tests/mp_ref.py is what the compiler emits.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "caf_internal.h"
#include "caf_wave.h"  // wave_scan_inclusive, block_carry, block_exclusive, block_sum

#pragma clang fp contract(off)

namespace caf {

namespace {

constexpr int MP_THREADS = 256;                 // threads of a work item up to W = MP_WIDE, and of the small kernels
constexpr int MP_THREADS_WIDE = 512;            // ... above it: a long window fills the LDS of its CU, and the item's waves are all the CU runs
constexpr int MP_WIDE = 1024;
constexpr int MP_S = 512;                       // window positions per work item
constexpr int MP_KC = 32;                       // diagonals per work item
constexpr int MP_WMAX = 4096;                   // the longest window
constexpr int64_t MP_LDS_LIMIT = 160 * 1024 - 64;
enum { MP_RAW = 0, MP_COUNT = 1, MP_FILL = 2, MP_PROFILE = 3 };

// the dynamic LDS of an item: P (S + W double2), the energies of its positions (S) and of their partners (S + KC), the left
// slice (S + W - 1 float2), the right window (KC + S + W - 1), and the mode's tail: flags or the partners' keys (S + KC words)
constexpr int64_t mp_lds_bytes(int64_t w) {
    return 16 * (MP_S + w) + 8 * (MP_S + MP_S + MP_KC) + 8 * (MP_S + w - 1) + 8 * (MP_KC + MP_S + w - 1) + 8 * (MP_S + MP_KC);
}
static_assert(mp_lds_bytes(MP_WMAX) <= MP_LDS_LIMIT, "the longest window must fit one CU's LDS");
static_assert(MP_S % MP_THREADS == 0 && MP_S % MP_THREADS_WIDE == 0 && MP_KC <= MP_THREADS, "a thread owns MP_ROUNDS positions; thread d clears diagonal d's count");

inline int32_t mp_threads(int32_t w) { return w > MP_WIDE ? MP_THREADS_WIDE : MP_THREADS; }
// products per thread: (S + W - 1) / threads rounded up, then up to an odd number
inline int32_t mp_epb(int32_t w) { return ((MP_S + w - 1 + mp_threads(w) - 1) / mp_threads(w)) | 1; }

struct D2 {
    double r, i;
};

struct MpArgs {
    const float2* x;
    const double* en;
    int64_t N, M;
    int32_t W, k0, ndiag, nseg, epb;
    const int32_t* diag;  // != NULL: the diagonals, strictly increasing; one per item.  NULL: k0 + 0 .. ndiag - 1, MP_KC per item
    float thr;
    float* raw;
    int32_t* counts;        // [ndiag][nseg]: MP_COUNT the runs of the (diagonal, segment); after k_mp_rowscan their offsets in the diagonal
    const int64_t* rowoff;  // [ndiag + 1] the diagonals' offsets in the list
    int64_t capacity;
    int32_t* runs;  // [capacity][3]
    unsigned long long* keys;  // [M]
};

__global__ __launch_bounds__(MP_THREADS) void k_mp_energy(const float2* __restrict__ x, int32_t W, int64_t M, double* __restrict__ en) {
    const int64_t n = (int64_t)blockIdx.x * MP_THREADS + threadIdx.x;
    if (n >= M) return;
    double e = 0.0;
    for (int32_t t = 0; t < W; t++) e += sample_energy(x[n + t]);  // (n + t <= M - 1 + W - 1 = N - 1)
    en[n] = e;
}

// x conj(y) with one rounding per component: the second product of each is exact in float64
__device__ __forceinline__ D2 mp_product(const float2 a, const float2 b) {
    return D2{__builtin_fma((double)a.x, (double)b.x, (double)a.y * (double)b.y),
              __builtin_fma((double)a.y, (double)b.x, -((double)a.x * (double)b.y))};
}

// P[0 .. L] of the L products xl[t] conj(xr[t]); ends with a barrier
template <int MP_WAVES>
__device__ __forceinline__ void mp_prefix(const float2* xl, const float2* xr, int32_t L, int32_t epb, double2* P, D2 (&s_carry)[MP_WAVES]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t tb = min(tid * epb, L), te = min(tb + epb, L);
    D2 sum{0.0, 0.0};
    for (int32_t t = tb; t < te; t++) {
        const D2 p = mp_product(xl[t], xr[t]);
        sum.r += p.r;
        sum.i += p.i;
    }
    const D2 incl{wave_scan_inclusive(sum.r, lane), wave_scan_inclusive(sum.i, lane)};
    D2 first{__shfl_up(incl.r, 1, 64), __shfl_up(incl.i, 1, 64)};  // what the lanes before this one add up to
    if (lane == 0) first = D2{0.0, 0.0};
    D2 run = block_carry(first, incl, lane, wave, s_carry, [](D2 a, D2 b) { return D2{a.r + b.r, a.i + b.i}; });
    if (tid == 0) P[0] = make_double2(0.0, 0.0);
    for (int32_t t = tb; t < te; t++) {
        const D2 p = mp_product(xl[t], xr[t]);
        run.r += p.r;
        run.i += p.i;
        P[t + 1] = make_double2(run.r, run.i);
    }
    __syncthreads();
}

__device__ __forceinline__ float mp_value(const double2* P, int32_t t, int32_t W, double e1, double e2) {
    const double2 a = P[t], b = P[t + W];
    const double dr = b.x - a.x, di = b.y - a.y;
    if (e1 == 0.0 || e2 == 0.0) return NAN;
    return (float)(__builtin_fma(dr, dr, di * di) / (e1 * e2));
}

template <int MODE, int THREADS>
__global__ __launch_bounds__(THREADS) void k_mp(const MpArgs a) {
    constexpr int MP_THREADS = THREADS, MP_WAVES = THREADS / 64, MP_ROUNDS = MP_S / THREADS;  // (shadowing the small kernels' constant)
    extern __shared__ double2 s_dyn[];
    __shared__ D2 s_carry[MP_WAVES];
    __shared__ int32_t s_cnt[MP_ROUNDS][MP_WAVES];
    __shared__ int32_t s_sum[MP_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t W = a.W;
    const int32_t seg = (int32_t)(blockIdx.x % (unsigned)a.nseg), chunk = (int32_t)(blockIdx.x / (unsigned)a.nseg);
    const int32_t per_item = a.diag ? 1 : MP_KC;
    const int32_t kk0 = chunk * per_item, nkc = min(per_item, a.ndiag - kk0);
    const int32_t kfirst = a.diag ? a.diag[kk0] : a.k0 + kk0;
    const int64_t i0 = (int64_t)seg * MP_S;
    const int32_t cnt0 = (int32_t)min((int64_t)MP_S, a.M - kfirst - i0);  // positions of the chunk's first (longest) diagonal
    if (cnt0 <= 0) {
        if (MODE == MP_COUNT && tid < nkc) a.counts[(int64_t)(kk0 + tid) * a.nseg + seg] = 0;
        return;
    }

    double2* P = s_dyn;
    double* el = (double*)(P + MP_S + W);
    double* er = el + MP_S;
    float2* xl = (float2*)(er + MP_S + MP_KC);
    float2* xr = xl + (MP_S + W - 1);
    unsigned long long* col = (unsigned long long*)(xr + (MP_KC + MP_S + W - 1));  // MP_PROFILE
    uint8_t* flags = (uint8_t*)col;                                                // MP_COUNT, MP_FILL

    for (int32_t t = tid; t < cnt0 + W - 1; t += MP_THREADS) xl[t] = a.x[i0 + t];  // (i0 + t <= N - 1 - kfirst)
    for (int32_t u = tid; u < nkc - 1 + cnt0 + W - 1; u += MP_THREADS) {
        const int64_t g = i0 + kfirst + u;
        xr[u] = g < a.N ? a.x[g] : make_float2(0.f, 0.f);
    }
    for (int32_t t = tid; t < cnt0; t += MP_THREADS) el[t] = a.en[i0 + t];
    for (int32_t u = tid; u < nkc - 1 + cnt0; u += MP_THREADS) {
        const int64_t g = i0 + kfirst + u;
        er[u] = g < a.M ? a.en[g] : 0.0;
    }
    unsigned long long row[MP_ROUNDS];
    if (MODE == MP_PROFILE) {
        for (int32_t u = tid; u < MP_S + MP_KC; u += MP_THREADS) col[u] = 0ull;
#pragma unroll
        for (int r = 0; r < MP_ROUNDS; r++) row[r] = 0ull;
    }
    __syncthreads();

    for (int32_t d = 0; d < nkc; d++) {
        const int32_t k = kfirst + d;
        const int32_t cnt = (int32_t)min((int64_t)MP_S, a.M - k - i0);
        if (cnt <= 0) {  // (and for every later diagonal of the chunk)
            if (MODE == MP_COUNT && tid < nkc - d) a.counts[(int64_t)(kk0 + d + tid) * a.nseg + seg] = 0;
            break;
        }
        mp_prefix(xl, xr + d, cnt + W - 1, a.epb, P, s_carry);

        bool is_start[MP_ROUNDS], is_end[MP_ROUNDS];
#pragma unroll
        for (int r = 0; r < MP_ROUNDS; r++) {
            const int32_t t = tid + MP_THREADS * r;
            if (t < cnt) {
                const float v = mp_value(P, t, W, el[t], er[t + d]);
                if (MODE == MP_RAW) {
                    const int64_t rel = k - a.k0;
                    a.raw[rel * a.M - ((int64_t)a.k0 + k - 1) * rel / 2 + i0 + t] = v;
                } else if (MODE == MP_PROFILE) {
                    if (v == v) {
                        const unsigned long long hi = (unsigned long long)__float_as_uint(v) << 32;
                        const unsigned long long right = hi | (uint32_t)~(2u * (uint32_t)k + 1u);  // for i: the partner i + k
                        const unsigned long long left = hi | (uint32_t)~(2u * (uint32_t)k);        // for i + k: the partner i
                        row[r] = right > row[r] ? right : row[r];
                        col[t + d] = left > col[t + d] ? left : col[t + d];  // (this thread alone touches col[t + d] in diagonal d)
                    }
                } else {
                    flags[t] = v > a.thr;
                }
            }
        }
        if (MODE == MP_COUNT || MODE == MP_FILL) {
            __syncthreads();
            int32_t mine = 0;
            unsigned long long mask[MP_ROUNDS];
#pragma unroll
            for (int r = 0; r < MP_ROUNDS; r++) {
                const int32_t t = tid + MP_THREADS * r;
                const bool f = t < cnt && flags[t];
                is_start[r] = f && (t == 0 || !flags[t - 1]);
                is_end[r] = f && (t == cnt - 1 || !flags[t + 1]);
                mine += is_start[r];
                if (MODE == MP_FILL) {
                    mask[r] = __ballot(is_start[r]);
                    if (lane == 0) s_cnt[r][wave] = __popcll(mask[r]);
                }
            }
            if (MODE == MP_COUNT) {
                const int32_t c = block_sum(mine, s_sum);
                if (tid == 0) a.counts[(int64_t)(kk0 + d) * a.nseg + seg] = c;
            } else {
                __syncthreads();
                const int64_t base = a.rowoff[kk0 + d] + a.counts[(int64_t)(kk0 + d) * a.nseg + seg];
                int32_t before = 0;  // the starts at lower positions: t = MP_THREADS r + 64 wave + lane
#pragma unroll
                for (int r = 0; r < MP_ROUNDS; r++) {
                    int32_t here = 0;
#pragma unroll
                    for (int w = 0; w < MP_WAVES; w++) {
                        if (w < wave) here += s_cnt[r][w];
                    }
                    // the starts up to and including this position: a start's and its end's rank + 1 (an end closes the last start at or before it)
                    const int32_t upto = before + here + __popcll(mask[r] & (~0ull >> (63 - lane)));
                    const int64_t at = base + upto - 1;
                    if ((is_start[r] || is_end[r]) && at < a.capacity) {
                        const int64_t pos = i0 + tid + MP_THREADS * r;
                        if (is_start[r]) {
                            a.runs[3 * at] = k;
                            a.runs[3 * at + 1] = (int32_t)pos;
                        }
                        if (is_end[r]) a.runs[3 * at + 2] = (int32_t)(pos + 1);
                    }
#pragma unroll
                    for (int w = 0; w < MP_WAVES; w++) before += s_cnt[r][w];
                }
            }
        }
        __syncthreads();  // P, the flags, the slots of the folds and col[] are free for the next diagonal
    }

    if (MODE == MP_PROFILE) {
#pragma unroll
        for (int r = 0; r < MP_ROUNDS; r++) {
            if (row[r]) atomicMax(a.keys + i0 + tid + MP_THREADS * r, row[r]);
        }
        for (int32_t u = tid; u < MP_S + MP_KC; u += MP_THREADS) {
            const unsigned long long key = col[u];
            if (key) atomicMax(a.keys + i0 + kfirst + u, key);  // (a key was written only for a partner position below M)
        }
    }
}

// the counts of one diagonal's segments -> their exclusive scan, in place; the total to rowtot
__global__ __launch_bounds__(MP_THREADS) void k_mp_rowscan(int32_t* __restrict__ counts, int32_t nseg, int64_t* __restrict__ rowtot) {
    __shared__ int32_t s_w[MP_THREADS / 64];
    __shared__ int32_t s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t* row = counts + (int64_t)blockIdx.x * nseg;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int32_t c0 = 0; c0 < nseg; c0 += MP_THREADS) {
        const int32_t s = c0 + tid;
        const int32_t v = s < nseg ? row[s] : 0;
        const int32_t incl = wave_scan_inclusive(v, lane);
        const int32_t off = s_base + block_exclusive(incl, v, lane, wave, s_w);
        if (s < nseg) row[s] = off;
        __syncthreads();
        if (tid == MP_THREADS - 1) s_base = off + v;
        __syncthreads();
    }
    if (tid == 0) rowtot[blockIdx.x] = s_base;
}

__global__ __launch_bounds__(MP_THREADS) void k_mp_unpack(const unsigned long long* __restrict__ keys, int64_t M, float* __restrict__ val,
                                                        int32_t* __restrict__ idx) {
    const int64_t p = (int64_t)blockIdx.x * MP_THREADS + threadIdx.x;
    if (p >= M) return;
    const unsigned long long key = keys[p];
    if (key == 0ull) {
        val[p] = 0.f;
        idx[p] = -1;
        return;
    }
    const uint32_t code = ~(uint32_t)key;
    const int64_t k = code >> 1;
    val[p] = __uint_as_float((uint32_t)(key >> 32));
    idx[p] = (int32_t)((code & 1u) ? p + k : p - k);
}

template <int MODE>
int launch_mp(const MpArgs& a, int64_t items, hipStream_t st) {
    const size_t lds = (size_t)mp_lds_bytes(a.W);
    if (mp_threads(a.W) == MP_THREADS_WIDE) {
        if (const int rc = allow_dynamic_lds((const void*)k_mp<MODE, MP_THREADS_WIDE>, lds)) return rc;
        hipLaunchKernelGGL((k_mp<MODE, MP_THREADS_WIDE>), dim3((unsigned)items), dim3(MP_THREADS_WIDE), lds, st, a);
    } else {
        if (const int rc = allow_dynamic_lds((const void*)k_mp<MODE, MP_THREADS>, lds)) return rc;
        hipLaunchKernelGGL((k_mp<MODE, MP_THREADS>), dim3((unsigned)items), dim3(MP_THREADS), lds, st, a);
    }
    return CAF_OK;
}

// the checks every call shares, and what follows from N and W
int mp_common(const char* what, const float* d_x, int64_t n, int32_t w, int64_t* m, int32_t* nseg) {
    const std::string s(what);
    if (!(n >= 2 && n < ((int64_t)1 << 31))) return set_error(s + ": 2 <= N < 2^31"), CAF_ERR_INVALID;
    if (!(w >= 1 && w <= MP_WMAX)) return set_error(s + ": 1 <= W <= " + std::to_string(MP_WMAX)), CAF_ERR_INVALID;
    if (!(n > w)) return set_error(s + ": the record must be longer than the window"), CAF_ERR_INVALID;
    if (!d_x) return set_error(s + ": NULL argument"), CAF_ERR_INVALID;
    *m = n - w + 1;
    *nseg = (int32_t)((*m - 1 + MP_S - 1) / MP_S);  // segments of the longest diagonal (M - 1 values)
    return CAF_OK;
}

int mp_items(const char* what, int64_t ndiag, bool list, int32_t nseg, int64_t* items) {
    const int64_t chunks = list ? ndiag : (ndiag + MP_KC - 1) / MP_KC;
    *items = chunks * nseg;
    if (*items >= ((int64_t)1 << 31)) return set_error(std::string(what) + ": more than 2^31 work items; restrict the diagonals of one call"), CAF_ERR_INVALID;
    return CAF_OK;
}

int mp_energy(const float2* x, int32_t w, int64_t m, Scratch& sc, double** en, hipStream_t st) {
    if (const int rc = sc.get(en, m)) return rc;
    hipLaunchKernelGGL(k_mp_energy, dim3(cdiv(m, MP_THREADS)), dim3(MP_THREADS), 0, st, x, w, m, *en);
    return CAF_OK;
}

}  // namespace

}  // namespace caf

using namespace caf;

int32_t caf_mp_geometry(int64_t n, int32_t w, int64_t num_diagonals, int32_t* segment, int32_t* chunk, int32_t* max_window,
                        int32_t* products_per_thread, int64_t* energy_bytes, int64_t* chains_bytes, int64_t* profile_bytes, int64_t* lds_bytes) {
    if (segment) *segment = MP_S;
    if (chunk) *chunk = MP_KC;
    if (max_window) *max_window = MP_WMAX;
    const bool sized = n >= 2 && w >= 1 && w <= MP_WMAX && n > w;
    const int64_t m = sized ? n - w + 1 : 0;
    const int64_t nseg = sized ? (m - 1 + MP_S - 1) / MP_S : 0;
    if (products_per_thread) *products_per_thread = sized ? mp_epb(w) : 0;
    if (energy_bytes) *energy_bytes = 8 * m;
    if (chains_bytes) *chains_bytes = sized && num_diagonals > 0 ? 8 * m + 4 * num_diagonals * nseg + 8 * (num_diagonals + 1) : 0;
    if (profile_bytes) *profile_bytes = 16 * m;
    if (lds_bytes) *lds_bytes = sized ? mp_lds_bytes(w) : 0;
    return CAF_OK;
}

int32_t caf_mp_raw(const float* d_x, int64_t n, int32_t w, int32_t k0, int32_t k1, float* d_out, void* stream) {
    int64_t m = 0, items = 0;
    int32_t nseg = 0;
    if (const int rc = mp_common("caf_mp_raw", d_x, n, w, &m, &nseg)) return rc;
    CAF_REQUIRE(k0 >= 1 && k0 < k1 && k1 <= m, "caf_mp_raw: 1 <= k0 < k1 <= N - W + 1");
    CAF_REQUIRE(d_out, "caf_mp_raw: NULL argument");
    if (const int rc = mp_items("caf_mp_raw", (int64_t)k1 - k0, false, nseg, &items)) return rc;
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    MpArgs a{};
    a.x = (const float2*)d_x, a.N = n, a.M = m, a.W = w, a.k0 = k0, a.ndiag = k1 - k0, a.nseg = nseg, a.epb = mp_epb(w), a.raw = d_out;
    double* en = nullptr;
    if (const int rc = mp_energy(a.x, w, m, sc, &en, st)) return rc;
    a.en = en;
    if (const int rc = launch_mp<MP_RAW>(a, items, st)) return rc;
    CAF_HIP_TRY(hipGetLastError());
    return sc.finish();
}

int32_t caf_mp_chains(const float* d_x, int64_t n, int32_t w, int32_t k0, int32_t k1, const int32_t* d_diagonals, int32_t num_diagonals,
                      float min_threshold, int64_t capacity, int32_t* d_runs, int64_t* h_total, void* stream) {
    int64_t m = 0, items = 0;
    int32_t nseg = 0;
    if (const int rc = mp_common("caf_mp_chains", d_x, n, w, &m, &nseg)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool list = d_diagonals != nullptr;
    if (list) {  // (downloaded and checked before a launch: <= 2^31 words, complete on return)
        CAF_REQUIRE(num_diagonals >= 1, "caf_mp_chains: an empty list of diagonals");
        std::vector<int32_t> h((size_t)num_diagonals);
        if (const int rc = host_d2h(h.data(), d_diagonals, (int64_t)num_diagonals * 4, st)) return rc;
        for (int32_t i = 0; i < num_diagonals; i++) {
            if (h[i] < 1 || h[i] >= m || (i && h[i] <= h[i - 1])) {
                set_error("caf_mp_chains: the diagonals must be strictly increasing within 1 .. N - W (entry " + std::to_string(i) + " is " +
                          std::to_string(h[i]) + ")");
                return CAF_ERR_INVALID;
            }
        }
        k0 = 0;
    } else {
        CAF_REQUIRE(k0 >= 1 && k0 < k1 && k1 <= m, "caf_mp_chains: 1 <= k0 < k1 <= N - W + 1");
        num_diagonals = k1 - k0;
    }
    CAF_REQUIRE(h_total && capacity >= 0 && (capacity == 0 || d_runs), "caf_mp_chains: h_total is required, and d_runs with a capacity");
    CAF_REQUIRE(!std::isnan(min_threshold), "caf_mp_chains: the threshold is NaN");
    if (const int rc = mp_items("caf_mp_chains", num_diagonals, list, nseg, &items)) return rc;
    Scratch sc(st);
    MpArgs a{};
    a.x = (const float2*)d_x, a.N = n, a.M = m, a.W = w, a.k0 = k0, a.ndiag = num_diagonals, a.nseg = nseg, a.epb = mp_epb(w);
    a.diag = d_diagonals, a.thr = min_threshold, a.capacity = capacity, a.runs = d_runs;
    double* en = nullptr;
    int64_t* rowoff = nullptr;
    if (const int rc = mp_energy(a.x, w, m, sc, &en, st)) return rc;
    if (const int rc = sc.get(&a.counts, (int64_t)num_diagonals * nseg)) return rc;
    if (const int rc = sc.get(&rowoff, (int64_t)num_diagonals + 1)) return rc;
    a.en = en, a.rowoff = rowoff;
    if (const int rc = launch_mp<MP_COUNT>(a, items, st)) return rc;
    hipLaunchKernelGGL(k_mp_rowscan, dim3((unsigned)num_diagonals), dim3(MP_THREADS), 0, st, a.counts, nseg, rowoff);
    launch_scan_exclusive(rowoff, (int64_t)num_diagonals, st);
    CAF_HIP_TRY(hipGetLastError());
    if (const int rc = host_d2h(h_total, rowoff + num_diagonals, 8, st)) return rc;
    if (capacity > 0 && *h_total > 0) {
        if (const int rc = launch_mp<MP_FILL>(a, items, st)) return rc;
        CAF_HIP_TRY(hipGetLastError());
    }
    return sc.finish();
}

int32_t caf_mp_profile(const float* d_x, int64_t n, int32_t w, int32_t kmin, int32_t kmax, float* d_value, int32_t* d_index, void* stream) {
    int64_t m = 0, items = 0;
    int32_t nseg = 0;
    if (const int rc = mp_common("caf_mp_profile", d_x, n, w, &m, &nseg)) return rc;
    CAF_REQUIRE(kmin >= 1 && kmax <= m - 1, "caf_mp_profile: 1 <= kmin and kmax <= N - W");
    CAF_REQUIRE(d_value && d_index, "caf_mp_profile: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st);
    unsigned long long* keys = nullptr;
    if (const int rc = sc.get(&keys, m)) return rc;
    CAF_HIP_TRY(hipMemsetAsync(keys, 0, (size_t)m * 8, st));
    if (kmin <= kmax) {  // (an empty range: every position without a partner)
        if (const int rc = mp_items("caf_mp_profile", (int64_t)kmax - kmin + 1, false, nseg, &items)) return rc;
        MpArgs a{};
        a.x = (const float2*)d_x, a.N = n, a.M = m, a.W = w, a.k0 = kmin, a.ndiag = kmax - kmin + 1, a.nseg = nseg, a.epb = mp_epb(w), a.keys = keys;
        double* en = nullptr;
        if (const int rc = mp_energy(a.x, w, m, sc, &en, st)) return rc;
        a.en = en;
        if (const int rc = launch_mp<MP_PROFILE>(a, items, st)) return rc;
    }
    hipLaunchKernelGGL(k_mp_unpack, dim3(cdiv(m, MP_THREADS)), dim3(MP_THREADS), 0, st, (const unsigned long long*)keys, m, d_value, d_index);
    CAF_HIP_TRY(hipGetLastError());
    return sc.finish();
}
