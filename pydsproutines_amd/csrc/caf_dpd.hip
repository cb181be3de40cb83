// Direct position determination (localizationRoutines.py: gridSearchCAF_direct, DPDMixin): CAF surfaces added up over a grid of
// candidate points, without a per-pair decision.  For a grid point p and the record k = (s1, s2, v1, v2) with its map
// (surface, nd, nf, stride_d, stride_f, r0, inv_dr, d0, inv_dd, w, fill):
//   x = rho2 - rho1,  y = u2 - u1,  u_i = (p - s_i).v_i / rho_i                   (k_locate's operations, caf_locate.hip)
//   a = (x - r0) inv_dr,  b = (y - d0) inv_dd                                     (one difference, one product each)
//   in range: 0 <= a <= nd - 1 and 0 <= b <= nf - 1 (a NaN fails);  i = min(floor(a), nd - 2), t = a - i, j and s from b alike
//   value = lerp(lerp(S[i, j], S[i, j + 1], s), lerp(S[i + 1, j], S[i + 1, j + 1], s), t),  lerp(p, q, t) = fma(t, q - p, p)
//           in float64 on the float32 corners (their differences are exact); out of range: value = fill, and no hit
//   score[p] = sum_k w_k value_k      in the order of k, one fma per record.
// TD maps (nf == 1) have no b, read no velocity and take one lerp along d; FD maps (nd == 1) one along f.  A NaN corner of the
// touched cell makes the score NaN, also at weight 0 of that corner.  A point on a sensor has that range 0 (selected) and a NaN
// range rate, which is a miss.
//
//   k_dpd<TD, FD, SRC>   k_locate's frame (caf_grid.h): one workgroup per DPD_P = 1024 consecutive points (four per thread, 256
//                        apart) and per set (blockIdx.y); records and maps staged in LDS DPD_C = 64 at a time (8 + 5 KiB) and read
//                        back as broadcasts.  The corners are gathered through L2: neighbouring points touch neighbouring cells.
//   k_grid_fold<true>    the workgroups' (maximum, index) partials of each set -> one (value, index) per set: first of equal values,
//                        NaN never wins, nothing but NaN: (NaN, -1).  No atomics.
// Every load lies inside the map for every input: the coordinates are clamped into [0, nd - 1] x [0, nf - 1] before they are split
// (fmax drops a NaN), so the clamped coordinate of an in-range lookup is the coordinate itself, and a miss loads a cell it does not
// use.  All surface offsets are int64.
//
// The error count, in units of eps = 2^-53 (tests/dpd_ref.py forms the bound from it): x is off by c1 (rho1 + rho2), c1 = 6, and y
// by c2 sum_i |a_i v_i| / rho, c2 = 10 (caf_locate.hip); a = (x - r0) inv_dr rounds twice: |da| <= |inv_dr| dx + 2 |a|, t = a - i
// is exact; the three lerps: each fma rounds once and the difference of the two f-lerps once, 4 times the largest corner
// magnitude; the running sum rounds once per record.
// The maps (a host array, checked here first) and the arg max partials ride the call's stream in one pooled block: a pinned
// staging block, hipMemcpyAsync, the launches, an event (caf_lane.h).  The call waits for nothing.
// Floating-point contraction is off in this file: every product and sum is rounded where it is written, and each fma is spelled.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "caf_internal.h"
#include "caf_grid.h"
#include "caf_lane.h"
#include "caf_wave.h"

#pragma clang fp contract(off)

namespace caf {

namespace {

constexpr int DPD_T = 256;              // threads per workgroup
constexpr int DPD_PPT = 4;              // points per thread
constexpr int DPD_P = DPD_T * DPD_PPT;  // points per workgroup
constexpr int DPD_C = 64;               // records per LDS chunk (8 KiB of records, 5 KiB of maps)
constexpr int DPD_REC = 16;             // doubles per record: s1(3) s2(3) v1(3) v2(3), four not read
constexpr int DPD_MAPW = sizeof(caf_dpd_map) / 8;  // a map in 8-byte words
constexpr int64_t DPD_MAX_K = (int64_t)1 << 20;
static_assert(sizeof(caf_dpd_map) == 80 && DPD_MAPW * 8 == sizeof(caf_dpd_map), "caf_dpd_map is ten 8-byte words");

// a coordinate clamped into [0, top] (NaN -> 0) and split into the cell's first entry (at most last) and the fraction
__device__ __forceinline__ void split_clamped(double c, double top, int last, int& i, double& t) {
    const double cc = fmin(fmax(c, 0.0), top);
    i = std::min((int)cc, last);
    t = cc - (double)i;
}

template <bool TD, bool FD, int SRC>
__global__ __launch_bounds__(DPD_T) void k_dpd(const LocSrc src, int64_t N, const double* __restrict__ rec, const caf_dpd_map* __restrict__ maps,
                                               int64_t K, const int64_t* __restrict__ set_starts, void* __restrict__ score, int score_f32,
                                               int32_t* __restrict__ hits, double* __restrict__ part_v, int64_t* __restrict__ part_i) {
    __shared__ double s_rec[DPD_C * DPD_REC];
    __shared__ caf_dpd_map s_map[DPD_C];
    __shared__ WaveSlots<DPD_T / 64, double, long long> s_best;
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * DPD_P;
    const int set = blockIdx.y;

    int64_t k0, k1;
    set_records(set_starts, set, K, k0, k1);

    double px[DPD_PPT], py[DPD_PPT], pz[DPD_PPT], acc[DPD_PPT];
    int32_t hit[DPD_PPT];
    loc_points<SRC, DPD_T, DPD_PPT>(src, N, base, tid, px, py, pz);
#pragma unroll
    for (int j = 0; j < DPD_PPT; j++) acc[j] = 0.0, hit[j] = 0;

    for (int64_t kc = k0; kc < k1; kc += DPD_C) {
        const int nrec = (int)std::min<int64_t>(DPD_C, k1 - kc);
        const double* g = rec + kc * DPD_REC;
        for (int q = tid; q < nrec * DPD_REC; q += DPD_T) s_rec[q] = g[q];
        const uint64_t* gm = reinterpret_cast<const uint64_t*>(maps + kc);
        uint64_t* sm = reinterpret_cast<uint64_t*>(s_map);
        for (int q = tid; q < nrec * DPD_MAPW; q += DPD_T) sm[q] = gm[q];
        __syncthreads();
        for (int k = 0; k < nrec; k++) {
            const double* r = s_rec + k * DPD_REC;  // the same address in every lane: broadcast reads
            const caf_dpd_map& m = s_map[k];
            const double s1x = r[0], s1y = r[1], s1z = r[2], s2x = r[3], s2y = r[4], s2z = r[5];
            double v1x = 0, v1y = 0, v1z = 0, v2x = 0, v2y = 0, v2z = 0;
            if constexpr (FD) v1x = r[6], v1y = r[7], v1z = r[8], v2x = r[9], v2y = r[10], v2z = r[11];
            const float* __restrict__ surf = m.d_surface;
            const int64_t sd = m.stride_d, sf = m.stride_f;
            const double w = m.w, fill = m.fill;
            const double top_d = (double)(m.nd - 1), top_f = (double)(m.nf - 1);
#pragma unroll
            for (int j = 0; j < DPD_PPT; j++) {
                const double a1x = px[j] - s1x, a1y = py[j] - s1y, a1z = pz[j] - s1z;
                const double a2x = px[j] - s2x, a2y = py[j] - s2y, a2z = pz[j] - s2z;
                const double q1 = fma(a1z, a1z, fma(a1y, a1y, a1x * a1x));
                const double q2 = fma(a2z, a2z, fma(a2y, a2y, a2x * a2x));
                const double y1 = rsqrt_once(q1), y2 = rsqrt_once(q2);
                bool in = true;
                int64_t off = 0;
                double td = 0.0, tf = 0.0;
                if constexpr (TD) {
                    const double rho1 = q1 == 0.0 ? 0.0 : q1 * y1;
                    const double rho2 = q2 == 0.0 ? 0.0 : q2 * y2;
                    const double a = ((rho2 - rho1) - m.r0) * m.inv_dr;
                    in = a >= 0.0 && a <= top_d;  // (a NaN fails both)
                    int i;
                    split_clamped(a, top_d, m.nd - 2, i, td);
                    off = (int64_t)i * sd;
                }
                if constexpr (FD) {
                    const double u1 = fma(a1z, v1z, fma(a1y, v1y, a1x * v1x)) * y1;
                    const double u2 = fma(a2z, v2z, fma(a2y, v2y, a2x * v2x)) * y2;
                    const double b = ((u2 - u1) - m.d0) * m.inv_dd;
                    in = in && b >= 0.0 && b <= top_f;
                    int i;
                    split_clamped(b, top_f, m.nf - 2, i, tf);
                    off += (int64_t)i * sf;
                }
                // two lerps along f, then one along d; the corners' differences are exact in float64
                double v;
                if constexpr (FD) {
                    const double c00 = (double)surf[off], c01 = (double)surf[off + sf];
                    v = fma(tf, c01 - c00, c00);
                    if constexpr (TD) {
                        const double c10 = (double)surf[off + sd], c11 = (double)surf[off + sd + sf];
                        const double v1 = fma(tf, c11 - c10, c10);
                        v = fma(td, v1 - v, v);
                    }
                } else {
                    const double c0 = (double)surf[off], c1 = (double)surf[off + sd];
                    v = fma(td, c1 - c0, c0);
                }
                acc[j] = fma(w, in ? v : fill, acc[j]);
                hit[j] += in ? 1 : 0;
            }
        }
        __syncthreads();  // the chunk is overwritten next
    }

    const int64_t out0 = (int64_t)set * N;
    if (score || hits) {
#pragma unroll
        for (int j = 0; j < DPD_PPT; j++) {
            const int64_t at = base + tid + j * DPD_T;
            if (at < N) {
                if (score) store_value(score, score_f32, out0 + at, acc[j]);
                if (hits) hits[out0 + at] = hit[j];
            }
        }
    }
    if (part_v) {
        double bv;
        long long bi;
        thread_first_max<DPD_T, DPD_PPT>(acc, N, base, tid, bv, bi);
        block_argmax(s_best, bv, bi);
        if (tid == 0) {
            const int64_t o = (int64_t)set * gridDim.x + blockIdx.x;
            part_v[o] = bv;
            part_i[o] = (int64_t)bi;
        }
    }
}

using DpdKernel = void (*)(const LocSrc, int64_t, const double*, const caf_dpd_map*, int64_t, const int64_t*, void*, int, int32_t*, double*,
                           int64_t*);

// the maps of the call, each by the rules of its mode, or a refusal that names the map
int32_t dpd_maps_ok(const caf_dpd_map* h_maps, int64_t K, int mode) {
    for (int64_t k = 0; k < K; ++k) {
        const caf_dpd_map& m = h_maps[k];
        const std::string at = " (map " + std::to_string(k) + ")";
        CAF_REQUIRE(m.d_surface != nullptr, "caf_dpd_grid: NULL surface" + at);
        if (mode == CAF_LOCATE_TD) CAF_REQUIRE(m.nd >= 2 && m.nf == 1, "caf_dpd_grid: a TD map needs nd >= 2 and nf == 1" + at);
        if (mode == CAF_LOCATE_FD) CAF_REQUIRE(m.nd == 1 && m.nf >= 2, "caf_dpd_grid: an FD map needs nd == 1 and nf >= 2" + at);
        if (mode == CAF_LOCATE_TDFD) CAF_REQUIRE(m.nd >= 2 && m.nf >= 2, "caf_dpd_grid: a TDFD map needs nd >= 2 and nf >= 2" + at);
        CAF_REQUIRE((m.nd == 1 || m.stride_d != 0) && (m.nf == 1 || m.stride_f != 0),
                    "caf_dpd_grid: the stride of an axis with more than one entry must not be 0" + at);
        CAF_REQUIRE(std::isfinite(m.r0) && std::isfinite(m.inv_dr) && std::isfinite(m.d0) && std::isfinite(m.inv_dd) && std::isfinite(m.w) &&
                        std::isfinite(m.fill),
                    "caf_dpd_grid: r0, inv_dr, d0, inv_dd, w and fill must be finite" + at);
    }
    return CAF_OK;
}

}  // namespace

}  // namespace caf

using namespace caf;

int32_t caf_dpd_geometry(int32_t* points_per_workgroup, int32_t* records_per_chunk) {
    if (points_per_workgroup) *points_per_workgroup = DPD_P;
    if (records_per_chunk) *records_per_chunk = DPD_C;
    return CAF_OK;
}

int32_t caf_dpd_grid(const caf_dpd_desc* desc) {
    CAF_REQUIRE(desc != nullptr, "caf_dpd_grid: NULL descriptor");
    const caf_locate_desc* grid = &desc->grid;
    const int mode = grid->mode;
    CAF_REQUIRE(mode == CAF_LOCATE_TD || mode == CAF_LOCATE_FD || mode == CAF_LOCATE_TDFD,
                "caf_dpd_grid: mode must be CAF_LOCATE_TD, CAF_LOCATE_FD or CAF_LOCATE_TDFD");
    LocSrc src;
    int64_t N, tiles;
    int rc;
    if ((rc = grid_source("caf_dpd_grid", grid, DPD_T, DPD_P, &src, &N, &tiles))) return rc;
    const int64_t K = desc->K;
    const int32_t B = desc->B;
    if ((rc = grid_sets_ok("caf_dpd_grid", grid, desc->d_records, K, desc->d_set_starts, B, 1))) return rc;
    CAF_REQUIRE(K <= DPD_MAX_K, "caf_dpd_grid: at most 2^20 records and maps per call");
    CAF_REQUIRE(desc->h_maps != nullptr, "caf_dpd_grid: NULL map array (a host array of K caf_dpd_map)");
    if ((rc = dpd_maps_ok(desc->h_maps, K, mode))) return rc;
    const bool want_max = desc->d_max_val != nullptr || desc->d_max_idx != nullptr;
    if (!desc->d_score && !desc->d_hits && !want_max) return CAF_OK;

    hipStream_t st = (hipStream_t)desc->stream;
    int dev = 0;
    CAF_HIP_TRY(hipGetDevice(&dev));
    const int64_t map_bytes = K * (int64_t)sizeof(caf_dpd_map);  // (a multiple of 16: the partials behind it stay aligned)
    const int64_t nparts = want_max ? (int64_t)B * tiles : 0;
    Lane* lane = nullptr;
    if ((rc = lane_acquire("caf_dpd_grid", dev, map_bytes, &lane))) return rc;
    std::memcpy(lane->pinned, desc->h_maps, (size_t)map_bytes);
    void* d_block = nullptr;
    if ((rc = pool_alloc(&d_block, map_bytes + nparts * 16, st == nullptr))) {
        lane_abandon(lane, nullptr, st);
        return rc;
    }
    const caf_dpd_map* d_maps = (const caf_dpd_map*)d_block;
    double* pv = want_max ? (double*)((char*)d_block + map_bytes) : nullptr;
    int64_t* pi = want_max ? (int64_t*)(pv + nparts) : nullptr;

    hipError_t e = hipMemcpyAsync(d_block, lane->pinned, (size_t)map_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        for_source(grid->source, [&](auto s) {
            constexpr int SRC = decltype(s)::value;
            const DpdKernel k = mode == CAF_LOCATE_TD ? k_dpd<true, false, SRC> : mode == CAF_LOCATE_FD ? k_dpd<false, true, SRC> : k_dpd<true, true, SRC>;
            hipLaunchKernelGGL(k, dim3((unsigned)tiles, (unsigned)B), dim3(DPD_T), 0, st, src, N, desc->d_records, d_maps, K, desc->d_set_starts,
                               desc->d_score, grid->cost_f32, desc->d_hits, pv, pi);
        });
        e = hipGetLastError();
    }
    if (e == hipSuccess && want_max) {
        // (the fold reads a minimum's partials too: it is given the maxima's, and its minimum goes nowhere)
        hipLaunchKernelGGL(k_grid_fold<true>, dim3((unsigned)B), dim3(GRID_FOLD_T), 0, st, GridParts{pv, pi, pv, pi}, tiles, (double*)nullptr,
                           (int64_t*)nullptr, desc->d_max_val, desc->d_max_idx);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(lane->ev, st);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        lane_abandon(lane, d_block, st);
        set_error(std::string("caf_dpd_grid: ") + hipGetErrorString(e));
        return CAF_ERR_HIP;
    }
    lane_in_flight(lane, d_block);
    return CAF_OK;
}
