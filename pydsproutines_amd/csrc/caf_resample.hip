// Any-ratio resampler for ragged batches (filterRoutines.py: resampleRows; demodulationRoutines.py: conditionBursts).
// Per row r: x_r[n] (complex64, 0 outside 0 <= n < L_r), a carrier nu_r to remove, the input position t0_r of output 0, step_r
// input samples per output, w_r input samples per unit of the pulse argument, M_r outputs; one pulse table p[0 .. 2 H Q] for the
// call, h(u) its linear interpolation at (u + H) Q and 0 for |u| >= H:
//     t_m    = fma(m, step_r, t0_r)                                                                  (float64)
//     y_r[m] = (1 / w_r) sum_{n = a .. b} x_r[n] e^{-j 2 pi nu_r n} h((t_m - n) / w_r),   m < M_r;     0 for M_r <= m < out_pitch
//     a = max(floor(t_m - H w_r) + 1, 0), b = min(ceil(t_m + H w_r) - 1, L_r - 1)                     (float64, H w_r rounded once)
// One launch, k_resample.  A workgroup owns one tile of T outputs of one row:
//   table   p goes to LDS once per workgroup (a workgroup walks the rows blockIdx.y, blockIdx.y + gridDim.y, ...).
//   slice   the samples floor(t_first - H w) + 1 .. ceil(t_last + H w) - 1 of the row, clipped to the row, staged in LDS already
//           mixed: the phasor of sample n comes from nu n reduced exactly to a fraction of a turn (caf_phase.h), nothing is
//           carried from one sample to the next, so a sample has the same mixed value in whatever tile stages it.
//   sum     a thread owns the outputs m0 + tid, m0 + tid + 256, ... and runs n upwards through its own support.  The table
//           position q = fma(t_m - n, Q / w, H Q), clamped to 0 .. 2 H Q, is float64 and is split into entry i and fraction f;
//           the lerp fma(f, p[i + 1] - p[i], p[i]), the products and the sum (one fma per part and term) are float32, and so
//           is the final product with the float32 nearest 1 / w.
// T is chosen per call from the largest step and width (rs_geometry): the largest power of two up to 1024 whose table and
// slice fit the 160 KiB of LDS.  No atomics; the order of an output's sum depends on (t_m, w) alone, so a row gives the same
// bits alone, anywhere in a batch, for every T, on every run.  Every load is checked against L_r; every element of d_y up to
// out_pitch is written.
// The rows' records (host arrays, checked here first) ride the call's stream (caf_lane.h): a pinned staging block,
// hipMemcpyAsync into a pooled device block, the launch, an event.  Both blocks stay with their lane until that event has
// completed -- asked, never waited for, by the calls that follow -- and only then does the device block go back to the pool:
// stream order, with no synchronisation on either the null stream or a caller's.
#include "caf_internal.h"
#include "caf_lane.h"
#include "caf_phase.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#pragma clang fp contract(off)

namespace caf {

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_MAX_TILE = 1024;
constexpr int64_t RS_LDS = 160 * 1024;

struct RsRow {
    double nu, t0, step;
    double r;   // Q / w
    double hw;  // H w
    float inv_w;
    int32_t len, count;
    int32_t pad;
};

struct RsArgs {
    const float2* x;
    int64_t pitch, rows;
    const RsRow* row;
    const float* table;
    int32_t H, Q, tile, cap;  // cap: the samples the slice holds
    float2* y;
    int64_t out_pitch;
};

__device__ __forceinline__ int64_t rs_min(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ int64_t rs_max(int64_t a, int64_t b) { return a > b ? a : b; }

__global__ __launch_bounds__(RS_THREADS) void k_resample(const RsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int np = 2 * a.H * a.Q + 1;
    float* s_p = s_mem;
    float2* s_x = reinterpret_cast<float2*>(s_mem + ((np + 3) & ~3));
    const int tid = threadIdx.x;
    for (int i = tid; i < np; i += RS_THREADS) s_p[i] = a.table[i];
    const double hq = (double)(a.H * a.Q), top = 2.0 * hq;
    const int last = np - 2;  // the last entry a lerp may start from
    const int64_t m0 = (int64_t)blockIdx.x * a.tile;
    const int64_t m1 = rs_min(m0 + a.tile, a.out_pitch);

    for (int64_t row = blockIdx.y; row < a.rows; row += gridDim.y) {
        const RsRow rr = a.row[row];
        float2* yr = a.y + row * a.out_pitch;
        if (m0 >= rr.count) {  // a tile past M_r only writes its zeros
            for (int64_t m = m0 + tid; m < m1; m += RS_THREADS) yr[m] = make_float2(0.f, 0.f);
            continue;
        }
        const float2* xr = a.x + row * a.pitch;
        const int64_t mlast = rs_min(m1, rr.count) - 1;
        const double t_first = fma((double)m0, rr.step, rr.t0), t_last = fma((double)mlast, rr.step, rr.t0);
        // the slice, clipped to the row and (it fits by rs_geometry's count) to what the LDS holds
        const int64_t lo = rs_max((int64_t)floor(t_first - rr.hw) + 1, 0);
        const int64_t hi = rs_min(rs_min((int64_t)ceil(t_last + rr.hw) - 1, (int64_t)rr.len - 1), lo + a.cap - 1);
        const int count = hi >= lo ? (int)(hi - lo + 1) : 0;
        __syncthreads();  // the table is in place; the slice of the row before has been read
        for (int i = tid; i < count; i += RS_THREADS) {
            const int64_t n = lo + i;
            double whole, rest;
            mul_split(rr.nu, (double)n, &whole, &rest);
            s_x[i] = cmulf(xr[n], unit_f32(frac_turn(-rest)));
        }
        __syncthreads();
        for (int64_t m = m0 + tid; m < m1; m += RS_THREADS) {
            float2 acc = make_float2(0.f, 0.f);
            if (m < rr.count) {
                const double t = fma((double)m, rr.step, rr.t0);
                const int64_t na = rs_max((int64_t)floor(t - rr.hw) + 1, lo);
                const int64_t nb = rs_min((int64_t)ceil(t + rr.hw) - 1, hi);
                for (int64_t n = na; n <= nb; ++n) {
                    double q = fma(t - (double)n, rr.r, hq);
                    q = fmin(fmax(q, 0.0), top);
                    const int i = min((int)q, last);
                    const float f = (float)(q - (double)i);
                    const float p0 = s_p[i], p1 = s_p[i + 1];
                    const float h = fmaf(f, p1 - p0, p0);
                    const float2 z = s_x[(int)(n - lo)];
                    acc.x = fmaf(z.x, h, acc.x);
                    acc.y = fmaf(z.y, h, acc.y);
                }
                acc.x *= rr.inv_w;
                acc.y *= rr.inv_w;
            }
            yr[m] = acc;
        }
    }
}

bool rs_sizes_ok(int64_t H, int64_t Q, double max_step, double max_width) {
    return H >= 1 && H <= 16 && Q >= 2 && Q <= 1024 && H * Q <= 8192 && max_step >= 0.015625 && max_step <= 64.0 && max_width >= 1.0 &&
           max_width <= 64.0;
}
constexpr const char* RS_SIZES = "1 <= H <= 16, 2 <= Q <= 1024, H Q <= 8192, 2^-6 <= step <= 64, 1 <= width <= 64";

// the largest tile whose table and slice fit the LDS; the slice of T outputs spans (T - 1) step + 2 H w samples and a margin for
// the roundings of its ends
void rs_geometry(int H, int Q, double max_step, double max_width, int* tile, int64_t* cap, int64_t* lds) {
    const int64_t table = (((int64_t)2 * H * Q + 1 + 3) & ~(int64_t)3) * 4;
    for (int T = RS_MAX_TILE;; T /= 2) {
        const int64_t c = (int64_t)std::floor((T - 1) * max_step + 2.0 * H * max_width) + 4;
        if (table + c * 8 <= RS_LDS || T == 1) {
            *tile = T, *cap = c, *lds = table + c * 8;
            return;
        }
    }
}

int rs_support(int H, double max_width) { return (int)std::floor(2.0 * H * max_width) + 1; }

// CAF_RESAMPLE_DEBUG=1 (read per call, like CAF_SCF_DEBUG): one stderr line per caf_resample_rows call
bool rs_debug() {
    const char* e = std::getenv("CAF_RESAMPLE_DEBUG");
    return e && e[0] == '1';
}

}  // namespace

}  // namespace caf

using namespace caf;

int32_t caf_resample_geometry(int32_t half_width, int32_t phases, double max_step, double max_width, int32_t* tile, int32_t* threads,
                              int64_t* lds_bytes) {
    CAF_REQUIRE(rs_sizes_ok(half_width, phases, max_step, max_width), std::string("caf_resample_geometry: ") + RS_SIZES);
    int T = 0;
    int64_t cap = 0, lds = 0;
    rs_geometry(half_width, phases, max_step, max_width, &T, &cap, &lds);
    if (tile) *tile = T;
    if (threads) *threads = RS_THREADS;
    if (lds_bytes) *lds_bytes = lds;
    return CAF_OK;
}

int32_t caf_resample_rows(const caf_resample_desc* desc) {
    CAF_REQUIRE(desc, "caf_resample_rows: NULL descriptor");
    const int64_t rows = desc->rows, H = desc->half_width, Q = desc->phases;
    CAF_REQUIRE(desc->d_x && desc->d_table && desc->d_y, "caf_resample_rows: d_x, d_table and d_y are required");
    CAF_REQUIRE(desc->h_nu && desc->h_t0 && desc->h_step && desc->h_width && desc->h_counts,
                "caf_resample_rows: h_nu, h_t0, h_step, h_width and h_counts are required (host arrays of `rows` entries)");
    CAF_REQUIRE(rows >= 1 && rows < ((int64_t)1 << 31), "caf_resample_rows: 1 <= rows < 2^31");
    CAF_REQUIRE(desc->pitch >= 1 && desc->pitch < ((int64_t)1 << 31), "caf_resample_rows: 1 <= pitch < 2^31");
    CAF_REQUIRE(desc->out_pitch >= 1 && desc->out_pitch < ((int64_t)1 << 31), "caf_resample_rows: 1 <= out_pitch < 2^31");
    CAF_REQUIRE(rs_sizes_ok(H, Q, 1.0, 1.0), std::string("caf_resample_rows: ") + RS_SIZES);
    double max_step = 0.0, max_width = 0.0;
    for (int64_t r = 0; r < rows; ++r) {
        const double nu = desc->h_nu[r], t0 = desc->h_t0[r], step = desc->h_step[r], w = desc->h_width[r];
        const int64_t len = desc->h_lengths ? desc->h_lengths[r] : desc->pitch, cnt = desc->h_counts[r];
        const std::string at = " (row " + std::to_string(r) + ")";
        CAF_REQUIRE(step >= 0.015625 && step <= 64.0 && w >= 1.0 && w <= 64.0, std::string("caf_resample_rows: ") + RS_SIZES + at);
        CAF_REQUIRE(std::fabs(nu) <= 1048576.0, "caf_resample_rows: |nu| <= 2^20 cycles per sample" + at);
        CAF_REQUIRE(std::fabs(t0) < 2147483648.0, "caf_resample_rows: |t0| < 2^31" + at);
        CAF_REQUIRE(len >= 0 && len <= desc->pitch, "caf_resample_rows: 0 <= length <= pitch" + at);
        CAF_REQUIRE(cnt >= 0 && cnt <= desc->out_pitch, "caf_resample_rows: 0 <= count <= out_pitch" + at);
        max_step = std::max(max_step, step), max_width = std::max(max_width, w);
    }
    hipStream_t st = (hipStream_t)desc->stream;
    int T = 0;
    int64_t cap = 0, lds = 0;
    rs_geometry((int)H, (int)Q, max_step, max_width, &T, &cap, &lds);

    int dev = 0;
    CAF_HIP_TRY(hipGetDevice(&dev));
    if (const int rc = allow_dynamic_lds(reinterpret_cast<const void*>(k_resample), (size_t)lds)) return rc;
    const int64_t bytes = rows * (int64_t)sizeof(RsRow);
    Lane* lane = nullptr;
    if (const int rc = lane_acquire("caf_resample_rows", dev, bytes, &lane)) return rc;
    RsRow* h = (RsRow*)lane->pinned;
    for (int64_t r = 0; r < rows; ++r) {
        const double w = desc->h_width[r];
        RsRow& o = h[r];
        o.nu = desc->h_nu[r], o.t0 = desc->h_t0[r], o.step = desc->h_step[r];
        o.r = (double)Q / w, o.hw = (double)H * w, o.inv_w = (float)(1.0 / w);
        o.len = desc->h_lengths ? desc->h_lengths[r] : (int32_t)desc->pitch, o.count = desc->h_counts[r], o.pad = 0;
    }
    void* d_rows = nullptr;
    if (const int rc = pool_alloc(&d_rows, bytes, st == nullptr)) {
        lane_abandon(lane, nullptr, st);
        return rc;
    }
    RsArgs a{};
    a.x = (const float2*)desc->d_x, a.pitch = desc->pitch, a.rows = rows, a.row = (const RsRow*)d_rows, a.table = desc->d_table;
    a.H = (int32_t)H, a.Q = (int32_t)Q, a.tile = T, a.cap = (int32_t)cap, a.y = (float2*)desc->d_y, a.out_pitch = desc->out_pitch;
    hipError_t e = hipMemcpyAsync(d_rows, h, (size_t)bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_resample, dim3(cdiv(desc->out_pitch, T), (unsigned)std::min<int64_t>(rows, 65535)), dim3(RS_THREADS),
                           (size_t)lds, st, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(lane->ev, st);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        lane_abandon(lane, d_rows, st);
        set_error(std::string("caf_resample_rows: ") + hipGetErrorString(e));
        return CAF_ERR_HIP;
    }
    lane_in_flight(lane, d_rows);
    if (rs_debug())
        std::fprintf(stderr, "[caf resample] rows=%lld tile=%d threads=%d lds=%lld support=%d\n", (long long)rows, T, RS_THREADS,
                     (long long)lds, rs_support((int)H, max_width));
    return CAF_OK;
}
