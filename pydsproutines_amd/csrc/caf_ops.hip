// libcaf C-ABI, part 2: the per-delay path, the batched chirp-Z transform and the CZT zoom (include/caf.h).  Host-side
// C++ that validates arguments, manages scratch and launches the gfx950 kernels of caf_rows.hip / caf_kernels.hip /
// caf_perdelay*.hip / caf_zoom.hip and batched rocFFT rows (caf_fft.hip).
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "caf_internal.h"

using namespace caf;

namespace {

// ---- chirp-Z constants of the zoom, computed like CZTCached / IppCZT32fc (spectralRoutines.py:239-267,
// CZT.cpp:89-140): float64 on the host, stored as complex64; W exponent = step (the labelled grid IS the evaluated
// grid), nfft = next 7-smooth length >= m + k - 1.  Cached per (device, m, span, step).
typedef std::complex<double> cd;
void host_fft(std::vector<cd>& a) {  // in-place forward DFT, length with prime factors <= 7 (recursive mixed radix)
    const size_t n = a.size();
    if (n <= 1) return;
    size_t p = 0;
    for (size_t q : {2, 3, 5, 7})
        if (n % q == 0) {
            p = q;
            break;
        }
    if (!p) {  // (not reached for 7-smooth lengths) plain DFT
        std::vector<cd> o(n);
        for (size_t k = 0; k < n; ++k) {
            cd acc = 0;
            for (size_t j = 0; j < n; ++j) acc += a[j] * std::polar(1.0, -2.0 * M_PI * (double)((j * k) % n) / (double)n);
            o[k] = acc;
        }
        a.swap(o);
        return;
    }
    const size_t m = n / p;
    std::vector<std::vector<cd>> sub(p, std::vector<cd>(m));
    for (size_t j = 0; j < n; ++j) sub[j % p][j / p] = a[j];
    for (auto& v : sub) host_fft(v);
    for (size_t k = 0; k < n; ++k) {
        cd acc = 0;
        for (size_t r = 0; r < p; ++r) acc += sub[r][k % m] * std::polar(1.0, -2.0 * M_PI * (double)((r * k) % n) / (double)n);
        a[k] = acc;
    }
}
int64_t next_fast_len7(int64_t n) {
    for (;; ++n) {
        int64_t v = n;
        for (int q : {2, 3, 5, 7})
            while (v % q == 0) v /= q;
        if (v == 1) return n;
    }
}
struct ZoomCzt {
    int nfft = 0, k = 0;
    float2 *aa = nullptr, *fv = nullptr, *wws = nullptr;  // device, never freed (a handful of small arrays per process)
};
std::mutex g_zoom_mu;
std::map<std::tuple<int, int, double, double>, ZoomCzt> g_zoom_czt;

int zoom_num_bins(double span, double step) { return (int)std::floor(2.0 * span / step + 1.0 + 1e-9); }

int zoom_constants(int dev, int m, double span, double step, ZoomCzt* out) {
    std::lock_guard<std::mutex> lk(g_zoom_mu);
    const auto key = std::make_tuple(dev, m, span, step);
    auto it = g_zoom_czt.find(key);
    if (it != g_zoom_czt.end()) {
        *out = it->second;
        return CAF_OK;
    }
    ZoomCzt z;
    z.k = zoom_num_bins(span, step);
    z.nfft = (int)next_fast_len7((int64_t)m + z.k - 1);
    const int k = z.k, nfft = z.nfft;
    const int lo = -m + 1, hi = std::max(k - 1, m - 1);
    std::vector<cd> ww(hi - lo + 1);
    for (int i = lo; i <= hi; ++i) {
        double cyc = step * ((double)i * (double)i / 2.0);
        cyc -= std::floor(cyc);
        ww[i - lo] = std::polar(1.0, -2.0 * M_PI * cyc);
    }
    std::vector<cd> fv(nfft, cd(0, 0));
    for (int i = 0; i < k - 1 + m; ++i) fv[i] = 1.0 / ww[i];
    host_fft(fv);
    std::vector<std::complex<float>> aa(m), fvf(nfft), wws(k);
    for (int n = 0; n < m; ++n) {
        double cyc = span * (double)n;  // exp(-2 pi j f1 n) with f1 = -span
        cyc -= std::floor(cyc);
        const cd v = std::polar(1.0, 2.0 * M_PI * cyc) * ww[m - 1 + n];
        aa[n] = std::complex<float>((float)v.real(), (float)v.imag());
    }
    for (int i = 0; i < nfft; ++i) fvf[i] = std::complex<float>((float)fv[i].real(), (float)fv[i].imag());
    for (int i = 0; i < k; ++i) wws[i] = std::complex<float>((float)ww[m - 1 + i].real(), (float)ww[m - 1 + i].imag());
    int rc;
    if ((rc = upload_table(aa.data(), (int64_t)m * 8, false, (void**)&z.aa)) ||
        (rc = upload_table(fvf.data(), (int64_t)nfft * 8, false, (void**)&z.fv)) ||
        (rc = upload_table(wws.data(), (int64_t)k * 8, false, (void**)&z.wws))) {
        (void)hipFree(z.aa);  // (the tables that did get uploaded; hipFree(nullptr) does nothing)
        (void)hipFree(z.fv);
        return rc;
    }
    if (g_zoom_czt.size() > 64) g_zoom_czt.clear();  // (leaks a few hundred KB at worst; bounded)
    g_zoom_czt[key] = z;
    *out = z;
    return CAF_OK;
}

}  // namespace

extern "C" {

int32_t caf_fft_rows(const float* d_in, float* d_out, int64_t rows, int64_t len, int32_t inverse, void* stream) {
    CAF_REQUIRE(d_in && d_out && rows >= 0 && len >= 1, "caf_fft_rows: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    int rc = fft_rows((const float2*)d_in, (float2*)d_out, rows, len, inverse != 0, st);
    if (rc) return rc;
    if (inverse) launch_scale((float2*)d_out, rows * len, 1.0f / (float)len, st);  // numpy/cupy ifft normalisation
    CAF_HIP_TRY(hipGetLastError());
    return CAF_OK;
}

int32_t caf_xcorr_perdelay_one_kernel(int32_t n) {
    return (perdelay_fused_ok(n) || perdelay_decimal_ok(n) || perdelay_mixed_ok(n) || perdelay_jit_ok(n)) ? 1 : 0;
}

int32_t caf_perdelay_jit_describe(int32_t n, const char* arch, const char* dump_path, char* buf, int32_t len) {
    CAF_REQUIRE(buf && len > 0, "caf_perdelay_jit_describe: no buffer");
    std::string text;
    const int rc = perdelay_jit_describe(n, arch, dump_path, &text);
    std::snprintf(buf, (size_t)len, "%s", text.c_str());
    return rc;
}

int32_t caf_xcorr_perdelay(const float* d_cutout, int32_t n, const float* d_rx, int64_t rx_len, int64_t start,
                           int64_t step, int64_t num, int32_t zero_oor, float* d_qf2, int32_t* d_fidx, float* d_caf,
                           float* d_ccaf, int64_t batch_rows, void* stream) {
    CAF_REQUIRE(d_cutout && d_rx && n >= 1 && rx_len >= 1 && num >= 0 && step != 0, "caf_xcorr_perdelay: bad arguments");
    if (!zero_oor) {
        const int64_t last = start + (num - 1) * step;
        const int64_t lo = std::min(start, last), hi = std::max(start, last);
        CAF_REQUIRE(num == 0 || (lo >= 0 && hi + n <= rx_len), "caf_xcorr_perdelay: delay window leaves rx");
    }
    if (num == 0) return CAF_OK;
    hipStream_t st = (hipStream_t)stream;
    // CAF_JIT_ALL=1 (measurements): every power of two and of ten through the run-time-compiled kernel as well.  By default those
    // where it measured faster than the prebuilt kernels, from the row count at which its per-call work (energy prefix, cutout
    // norm: ~25 us) is paid back (profiles/r05/timing_pow2_pow10_through_jit.log, ms per 1e5 delays): 10000 (2.0 against the
    // radix-10 kernel's 4.0), 16384 (3.1 / 3.8), 8192 (1.50 / 1.82), 2048 (0.29 / 0.32).
    const bool jit_all = [n, num] {
        const char* e = getenv("CAF_JIT_ALL");
        if (e) return atoi(e) != 0;
        return n == 10000 || ((n == 8192 || n == 16384) && num >= 8192) || (n == 2048 && num >= (1 << 17));
    }();
    // Power-of-two cutouts up to 16384 samples: one fused kernel (product -> LDS FFT -> |.|^2 -> argmax; window energies
    // and the cutout norm summed in the kernel): no product matrix, no prefix pass, no scratch, no synchronisation.
    // CAF_PERDELAY_UNFUSED=1 keeps the three-kernel form below (A/B switch; it also serves every other length).
    static const bool unfused = [] {
        const char* e = getenv("CAF_PERDELAY_UNFUSED");
        return e && atoi(e) != 0;
    }();
    if (!unfused && perdelay_fused_ok(n) && !(jit_all && perdelay_jit_ok(n))) {
        const int rc1 = launch_perdelay_fused((const float2*)d_cutout, n, (const float2*)d_rx, rx_len, start, step, num,
                                              zero_oor ? 1 : 0, d_qf2, (uint32_t*)d_fidx, d_caf, (float2*)d_ccaf, st);
        if (rc1) return rc1;
        CAF_HIP_TRY(hipGetLastError());
        return CAF_OK;
    }
    Scratch sc(st, true);
    // energy prefix over the span of rx the delays touch (not the whole array: 128 delays of a 10^7-sample rx used
    // to cost a full pass), indices shifted accordingly; only when every window lies inside rx (otherwise the
    // out-of-range rules are stated against the whole array and the whole array is scanned)
    const int64_t s_last = start + (num - 1) * step;
    const int64_t span_lo = std::max<int64_t>(0, std::min(start, s_last));
    const int64_t span_hi = std::min<int64_t>(rx_len, std::max(start, s_last) + n);
    const bool clip = span_hi > span_lo && (span_lo > 0 || span_hi < rx_len) && span_lo == std::min(start, s_last) &&
                      span_hi == std::max(start, s_last) + n;  // only when no window leaves rx
    const float2* yv = (const float2*)d_rx + (clip ? span_lo : 0);
    const int64_t ylen_v = clip ? span_hi - span_lo : rx_len;
    const int64_t start_v = clip ? start - span_lo : start;
    double* prefix = nullptr;
    int rc = energy_prefix(yv, ylen_v, sc, &prefix, st);
    if (rc) return rc;
    // ||cutout|| in float64 on the device (no host round trip)
    double* d_cnorm = nullptr;
    if ((rc = sc.get(&d_cnorm, cutout_norm_scratch_doubles()))) return rc;
    const double* d_norm = launch_cutout_norm((const float2*)d_cutout, n, d_cnorm, st);
    // cutouts of 100 / 1000 / 10000 samples: one fused kernel with radix-10 passes in LDS (CAF_PERDELAY_UNFUSED=1: the chain below)
    {
        // lengths with prime factors up to 23 that are neither a power of two nor of ten: a kernel compiled for the length at run
        // time (caf_jit.hip); a length / box without one, or a compilation that fails (reported once), keeps the plan-driven
        // kernel (7-smooth lengths) or the three-kernel form below
        if (!unfused && (jit_all || !(perdelay_fused_ok(n) || perdelay_decimal_ok(n))) && perdelay_jit_ok(n)) {
            rc = launch_perdelay_jit((const float2*)d_cutout, n, yv, ylen_v, prefix, d_norm, start_v, step, num, zero_oor ? 1 : 0, d_qf2,
                                     (uint32_t*)d_fidx, d_caf, (float2*)d_ccaf, st);
            if (rc == CAF_OK) return sc.finish();
            perdelay_jit_failed(n);
            static bool said = false;
            if (!said) {
                said = true;
                char msg[2048];
                caf_last_error(msg, sizeof(msg));
                std::fprintf(stderr, "[caf] run-time compilation unavailable, using the prebuilt per-delay kernels: %s\n", msg);
            }
        }
        if (!unfused && (perdelay_decimal_ok(n) || perdelay_mixed_ok(n))) {
            // (the radix-10 kernel of caf_perdelay.hip / the plan-driven mixed-radix kernel of caf_perdelay_mr.hip)
            rc = perdelay_decimal_ok(n)
                     ? launch_perdelay_decimal((const float2*)d_cutout, n, yv, ylen_v, prefix, d_norm, start_v, step, num,
                                               zero_oor ? 1 : 0, d_qf2, (uint32_t*)d_fidx, d_caf, (float2*)d_ccaf, st)
                     : launch_perdelay_mixed((const float2*)d_cutout, n, yv, ylen_v, prefix, d_norm, start_v, step, num,
                                             zero_oor ? 1 : 0, d_qf2, (uint32_t*)d_fidx, d_caf, (float2*)d_ccaf, st);
            if (rc) return rc;
            return sc.finish();
        }
    }
    // rows per batch: up to 2^28 product elements (2 GiB of the 288) in flight, so that even 1e7-sample cutouts go
    // through rocFFT and the argmax a few dozen rows at a time
    if (batch_rows <= 0) batch_rows = std::max<int64_t>(1, std::min<int64_t>(num, ((int64_t)1 << 28) / n));
    batch_rows = std::min(batch_rows, num);
    float2* rows = nullptr;
    float2* direct = (float2*)d_ccaf;  // when the complex plane is wanted, build it in place
    if (!direct && (rc = sc.get(&rows, batch_rows * n))) return rc;
    unsigned long long* part = nullptr;  // long rows: chunked argmax
    if (const int ch = rows_argmax_chunks(batch_rows, n))
        if ((rc = sc.get(&part, batch_rows * ch))) return rc;
    for (int64_t r0 = 0; r0 < num; r0 += batch_rows) {
        const int64_t nr = std::min(batch_rows, num - r0);
        float2* buf = direct ? direct + r0 * n : rows;
        launch_sliding_multiply((const float2*)d_cutout, n, yv, ylen_v, prefix, start_v + r0 * step, step, nr, 1.0,
                                zero_oor ? 1 : 0, buf, st, d_norm);
        if ((rc = fft_rows(buf, buf, nr, n, false, st))) return rc;
        if (d_qf2 || d_fidx || d_caf)
            launch_rows_argmax(buf, nr, n, 1, 1.0f, (uint32_t*)(d_fidx ? d_fidx + r0 : nullptr), d_qf2 ? d_qf2 + r0 : nullptr,
                               d_caf ? d_caf + r0 * n : nullptr, st, part, 1);
    }
    return sc.finish();
}

int32_t caf_czt_run_many(const float* d_x, int64_t rows, int32_t m, int32_t k, int32_t nfft, const float* d_aa,
                         const float* d_fv, const float* d_ww, float* d_out, void* stream) {
    CAF_REQUIRE(d_x && d_aa && d_fv && d_ww && d_out, "caf_czt_run_many: NULL");
    CAF_REQUIRE(rows >= 0 && m >= 1 && k >= 1 && nfft >= m + k - 1, "caf_czt_run_many: need nfft >= m + k - 1");
    if (rows == 0) return CAF_OK;
    hipStream_t st = (hipStream_t)stream;
    Scratch sc(st, true);
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(rows, ((int64_t)1 << 25) / nfft));
    float2* buf = nullptr;
    int rc = sc.get(&buf, chunk * nfft);
    if (rc) return rc;
    for (int64_t r0 = 0; r0 < rows; r0 += chunk) {
        const int64_t nr = std::min(chunk, rows - r0);
        // y = x * aa, zero-padded to nfft
        launch_rows_mul_vec((const float2*)d_x + r0 * m, m, 0, (const float2*)d_aa, m, buf, nfft, nfft, nr, 1.0f, st);
        if ((rc = fft_rows(buf, buf, nr, nfft, false, st))) return rc;
        launch_rows_mul_vec(buf, nfft, 0, (const float2*)d_fv, nfft, buf, nfft, nfft, nr, 1.0f, st);
        if ((rc = fft_rows(buf, buf, nr, nfft, true, st))) return rc;
        // g[m-1 : m+k-1] * ww / nfft
        launch_rows_mul_vec(buf, nfft, m - 1, (const float2*)d_ww, k, (float2*)d_out + r0 * k, k, k, nr,
                            1.0f / (float)nfft, st);
    }
    return sc.finish();
}

int32_t caf_zoom_num_bins(double span, double step, int32_t* num_bins) {
    CAF_REQUIRE(num_bins && span > 0.0 && step > 0.0 && span / step < 1e6, "caf_zoom_num_bins: bad span/step");
    *num_bins = zoom_num_bins(span, step);
    return CAF_OK;
}

int32_t caf_zoom_czt(caf_plan plan, int32_t template_index, const float* d_rx, int64_t rx_len, const float* d_row_max,
                     const int32_t* d_row_arg, int64_t shift_start, int64_t num_shifts, int32_t k, float min_height,
                     double span, double step, const caf_zoom_outputs* out, void* stream) {
    CAF_REQUIRE(plan && d_rx && d_row_max && d_row_arg && out, "caf_zoom_czt: NULL argument");
    PlanZoomView v;
    int rc = plan_zoom_view(plan, &v);
    if (rc) return rc;
    CAF_REQUIRE(template_index >= 0 && template_index < v.T, "caf_zoom_czt: template_index outside the plan");
    CAF_REQUIRE(v.G == 1, "caf_zoom_czt: composite (multi-group) templates are not supported");
    CAF_REQUIRE(k >= 1 && k <= 4096, "caf_zoom_czt: need 1 <= k <= 4096");
    CAF_REQUIRE(span > 0.0 && step > 0.0 && span / step < 1e5, "caf_zoom_czt: bad span/step");
    CAF_REQUIRE(shift_start >= 0 && num_shifts >= 1 && shift_start + num_shifts - 1 + v.N <= rx_len,
                "caf_zoom_czt: delays run past the end of rx");
    CAF_REQUIRE(num_shifts < ((int64_t)1 << 31), "caf_zoom_czt: trace too long");
    int cur = -1;
    CAF_HIP_TRY(hipGetDevice(&cur));
    CAF_REQUIRE(cur == v.device, "caf_zoom_czt: the plan was created on another device than the current one");
    hipStream_t st = (hipStream_t)stream;
    ZoomCzt z;
    if ((rc = zoom_constants(v.device, v.N, span, step, &z))) return rc;
    Scratch sc(st);
    const int32_t max_cand = (int32_t)std::min<int64_t>(num_shifts, (int64_t)1 << 20);
    int32_t *tiles = nullptr, *cand = nullptr, *cnt = nullptr, *sel = nullptr, *selcnt = nullptr;
    float *vals = nullptr, *fmax = nullptr;
    uint32_t* farg = nullptr;
    float2 *rows = nullptr, *zk = nullptr;
    if ((rc = sc.get(&tiles, local_maxima_scratch_ints(num_shifts))) || (rc = sc.get(&cand, max_cand)) ||
        (rc = sc.get(&cnt, 1)) || (rc = sc.get(&sel, k)) || (rc = sc.get(&selcnt, 1)) || (rc = sc.get(&vals, max_cand)) ||
        (rc = sc.get(&fmax, k)) || (rc = sc.get(&farg, k)) || (rc = sc.get(&rows, (int64_t)k * z.nfft)) ||
        (rc = sc.get(&zk, (int64_t)k * z.k)))
        return rc;
    // 1. local maxima above min_height (peakfinding.cu:52 predicate), ascending index order, count on the device
    launch_find_local_maxima(d_row_max, num_shifts, min_height, tiles, max_cand, cand, cnt, st);
    // 2. the k strongest: value descending, index ascending
    launch_zoom_topk(d_row_max, cand, cnt, max_cand, k, vals, sel, selcnt, st);
    // 3. all product rows in one launch, already rotated, pre-chirped and padded
    launch_zoom_rows((const float2*)d_rx, v.d_uconj + (int64_t)template_index * v.N, v.N, v.d_tscale + template_index, d_row_arg,
                     v.d_nu, z.aa, sel, selcnt, k, shift_start, z.nfft, rows, st);
    // 4. one batched Bluestein transform
    if ((rc = fft_rows(rows, rows, k, z.nfft, false, st))) return rc;
    launch_rows_mul_vec(rows, z.nfft, 0, z.fv, z.nfft, rows, z.nfft, z.nfft, k, 1.0f, st);
    if ((rc = fft_rows(rows, rows, k, z.nfft, true, st))) return rc;
    launch_rows_mul_vec(rows, z.nfft, v.N - 1, z.wws, z.k, zk, z.k, z.k, k, 1.0f / (float)z.nfft, st);
    // 5. |.|^2, fine argmax (first index), optional planes
    launch_rows_argmax(zk, k, z.k, 1, 1.0f, farg, fmax, out->d_planes, st);
    launch_zoom_finish(d_row_max, d_row_arg, v.d_nu, sel, selcnt, k, shift_start, span, step, farg, fmax, max_cand, cnt,
                       out->d_count, out->d_delay, out->d_coarse_freq_index, out->d_coarse_qf2, out->d_fine_index,
                       out->d_fine_freq, out->d_fine_qf2, st);
    return sc.finish();
}

}  // extern "C"
