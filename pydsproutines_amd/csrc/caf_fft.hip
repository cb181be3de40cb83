// rocFFT plumbing shared by the hypothesis-engine plan and the kernel-level ops:
// batched 1-D complex64 transforms (in place or out of place) with an explicit batch distance.
#include <rocfft/rocfft.h>

#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "caf_internal.h"

namespace caf {

static std::once_flag g_rocfft_once;

#define CAF_FFT_TRY(expr)                                                                 \
    do {                                                                                  \
        rocfft_status _s = (expr);                                                        \
        if (_s != rocfft_status_success) {                                                \
            caf::set_error(std::string(#expr) + ": rocfft status " + std::to_string(_s)); \
            return CAF_ERR_ROCFFT;                                                        \
        }                                                                                 \
    } while (0)

int FftPlan::create(bool inverse, size_t len, size_t batch, size_t dist, bool inplace) {
    std::call_once(g_rocfft_once, [] { rocfft_setup(); });
    rocfft_plan_description desc = nullptr;
    CAF_FFT_TRY(rocfft_plan_description_create(&desc));
    size_t stride = 1;
    CAF_FFT_TRY(rocfft_plan_description_set_data_layout(desc, rocfft_array_type_complex_interleaved,
                                                        rocfft_array_type_complex_interleaved, nullptr, nullptr, 1,
                                                        &stride, dist, 1, &stride, dist));
    rocfft_plan p = nullptr;
    rocfft_status s = rocfft_plan_create(&p, inplace ? rocfft_placement_inplace : rocfft_placement_notinplace,
                                         inverse ? rocfft_transform_type_complex_inverse
                                                 : rocfft_transform_type_complex_forward,
                                         rocfft_precision_single, 1, &len, batch, desc);
    rocfft_plan_description_destroy(desc);
    CAF_FFT_TRY(s);
    plan = p;
    CAF_FFT_TRY(rocfft_plan_get_work_buffer_size(p, &work_bytes));
    rocfft_execution_info ei = nullptr;
    CAF_FFT_TRY(rocfft_execution_info_create(&ei));
    info = ei;
    if (work_bytes) {
        CAF_HIP_TRY(hipMalloc(&work, work_bytes));
        CAF_FFT_TRY(rocfft_execution_info_set_work_buffer(ei, work, work_bytes));
    }
    return CAF_OK;
}

int FftPlan::exec(void* in, void* out, hipStream_t st) {
    if (last_use_pending) {  // the previous owner's last transform may still be using the work buffer
        CAF_HIP_TRY(hipStreamWaitEvent(st, last_use, 0));
        last_use_pending = false;
    }
    CAF_FFT_TRY(rocfft_execution_info_set_stream((rocfft_execution_info)info, st));
    void* ib[1] = {in};
    void* ob[1] = {out};
    CAF_FFT_TRY(rocfft_execute((rocfft_plan)plan, ib, (out && out != in) ? ob : nullptr, (rocfft_execution_info)info));
    return CAF_OK;
}

void FftPlan::destroy() {
    if (last_use_pending) (void)hipEventSynchronize(last_use);
    if (info) rocfft_execution_info_destroy((rocfft_execution_info)info);
    if (plan) rocfft_plan_destroy((rocfft_plan)plan);
    if (work) (void)hipFree(work);  // (hipFree waits for the device: nothing is still using the buffer afterwards)
    if (last_use) (void)hipEventDestroy(last_use);
    *this = FftPlan();
}

// ---- checkout cache of rocFFT plans --------------------------------------------------------------------------
// rocfft_plan_create costs milliseconds (kernel selection / code-object loading), more than a small CAF job
// itself; the per-call entry points of the host layer (fastXcorr, cztXcorr, ...) build a CAF plan per call, and the
// kernel-level ops take a plan per chunk of rows.  Plans are therefore parked on release and handed out again for
// the same (device, direction, length, batch, distance, placement).
namespace {
struct FftKey {
    int dev, inverse, inplace;
    size_t len, batch, dist;
    bool operator<(const FftKey& o) const {
        return std::tie(dev, inverse, inplace, len, batch, dist) < std::tie(o.dev, o.inverse, o.inplace, o.len, o.batch, o.dist);
    }
};
// A plan keeps its slot while it is checked out (no node is allocated or freed per checkout); `parked` slots are the cache.
struct Slot {
    FftPlan plan;
    bool parked;
    uint64_t seq;  // when it was parked (larger = more recent)
};
std::mutex g_fft_mu;
std::multimap<FftKey, Slot> g_fft_slots;
uint64_t g_fft_seq = 0;
size_t g_fft_parked = 0, g_fft_parked_work = 0;
// Both bounds hold at once; the oldest parked plans go first (as in pool_free), and the plan that has just been released
// always stays, whatever its work size: a shape that is used call after call is never created twice.  96 plans: what the
// CAF plans' cache (32) and the ops' row-plan cache (64) kept between them before they were merged.
constexpr size_t FFT_PARK_MAX_PLANS = 96;
// Parked work buffers in all: the 32 x 64 MiB of the CAF plans' cache.  It covers the largest chunk the ops transform
// (2^27 elements): rocFFT reports work_bytes = 1 GiB for 2048 x 65536, 128 x 2^20 and 1 x 2^27 points in place (976.6 MiB
// for 128 x 1 000 000, 610 MiB for 8 x 10 000 000; none for 131072 x 1000).  A Bluestein length can need more on its own
// (1024 x 100 003: 4.0 GiB): that is what the rule above is for.
constexpr size_t FFT_PARK_MAX_WORK = (size_t)2 << 30;
}  // namespace

int fft_plan_acquire(FftPlan* out, bool inverse, size_t len, size_t batch, size_t dist, bool inplace) {
    int dev = 0;
    CAF_HIP_TRY(hipGetDevice(&dev));
    const FftKey k{dev, inverse ? 1 : 0, inplace ? 1 : 0, len, batch, dist};
    {
        std::lock_guard<std::mutex> lk(g_fft_mu);
        const auto range = g_fft_slots.equal_range(k);
        for (auto it = range.first; it != range.second; ++it)
            if (it->second.parked) {
                it->second.parked = false;
                *out = it->second.plan;
                --g_fft_parked;
                g_fft_parked_work -= out->work_bytes;
                return CAF_OK;
            }
    }
    *out = FftPlan();
    const int rc = out->create(inverse, len, batch, dist, inplace);
    if (rc) {
        out->destroy();
        return rc;
    }
    std::lock_guard<std::mutex> lk(g_fft_mu);
    out->slot = &g_fft_slots.emplace(k, Slot{FftPlan(), false, 0})->second;
    return CAF_OK;
}

void fft_plan_release(FftPlan* p, hipStream_t st) {
    if (!p->plan) return;
    if (st != nullptr && p->work) {
        if (!p->last_use && hipEventCreateWithFlags(&p->last_use, hipEventDisableTiming) != hipSuccess) p->last_use = nullptr;
        p->last_use_pending = p->last_use && hipEventRecord(p->last_use, st) == hipSuccess;
        if (!p->last_use_pending) (void)hipStreamSynchronize(st);  // (no event to be had: the plan is parked idle)
    }
    std::vector<FftPlan> evicted;  // (allocates nothing unless something is evicted)
    {
        std::lock_guard<std::mutex> lk(g_fft_mu);
        Slot* s = (Slot*)p->slot;
        s->plan = *p;
        s->parked = true;
        s->seq = ++g_fft_seq;
        ++g_fft_parked;
        g_fft_parked_work += p->work_bytes;
        *p = FftPlan();
        while (g_fft_parked > 1 && (g_fft_parked > FFT_PARK_MAX_PLANS || g_fft_parked_work > FFT_PARK_MAX_WORK)) {
            auto old = g_fft_slots.end();
            for (auto it = g_fft_slots.begin(); it != g_fft_slots.end(); ++it)
                if (it->second.parked && (old == g_fft_slots.end() || it->second.seq < old->second.seq)) old = it;
            --g_fft_parked;
            g_fft_parked_work -= old->second.plan.work_bytes;
            evicted.push_back(old->second.plan);
            g_fft_slots.erase(old);
        }
    }
    for (FftPlan& e : evicted) e.destroy();  // (outside the lock: hipFree waits for the device)
}

// rows FFT of a (rows, len) matrix, chunked so that the plan batch is bounded; a plan is checked out per chunk
int fft_rows(const float2* in, float2* out, int64_t rows, int64_t len, bool inverse, hipStream_t st) {
    const bool inplace = (out == in);
    for (int64_t done = 0; done < rows;) {
        // largest power-of-two chunk <= remaining keeps the number of distinct plans small
        int64_t chunk = 1;
        while (chunk * 2 <= rows - done && chunk * 2 * len <= ((int64_t)1 << 27)) chunk *= 2;
        FftPlan p;
        int rc = fft_plan_acquire(&p, inverse, (size_t)len, (size_t)chunk, (size_t)len, inplace);
        if (rc) return rc;
        rc = p.exec((void*)(in + done * len), inplace ? nullptr : (void*)(out + done * len), st);
        fft_plan_release(&p, st);
        if (rc) return rc;
        done += chunk;
    }
    return CAF_OK;
}

}  // namespace caf
