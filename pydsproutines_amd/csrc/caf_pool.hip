// Caching device allocator behind caf_malloc / caf_free and the library's own scratch buffers.
//
// The reference leans on cupy's memory pool: every cp.empty / cp.zeros inside its wrappers is a pool hit, not a
// cudaMalloc.  hipMalloc + hipFree cost 100-300 us per pair and hipFree synchronises the device, which is more than
// most of the kernel-level entry points take, so freed blocks are kept per (device, rounded size) and handed out
// again.  A block may be freed while work on the NULL stream still uses it (the host layer and null-stream scratch do
// that); work on any other stream has to be drained by whoever frees (Scratch::finish, _lib.held).  So pool_free looks
// at the null stream: if it is busy, the block is kept as pending.  Until an event recorded on that stream after the free
// has completed (Marks, below) the block goes only to a user that says it is ordered behind the null stream (null-stream Scratch); every other
// pool_alloc -- caf_malloc, scratch on a caller's stream, plan buffers: their next use may sit on a non-blocking stream or
// a staging lane, which nothing on the null stream is ordered with -- passes it over and takes another block or misses.
//
//   CAF_POOL_MB       upper bound of cached (free) bytes per process, default 8192; 0 disables caching.
//   CAF_POOL_POISON   diagnostic, read on every pool_alloc: a 32-bit word in hex (unset, empty or 0 = off).  When on, the
//                     whole rounded block is filled with the word before pool_alloc returns, on a pool hit and on a fresh
//                     hipMalloc alike, between two device synchronisations (so for users on any stream).  A kernel that
//                     reads scratch before writing it, or leaves part of an output unwritten, then shows the word instead
//                     of what the block's previous user left there (tests/test_gpu_pool_poison.py).
#include <cstdlib>
#include <map>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "caf_internal.h"

namespace caf {
namespace {

struct Live {
    int64_t bytes;
    int dev;
};

std::mutex g_mu;
struct Cached {
    void* p;
    uint64_t seq;  // when it was freed (larger = more recent)
    bool pending;  // freed while the null stream was busy: see Marks
};
// What is known of the null stream of one device.  Every block freed with seq <= settled is free of null-stream work.  A
// block freed later while that stream was busy waits for an event recorded there after its free.  No event is recorded at the
// free (every event is a packet on the stream it guards, and most blocks are never asked for by another stream's user): the
// first pool_alloc that is refused a pending block records ONE event for everything freed so far, and the blocks settle
// together once it has completed.  At most one event is in flight per device.
struct Marks {
    uint64_t settled = 0, covers = 0;  // covers: g_seq when the event in flight was recorded
    hipEvent_t ev = nullptr;
    bool in_flight = false;
};
constexpr int kMarkedDevices = 16;  // (beyond that a free under a busy null stream waits for the stream instead)
Marks g_marks[kMarkedDevices];
std::multimap<std::pair<int, int64_t>, Cached> g_free;  // (device, rounded bytes) -> block
uint64_t g_seq = 0;
std::unordered_map<void*, Live> g_live;                // blocks handed out
int64_t g_cached = 0, g_in_use = 0, g_hits = 0, g_misses = 0;

int64_t pool_limit() {
    static const int64_t lim = [] {
        const char* e = std::getenv("CAF_POOL_MB");
        const int64_t mb = e ? std::atoll(e) : 8192;
        return (mb < 0 ? 0 : mb) << 20;
    }();
    return lim;
}

// <= 1 MiB: next power of two (>= 512 B); above: next multiple of 1 MiB
int64_t round_size(int64_t bytes) {
    if (bytes <= 512) return 512;
    if (bytes <= ((int64_t)1 << 20)) {
        int64_t r = 512;
        while (r < bytes) r <<= 1;
        return r;
    }
    return (bytes + ((int64_t)1 << 20) - 1) & ~(((int64_t)1 << 20) - 1);
}

// CAF_POOL_POISON as a word; 0 = off
uint32_t poison_word() {
    const char* e = std::getenv("CAF_POOL_POISON");
    return e && *e ? (uint32_t)std::strtoul(e, nullptr, 16) : 0u;
}

// caller holds g_mu and `dev` is current; whether a block of `dev` freed at `seq` while the null stream was busy is free of that work
bool settled(int dev, uint64_t seq) {
    Marks& m = g_marks[dev];
    if (seq <= m.settled) return true;
    if (m.in_flight) {
        if (hipEventQuery(m.ev) != hipSuccess) {
            (void)hipGetLastError();  // (hipErrorNotReady is the answer, not a failure)
            return false;
        }
        m.in_flight = false;
        if (m.covers > m.settled) m.settled = m.covers;
        if (seq <= m.settled) return true;
    }
    // nothing in flight covers this block: one event for everything freed so far
    if (!m.ev && hipEventCreateWithFlags(&m.ev, hipEventDisableTiming) != hipSuccess) m.ev = nullptr;
    if (m.ev && hipEventRecord(m.ev, nullptr) == hipSuccess) {
        m.in_flight = true;
        m.covers = g_seq;
    } else {
        (void)hipGetLastError();
    }
    return false;
}

// caller holds g_mu; hipFree of every cached block of `dev` (or of all devices when dev < 0)
void trim_locked(int dev) {
    for (auto it = g_free.begin(); it != g_free.end();) {
        if (dev < 0 || it->first.first == dev) {
            (void)hipFree(it->second.p);
            g_cached -= it->first.second;
            it = g_free.erase(it);
        } else {
            ++it;
        }
    }
}

}  // namespace

int pool_alloc(void** out, int64_t bytes, bool behind_null_stream) {
    int dev = 0;
    CAF_HIP_TRY(hipGetDevice(&dev));
    const int64_t r = round_size(bytes);
    const uint32_t poison = poison_word();
    if (poison) CAF_HIP_TRY(hipDeviceSynchronize());  // the block's previous user may still run, on whatever stream
    std::lock_guard<std::mutex> lk(g_mu);
    auto range = g_free.equal_range({dev, r});
    auto it = g_free.end();
    // Blocks of one size lie in the order they were freed, and a block settles no later than one freed after it, so only the
    // first is looked at: one hipEventQuery per call at the most, however many blocks wait.
    if (range.first != range.second) {
        const Cached& c = range.first->second;
        // (a poisoned pool has just waited for the device: nothing is pending any more)
        if (behind_null_stream || !c.pending || poison || settled(dev, c.seq)) it = range.first;
    }
    void* p = nullptr;
    if (it != g_free.end()) {
        p = it->second.p;
        g_free.erase(it);
        g_cached -= r;
        ++g_hits;
    } else {
        ++g_misses;
        hipError_t e = hipMalloc(&p, (size_t)r);
        if (e == hipErrorOutOfMemory) {  // give the cache back to the driver and try once more
            (void)hipGetLastError();
            trim_locked(dev);
            e = hipMalloc(&p, (size_t)r);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error(std::string("hipMalloc(") + std::to_string(r) + " bytes): " + hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? CAF_ERR_NOMEM : CAF_ERR_HIP;
        }
    }
    g_live[p] = Live{r, dev};
    g_in_use += r;
    *out = p;
    if (const uint32_t w = poison) {  // (r is a multiple of 512)
        CAF_HIP_TRY(hipMemsetD32((hipDeviceptr_t)p, (int)w, (size_t)(r / 4)));
        CAF_HIP_TRY(hipDeviceSynchronize());
    }
    return CAF_OK;
}

int pool_free(void* p) {
    if (!p) return CAF_OK;
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_live.find(p);
    if (it == g_live.end()) {  // not ours (allocated before the pool existed / by the caller): plain free
        CAF_HIP_TRY(hipFree(p));
        return CAF_OK;
    }
    const Live l = it->second;
    g_live.erase(it);
    g_in_use -= l.bytes;
    if (l.bytes > pool_limit()) {  // (larger than the whole cache: straight back to the driver)
        CAF_HIP_TRY(hipFree(p));
        return CAF_OK;
    }
    // A full cache gives up its OLDEST blocks for the one that has just been in use -- kept the other way round (the new block
    // dropped), a process whose cache had filled with sizes it no longer asks for paid a hipMalloc + hipFree pair (10-20 ms
    // each at 160 MB, and a device synchronisation) for every scratch buffer of every later call.
    while (g_cached + l.bytes > pool_limit() && !g_free.empty()) {
        auto old = g_free.begin();
        for (auto it = g_free.begin(); it != g_free.end(); ++it)
            if (it->second.seq < old->second.seq) old = it;
        (void)hipFree(old->second.p);
        g_cached -= old->first.second;
        g_free.erase(old);
    }
    int cur = l.dev;
    (void)hipGetDevice(&cur);
    if (cur != l.dev) (void)hipSetDevice(l.dev);  // (the null stream asked is the one of the block's device)
    bool pending = false;
    if (hipStreamQuery(nullptr) == hipSuccess) {  // idle: this block and every block of the device freed before it are settled
        if (l.dev >= 0 && l.dev < kMarkedDevices) g_marks[l.dev].settled = g_seq + 1;
    } else {
        (void)hipGetLastError();  // (hipErrorNotReady is the answer, not a failure)
        if (l.dev >= 0 && l.dev < kMarkedDevices) pending = true;
        else (void)hipStreamSynchronize(nullptr);
    }
    if (cur != l.dev) (void)hipSetDevice(cur);
    g_free.emplace(std::make_pair(l.dev, l.bytes), Cached{p, ++g_seq, pending});
    g_cached += l.bytes;
    return CAF_OK;
}

void pool_trim() {
    std::lock_guard<std::mutex> lk(g_mu);
    trim_locked(-1);
}

void pool_stats(int64_t* cached, int64_t* in_use, int64_t* hits, int64_t* misses) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (cached) *cached = g_cached;
    if (in_use) *in_use = g_in_use;
    if (hits) *hits = g_hits;
    if (misses) *misses = g_misses;
}

}  // namespace caf
