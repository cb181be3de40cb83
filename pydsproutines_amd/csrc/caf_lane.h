// Host arrays of a call on their way to the device and back to the pool in stream order (caf_resample.hip: the rows' records;
// caf_dpd.hip: the maps and the arg max partials).  A lane is a pinned staging block, an event and the pooled device block of the
// call in flight.  The call fills the pinned block, copies it with hipMemcpyAsync into the device block on its stream, launches,
// records the event and returns.  Both blocks stay with their lane until that event has completed -- asked, never waited for, by
// the calls that follow -- and only then does the device block go back to the pool: no synchronisation on either the null stream
// or a caller's.  Everything is in the anonymous namespace: each includer keeps its own lanes.
#pragma once

#include <mutex>
#include <string>
#include <vector>

#include "caf_internal.h"

namespace caf {

namespace {

constexpr int LANE_MAX = 32;  // calls in flight per device before one waits for the oldest

struct Lane {
    int dev = 0;
    void* pinned = nullptr;
    int64_t cap = 0;
    hipEvent_t ev = nullptr;
    void* d_block = nullptr;  // the pooled block of the call in flight
    bool busy = false;
};
std::mutex g_lane_mu;
std::vector<Lane*> g_lanes;  // (kept for the life of the process)

// caller holds g_lane_mu: a lane whose event has completed gives its device block back and is idle again
void lane_settle(Lane* l, bool wait) {
    if (!l->busy || !l->d_block) return;
    if (wait) {
        (void)hipEventSynchronize(l->ev);
    } else if (hipEventQuery(l->ev) != hipSuccess) {
        (void)hipGetLastError();  // (hipErrorNotReady is the answer, not a failure)
        return;
    }
    (void)pool_free(l->d_block);
    l->d_block = nullptr;
    l->busy = false;
}

// an idle lane of `dev` whose pinned block holds `bytes`; failures are worded under `entry`
int lane_acquire(const char* entry, int dev, int64_t bytes, Lane** out) {
    std::lock_guard<std::mutex> lk(g_lane_mu);
    Lane* idle = nullptr;
    int mine = 0;
    for (Lane* l : g_lanes) {
        if (l->dev != dev) continue;
        ++mine;
        lane_settle(l, false);
        if (!l->busy && (!idle || (idle->cap < bytes && l->cap > idle->cap))) idle = l;
    }
    if (!idle && mine >= LANE_MAX) {  // that many calls in flight: wait for the oldest
        for (Lane* l : g_lanes)
            if (l->dev == dev && l->d_block) {
                lane_settle(l, true);
                idle = l;
                break;
            }
    }
    if (!idle) {
        idle = new Lane;
        idle->dev = dev;
        if (hipEventCreateWithFlags(&idle->ev, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            delete idle;
            set_error(std::string(entry) + ": hipEventCreate failed");
            return CAF_ERR_HIP;
        }
        g_lanes.push_back(idle);
    }
    if (idle->cap < bytes) {
        if (idle->pinned) (void)hipHostFree(idle->pinned);
        idle->pinned = nullptr, idle->cap = 0;
        int64_t c = 4096;
        while (c < bytes) c *= 2;
        const hipError_t e = hipHostMalloc(&idle->pinned, (size_t)c, hipHostMallocDefault);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            idle->pinned = nullptr;
            set_error(std::string(entry) + ": hipHostMalloc: " + hipGetErrorString(e));
            return CAF_ERR_NOMEM;
        }
        idle->cap = c;
    }
    idle->busy = true;  // (taken: no other thread fills it; d_block is set once the block exists)
    *out = idle;
    return CAF_OK;
}

// the call failed before its event was recorded: nothing of it may still run when the blocks go back
void lane_abandon(Lane* l, void* d_block, hipStream_t st) {
    (void)hipStreamSynchronize(st);
    (void)hipGetLastError();
    if (d_block) (void)pool_free(d_block);
    std::lock_guard<std::mutex> lk(g_lane_mu);
    l->busy = false;
}

// the event is on the stream: from here on the lane settles by it
void lane_in_flight(Lane* l, void* d_block) {
    std::lock_guard<std::mutex> lk(g_lane_mu);
    l->d_block = d_block;
}

}  // namespace

}  // namespace caf
