// ---- Replay of launch-bound calls.  A small network (config 1: 19 GNN_simple layers over 32 SBM-50 graphs)
// enqueues ~200 kernels of 3-10 us each per step, and the host's enqueue (~2 ms) is the step.  Such a call,
// met a third time with the same configuration and the same device pointers (a training loop: the same input
// tensors, the caching allocator's same workspace / output / gradient blocks), is captured once on a private
// stream into a HIP graph and from then on replayed with one hipGraphLaunch on the caller's stream.  The
// enqueue reads nothing from the host but the configuration and the pointers (no host synchronisation, no
// data-dependent launch), so the replay runs the same kernels on the same buffers.  Not for the headline
// shapes: their kernels outlast the enqueue, and a replayed graph runs the side stream's branch serially
// (DESIGN.md §8 round 3).  HGNN_EXEC_GRAPH=0 never, =1 always, unset: calls of <= 4096 node rows.  Calls
// inside a caller's capture, timed calls and calls with per-layer DP events enqueue as before.
#pragma once

#include <utility>
#include <vector>

#include "kernels.h"

namespace hgnn {

struct ReplayEntry {
    std::vector<uintptr_t> key;
    int seen = 0;
    bool failed = false;
    hipGraphExec_t exec = nullptr;
    hipEvent_t done = nullptr;  // recorded on the caller's stream after each launch of exec
    unsigned long long last = 0;
};

struct ReplayCache {
    std::vector<ReplayEntry> e;
    unsigned long long tick = 0;
    int dev = -1;
    hipStream_t cap = nullptr;
};
// entries per cache: a step is two (its forward and its backward)
constexpr size_t REPLAY_MAX = 32;

// The calling thread's cache, on the device of stream s (entries of another device are released first)
int replay_cache(hipStream_t s, ReplayCache** out);
// Destroy an entry's executable graph once its last launch has finished: a wait on that launch's
// event, not a device-wide synchronisation (which would also wait for other streams, e.g. the DP
// communication stream, and is not allowed while another stream of the device is capturing).
void replay_release(ReplayEntry& x);
int replay_launch(ReplayEntry& x, hipStream_t s);
bool replay_eligible(const hgnn_net_config* c);

struct KeyBuilder {
    std::vector<uintptr_t> k;
    void add(uintptr_t v) { k.push_back(v); }
    void ptr(const void* p) { k.push_back(reinterpret_cast<uintptr_t>(p)); }
    void cfg(const hgnn_net_config* c) {
        const int32_t* w = reinterpret_cast<const int32_t*>(c);
        for (size_t i = 0; i < sizeof(hgnn_net_config) / 4; ++i) add((uintptr_t)(uint32_t)w[i]);
    }
    void inputs(const hgnn_net_inputs* in) {
        if (!in) return add(0);
        const void* const* p = reinterpret_cast<const void* const*>(in);
        for (size_t i = 0; i < sizeof(hgnn_net_inputs) / sizeof(void*); ++i) ptr(p[i]);
    }
    void csr(const hgnn_csr_batch* b) {
        if (!b) return add(0);
        ptr(b->d_node_off);
        ptr(b->d_edge_off);
        ptr(b->d_totals);
        ptr(b->d_n_batch);
        ptr(b->d_e_batch);
        ptr(b->d_x);
        ptr(b->d_xl);
        for (int k = 0; k < S_COUNT; ++k) {
            ptr(b->d_rows[k]);
            ptr(b->d_entries[k]);
        }
        add((uintptr_t)b->stride_w);
        add((uintptr_t)b->nodes);
        add((uintptr_t)b->edges);
    }
    template <typename T>
    void ptrs(T* const* p, int n) {
        for (int i = 0; i < n; ++i) ptr(p ? p[i] : nullptr);
    }
};

template <typename F>
int replayed(std::vector<uintptr_t> key, hipStream_t s, F&& enqueue) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    HGNN_HOST_CHECK(hipStreamIsCapturing(s, &st));
    if (st != hipStreamCaptureStatusNone) return enqueue(s);  // inside the caller's own capture
    ReplayCache* cache = nullptr;
    TRY(replay_cache(s, &cache));
    ReplayCache& rc = *cache;
    ReplayEntry* hit = nullptr;
    for (auto& x : rc.e)
        if (x.key == key) {
            hit = &x;
            break;
        }
    if (hit && hit->exec) {
        hit->last = ++rc.tick;
        return replay_launch(*hit, s);
    }
    if (!hit) {
        if (rc.e.size() >= REPLAY_MAX) {  // evict the least recently used entry
            size_t v = 0;
            for (size_t i = 1; i < rc.e.size(); ++i)
                if (rc.e[i].last < rc.e[v].last) v = i;
            replay_release(rc.e[v]);  // waits for its last launch only
            rc.e.erase(rc.e.begin() + v);
        }
        rc.e.push_back(ReplayEntry{});
        hit = &rc.e.back();
        hit->key = std::move(key);
    }
    hit->last = ++rc.tick;
    if (hit->failed || ++hit->seen < 3) return enqueue(s);
    // third call: capture the enqueue on the private stream, replay it on the caller's
    HGNN_HOST_CHECK(hipStreamBeginCapture(rc.cap, hipStreamCaptureModeRelaxed));
    const int r = enqueue(rc.cap);
    hipGraph_t gr = nullptr;
    const hipError_t ee = hipStreamEndCapture(rc.cap, &gr);
    hipGraphExec_t x = nullptr;
    hipEvent_t done = nullptr;
    const bool ok = r == 0 && ee == hipSuccess && gr && hipGraphInstantiate(&x, gr, nullptr, nullptr, 0) == hipSuccess &&
                    hipEventCreateWithFlags(&done, hipEventDisableTiming) == hipSuccess;
    if (gr) (void)hipGraphDestroy(gr);
    if (!ok) {
        (void)hipGetLastError();
        if (x) (void)hipGraphExecDestroy(x);
        hit->failed = true;
        return r ? r : enqueue(s);
    }
    hit->exec = x;
    hit->done = done;
    return replay_launch(*hit, s);
}

}  // namespace hgnn
