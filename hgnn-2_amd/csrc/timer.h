// Optional per-kernel-class timer (bench.py times the dominant kernel class and the aggregation classes
// inside their timed regions with it).  Disabled (nullptr) on the normal path.  Modes (hgnn_timer_create_ex):
//   HGNN_TIMER_STAMPS     the launches of the timed classes that carry a stamp slot (the aggregation and GEMM
//                         kernels) write s_memrealtime per wave at entry and exit (common.h WaveStamp); a
//                         launch's time = max(exit) - min(entry).  Nothing is added to the stream, so the timed
//                         kernel runs as in an untimed step.
//   HGNN_TIMER_DISPATCH   every dispatch of a timed class gets an event pair bound to the dispatch itself
//                         (hipExtLaunchKernel); every class is covered, but a timed dispatch runs slower (its
//                         completion signal's system-scope release: 19 -> 30 us per aggregation-backward launch
//                         inside rocprofv3's own trace).
//   HGNN_TIMER_MARKERS    marker events recorded on the stream around each call (the round-1..4 form).
#pragma once

#include <vector>

#include "common.h"

namespace hgnn {

struct Timer {
    std::vector<hipEvent_t> ev;   // pairs: start, stop
    std::vector<int> cls;
    int used = 0;
    unsigned mask = 0;
    int mode = HGNN_TIMER_DISPATCH;
    uint64_t* st = nullptr;  // stamp buffer (device)
    long long st_cap = 0, st_used = 0;
    std::vector<int> st_off, st_n;
    std::vector<uintptr_t> st_strm;
    std::vector<double> st_ms;  // per launch, filled on the first read after a region
    std::vector<uint64_t> st_lo, st_hi;  // per launch: first entry / last exit stamp (10 ns ticks)
    bool st_read = false;
    int rd_used = -1;         // used / st_used at the last read: a read is reused only while neither moved
    long long rd_st_used = -1;
};

struct ClockScope {  // t_clock for the launches of one TL call
    LaunchClock c;
    LaunchClock* prev;
    ClockScope(Timer* tm, int k, hipStream_t s) : prev(t_clock) {
        c = LaunchClock{};
        c.cls = tm->cls.data();
        c.cap = (int)tm->cls.size();
        c.used = &tm->used;
        c.k = k;
        if (tm->mode == HGNN_TIMER_STAMPS) {
            c.st = tm->st;
            c.st_off = tm->st_off.data();
            c.st_n = tm->st_n.data();
            c.st_cap = tm->st_cap;
            c.st_used = &tm->st_used;
            c.strm = reinterpret_cast<uintptr_t>(s);
            c.st_strm = tm->st_strm.data();
        } else {
            c.ev = tm->ev.data();
        }
        t_clock = &c;
    }
    ~ClockScope() { t_clock = prev; }
};

// One launcher call of class k on stream s under the timer tm (nullptr: untimed).  The timer's events or stamps
// go on s, the stream the kernel runs on.
template <typename F>
inline int timed(Timer* tm, int k, hipStream_t s, F&& launch) {
    if (!tm || !(tm->mask & (1u << k)) || tm->used >= (int)tm->cls.size()) return launch();
    if (tm->mode != HGNN_TIMER_MARKERS) {
        ClockScope cs(tm, k, s);
        return launch();
    }
    HGNN_HOST_CHECK(hipEventRecord(tm->ev[2 * tm->used], s));
    TRY(launch());
    HGNN_HOST_CHECK(hipEventRecord(tm->ev[2 * tm->used + 1], s));
    tm->cls[tm->used++] = k;
    return 0;
}

// TL(class, stream, launcher call): the call under the enclosing scope's timer `tm`; a non-zero status returns
#define TL(k, stream, call) TRY(hgnn::timed(tm, (k), (stream), [&] { return (call); }))

}  // namespace hgnn
