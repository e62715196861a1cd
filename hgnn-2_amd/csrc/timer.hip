// The hgnn_timer_* entry points (timer.h).
#include "timer.h"

#include "switches.h"

using namespace hgnn;

extern "C" {

void* hgnn_timer_create_ex(int max_launches, unsigned class_mask, int mode, long long stamp_words) {
    if (max_launches <= 0) return nullptr;
    if (mode != HGNN_TIMER_STAMPS && mode != HGNN_TIMER_DISPATCH && mode != HGNN_TIMER_MARKERS) return nullptr;
    Timer* t = new Timer();
    t->cls.resize(max_launches);
    t->mask = class_mask;
    t->mode = mode;
    if (mode == HGNN_TIMER_STAMPS) {
        if (stamp_words <= 0 || stamp_words > (1ll << 31) - 1) {
            delete t;
            return nullptr;
        }
        t->st_off.resize(max_launches);
        t->st_n.resize(max_launches);
        t->st_strm.resize(max_launches);
        t->st_cap = stamp_words;
        if (hipMalloc(&t->st, (size_t)stamp_words * 8) != hipSuccess ||
            hipMemset(t->st, 0, (size_t)stamp_words * 8) != hipSuccess) {
            if (t->st) (void)hipFree(t->st);
            delete t;
            return nullptr;
        }
        return t;
    }
    t->ev.resize(2 * (size_t)max_launches);
    for (auto& e : t->ev) {
        if (hipEventCreate(&e) != hipSuccess) {
            delete t;
            return nullptr;
        }
    }
    return t;
}

void* hgnn_timer_create(int max_launches, unsigned class_mask) {
    return hgnn_timer_create_ex(max_launches, class_mask,
                                hgnn::switches().timer_markers ? HGNN_TIMER_MARKERS : HGNN_TIMER_DISPATCH, 0);
}

void hgnn_timer_reset(void* timer) {
    if (!timer) return;
    Timer* t = static_cast<Timer*>(timer);
    t->used = 0;
    if (t->st) {
        (void)hipDeviceSynchronize();
        (void)hipMemset(t->st, 0, (size_t)t->st_used * 8);
        t->st_used = 0;
        t->st_read = false;
    }
}

// Stamp mode: a launch's time = max over its waves' exit stamps - min over their entry stamps (100 MHz).
static int timer_read_stamps(Timer* t) {
    if (t->st_read && t->rd_used == t->used && t->rd_st_used == t->st_used) return HGNN_OK;
    if (hipDeviceSynchronize() != hipSuccess) return HGNN_ERR_HIP;
    std::vector<uint64_t> h((size_t)t->st_used);
    if (t->st_used && hipMemcpy(h.data(), t->st, (size_t)t->st_used * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return HGNN_ERR_HIP;
    t->st_ms.assign(t->used, 0.0);
    t->st_lo.assign(t->used, 0);
    t->st_hi.assign(t->used, 0);
    for (int i = 0; i < t->used; ++i) {
        uint64_t lo = ~0ull, hi = 0;
        for (int w = 0; w < t->st_n[i] / 2; ++w) {
            const uint64_t a = h[t->st_off[i] + 2 * w], b = h[t->st_off[i] + 2 * w + 1];
            if (a && a < lo) lo = a;
            if (b > hi) hi = b;
        }
        t->st_ms[i] = hi > lo && lo != ~0ull ? (double)(hi - lo) * 1e-5 : 0.0;  // 10 ns ticks -> ms
        t->st_lo[i] = lo == ~0ull ? 0 : lo;
        t->st_hi[i] = hi;
    }
    t->st_read = true;
    t->rd_used = t->used;
    t->rd_st_used = t->st_used;
    return HGNN_OK;
}

int hgnn_timer_elapsed(void* timer, int kernel_class, double* total_ms, int* launches) {
    if (!timer || !total_ms || !launches) return HGNN_ERR_ARG;
    Timer* t = static_cast<Timer*>(timer);
    double tot = 0.0;
    int n = 0;
    if (t->mode == HGNN_TIMER_STAMPS) {
        const int r = timer_read_stamps(t);
        if (r) return r;
        for (int i = 0; i < t->used; ++i)
            if (t->cls[i] == kernel_class) {
                tot += t->st_ms[i];
                ++n;
            }
        *total_ms = tot;
        *launches = n;
        return HGNN_OK;
    }
    for (int i = 0; i < t->used; ++i) {
        if (t->cls[i] != kernel_class) continue;
        float ms = 0.f;
        if (hipEventSynchronize(t->ev[2 * i + 1]) != hipSuccess) return HGNN_ERR_HIP;
        if (hipEventElapsedTime(&ms, t->ev[2 * i], t->ev[2 * i + 1]) != hipSuccess) return HGNN_ERR_HIP;
        tot += ms;
        ++n;
    }
    *total_ms = tot;
    *launches = n;
    return HGNN_OK;
}

int hgnn_timer_launches(void* timer, int max, int* cls, double* t_entry_us, double* t_exit_us, int* stream_idx) {
    if (!timer || max < 0 || (max > 0 && (!cls || !t_entry_us || !t_exit_us))) return -HGNN_ERR_ARG;
    Timer* t = static_cast<Timer*>(timer);
    if (t->mode != HGNN_TIMER_STAMPS) return -HGNN_ERR_UNSUPPORTED;
    const int r = timer_read_stamps(t);
    if (r) return -r;
    uint64_t base = ~0ull;
    for (int i = 0; i < t->used; ++i)
        if (t->st_lo[i] && t->st_lo[i] < base) base = t->st_lo[i];
    const int n = t->used < max ? t->used : max;
    std::vector<uintptr_t> seen;
    for (int i = 0; i < n; ++i) {
        cls[i] = t->cls[i];
        if (stream_idx) {
            int q = 0;
            while (q < (int)seen.size() && seen[q] != t->st_strm[i]) ++q;
            if (q == (int)seen.size()) seen.push_back(t->st_strm[i]);
            stream_idx[i] = q;
        }
        t_entry_us[i] = t->st_lo[i] ? (double)(t->st_lo[i] - base) * 1e-2 : -1.0;
        t_exit_us[i] = t->st_hi[i] ? (double)(t->st_hi[i] - base) * 1e-2 : -1.0;
    }
    return t->used;
}

long long hgnn_timer_waves(void* timer, int launch, long long max, double* entry_us, double* exit_us) {
    if (!timer || max < 0 || (max > 0 && (!entry_us || !exit_us))) return -HGNN_ERR_ARG;
    Timer* t = static_cast<Timer*>(timer);
    if (t->mode != HGNN_TIMER_STAMPS) return -HGNN_ERR_UNSUPPORTED;
    if (launch < 0 || launch >= t->used) return -HGNN_ERR_ARG;
    if (hipDeviceSynchronize() != hipSuccess) return -HGNN_ERR_HIP;
    const int r = timer_read_stamps(t);
    if (r) return -r;
    uint64_t base = ~0ull;
    for (int i = 0; i < t->used; ++i)
        if (t->st_lo[i] && t->st_lo[i] < base) base = t->st_lo[i];
    const long long nw = t->st_n[launch] / 2, n = nw < max ? nw : max;
    if (n > 0) {
        std::vector<uint64_t> h((size_t)(2 * n));
        if (hipMemcpy(h.data(), t->st + t->st_off[launch], (size_t)(2 * n) * 8, hipMemcpyDeviceToHost) != hipSuccess)
            return -HGNN_ERR_HIP;
        for (long long w = 0; w < n; ++w) {
            entry_us[w] = h[2 * w] ? (double)(h[2 * w] - base) * 1e-2 : -1.0;
            exit_us[w] = h[2 * w + 1] ? (double)(h[2 * w + 1] - base) * 1e-2 : -1.0;
        }
    }
    return nw;
}

void hgnn_timer_destroy(void* timer) {
    if (!timer) return;
    Timer* t = static_cast<Timer*>(timer);
    for (auto& e : t->ev) (void)hipEventDestroy(e);
    if (t->st) {
        (void)hipDeviceSynchronize();
        (void)hipFree(t->st);
    }
    delete t;
}

}  // extern "C"
