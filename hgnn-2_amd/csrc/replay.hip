// The replay cache of the executor's launch-bound calls (replay.h).
#include "replay.h"

namespace hgnn {

void replay_release(ReplayEntry& x) {
    if (x.done) (void)hipEventSynchronize(x.done);
    if (x.exec) (void)hipGraphExecDestroy(x.exec);
    if (x.done) (void)hipEventDestroy(x.done);
    x.exec = nullptr;
    x.done = nullptr;
}

int replay_launch(ReplayEntry& x, hipStream_t s) {
    if (hipGraphLaunch(x.exec, s) != hipSuccess) return HGNN_ERR_HIP;
    return hipEventRecord(x.done, s) == hipSuccess ? 0 : HGNN_ERR_HIP;
}

bool replay_eligible(const hgnn_net_config* c) {
    const Tri mode = switches().exec_graph;  // HGNN_EXEC_GRAPH=0 / =1: never / always
    if (mode != Tri::Auto) return mode == Tri::On;
    return (long long)c->bs * c->nmax <= 4096 && (c->kind == 0 || (long long)c->bs * c->emax <= 8192);
}

static int replay_reset(ReplayCache& rc, int dev) {
    if (rc.dev >= 0) {
        for (auto& x : rc.e) replay_release(x);
        if (rc.cap) (void)hipStreamDestroy(rc.cap);
    }
    rc = ReplayCache{};
    int cur = 0;
    HGNN_HOST_CHECK(hipGetDevice(&cur));
    HGNN_HOST_CHECK(hipSetDevice(dev));
    const hipError_t e = hipStreamCreateWithFlags(&rc.cap, hipStreamNonBlocking);
    HGNN_HOST_CHECK(hipSetDevice(cur));
    if (e != hipSuccess) return HGNN_ERR_HIP;
    rc.dev = dev;
    return 0;
}

int replay_cache(hipStream_t s, ReplayCache** out) {
    thread_local ReplayCache rc;
    hipDevice_t dev = 0;
    HGNN_HOST_CHECK(hipStreamGetDevice(s, &dev));
    if (rc.dev != dev) TRY(replay_reset(rc, dev));
    *out = &rc;
    return 0;
}

}  // namespace hgnn
