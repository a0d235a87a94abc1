// Host plumbing (mbrl_host.h, and the device queries of mbrl_internal.h) and the ABI entries that
// are no planner's: version, build info, last error, options, mapped host memory, events.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include <atomic>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <tuple>

#include "mbrl_host.h"

namespace mbrl {

static thread_local std::string g_err;

// mbrl_set_option switches (include/mbrl_cem.h MBRL_OPT_*); 0 = automatic.
static std::atomic<int> g_opt[MBRL_OPT_END];

int opt(int option) { return g_opt[option].load(std::memory_order_relaxed); }

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int hip_check(hipError_t e, const char* what) {
    if (e == hipSuccess) return MBRL_OK;
    return fail(MBRL_EHIP, "%s: %s", what, hipGetErrorString(e));
}

// Compute units of the current device (cached per device; 256 on MI355X).
int device_cu_count() {
    static std::mutex mu;
    static std::map<int, int> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(dev);
    if (it != cache.end()) return it->second;
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cache[dev] = n;
    return n;
}

hipError_t ensure_dynamic_lds(const void* fn, int bytes) {
    static std::mutex mu;
    static std::set<std::tuple<const void*, int, int>> done;
    int dev = 0;
    hipError_t err = hipGetDevice(&dev);
    if (err != hipSuccess) return err;
    std::lock_guard<std::mutex> lock(mu);
    if (done.count({fn, dev, bytes})) return hipSuccess;
    err = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (err == hipSuccess) done.insert({fn, dev, bytes});
    return err;
}

bool grid_fits(const void* fn, int threads, size_t lds, int blocks) {
    static std::mutex mu;
    static std::map<std::tuple<const void*, int, size_t, int>, int> cache;   // -> resident workgroups
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    const auto key = std::make_tuple(fn, threads, lds, dev);
    {
        std::lock_guard<std::mutex> lock(mu);
        auto it = cache.find(key);
        if (it != cache.end()) return blocks <= it->second;
    }
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds) != hipSuccess) per_cu = 0;
    const int capacity = per_cu * device_cu_count();
    std::lock_guard<std::mutex> lock(mu);
    cache[key] = capacity;
    return blocks <= capacity;
}

int shape_geometry(const mbrl_mlp_shape* sh, Geometry* g) {
    if (!sh) return fail(MBRL_EINVAL, "shape is NULL");
    if (sh->precision != MBRL_PRECISION_F32 && sh->precision != MBRL_PRECISION_F16X3 &&
        sh->precision != MBRL_PRECISION_F16X6)
        return fail(MBRL_EINVAL, "precision %d is not an MBRL_PRECISION_* value", sh->precision);
    if (!make_geometry(sh->state_dim, sh->action_dim, sh->hidden, sh->n_hidden, sh->ensemble, sh->reward_head, g))
        return fail(MBRL_EUNSUPPORTED,
                    "unsupported MLP shape s=%d a=%d W=%d L=%d E=%d reward_head=%d (need all >= 1, W <= 1024, L <= %d)",
                    sh->state_dim, sh->action_dim, sh->hidden, sh->n_hidden, sh->ensemble, sh->reward_head, MAX_LAYERS);
    g->precision = sh->precision;
    return MBRL_OK;
}

}  // namespace mbrl

using namespace mbrl;

extern "C" {

int mbrl_abi_version(void) { return MBRL_ABI_VERSION; }

#if __has_include("src_digest.h")
#include "src_digest.h"
#else
#define MBRL_SRC_DIGEST "unknown"
#endif
const char* mbrl_build_info(void) { return "src=" MBRL_SRC_DIGEST " arch=gfx950"; }

const char* mbrl_last_error(void) { return g_err.c_str(); }

int mbrl_set_option(int32_t option, int32_t value) {
    if (option < 0 || option >= MBRL_OPT_END) return fail(MBRL_EINVAL, "unknown option %d", option);
    bool ok = false;
    switch (option) {
        case MBRL_OPT_ROLLOUT_TILE: ok = value == 0 || value == 4 || value == 8 || value == 16; break;
        case MBRL_OPT_SPLIT_TILE: ok = value == 0 || value == 16 || value == 32; break;
        case MBRL_OPT_ADAM_ARITH: ok = value >= 0 && value <= 16; break;
        case MBRL_OPT_TRAIN_TILE: ok = value == 0 || value == 32 || value == 64; break;
        case MBRL_OPT_ROLLOUT_PAIR: ok = value >= 0 && value <= 2; break;
        case MBRL_OPT_DEBUG_PAIR_ABORT: ok = value >= 0 && value <= 2; break;
        case MBRL_OPT_TRAJ_HOP: ok = value >= 0 && value <= 3; break;
        case MBRL_OPT_GD_HOP: ok = value >= 0 && value <= 3; break;
        case MBRL_OPT_PAIR_L2: ok = value >= 0 && value <= 2; break;
        case MBRL_OPT_DEBUG_SHARD_FAIL: ok = value >= 0 && value <= 1 << 20; break;
        case MBRL_OPT_DEBUG_SHARD_FAIL_RANK: ok = value >= 0 && value <= 1 << 20; break;
        case MBRL_OPT_SHARD_EMULATE: ok = value >= 0 && value <= 2; break;
        case MBRL_OPT_UPDATE_SPLIT: ok = value >= 0 && value <= 2; break;
        case MBRL_OPT_ROLLOUT_GROUP_SEAM: ok = value >= 0 && value <= 2; break;
        default: ok = value == 0 || value == 1; break;
    }
    if (!ok) return fail(MBRL_EINVAL, "option %d: value %d not allowed", option, value);
    return g_opt[option].exchange(value);
}

int mbrl_host_alloc(size_t bytes, void** host_ptr, void** device_ptr) {
    if (!host_ptr || !device_ptr || bytes == 0) return fail(MBRL_EINVAL, "mbrl_host_alloc: bad arguments");
    *host_ptr = nullptr;
    *device_ptr = nullptr;
    void* h = nullptr;
    int rc = hip_check(hipHostMalloc(&h, bytes, hipHostMallocMapped | hipHostMallocCoherent), "hipHostMalloc");
    if (rc) return rc;
    void* d = nullptr;
    rc = hip_check(hipHostGetDevicePointer(&d, h, 0), "hipHostGetDevicePointer");
    if (rc) {
        (void)hipHostFree(h);
        return rc;
    }
    *host_ptr = h;
    *device_ptr = d;
    return MBRL_OK;
}

int mbrl_host_free(void* host_ptr) {
    return host_ptr ? hip_check(hipHostFree(host_ptr), "hipHostFree") : MBRL_OK;
}

int mbrl_event_create(mbrl_event_t* event) {
    if (!event) return fail(MBRL_EINVAL, "event_create: NULL");
    hipEvent_t e = nullptr;
    if (int rc = hip_check(hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence),
                           "hipEventCreateWithFlags"))
        return rc;
    *event = reinterpret_cast<mbrl_event_t>(e);
    return MBRL_OK;
}

int mbrl_event_record(mbrl_event_t event, mbrl_stream_t stream) {
    if (!event) return fail(MBRL_EINVAL, "event_record: NULL event");
    return hip_check(hipEventRecord(reinterpret_cast<hipEvent_t>(event), reinterpret_cast<hipStream_t>(stream)),
                     "hipEventRecord");
}

int mbrl_stream_wait_event(mbrl_stream_t stream, mbrl_event_t event) {
    if (!event) return fail(MBRL_EINVAL, "stream_wait_event: NULL event");
    return hip_check(hipStreamWaitEvent(reinterpret_cast<hipStream_t>(stream), reinterpret_cast<hipEvent_t>(event), 0),
                     "hipStreamWaitEvent");
}

int mbrl_event_synchronize(mbrl_event_t event) {
    if (!event) return fail(MBRL_EINVAL, "event_synchronize: NULL event");
    return hip_check(hipEventSynchronize(reinterpret_cast<hipEvent_t>(event)), "hipEventSynchronize");
}

int mbrl_event_destroy(mbrl_event_t event) {
    return event ? hip_check(hipEventDestroy(reinterpret_cast<hipEvent_t>(event)), "hipEventDestroy") : MBRL_OK;
}

int mbrl_get_option(int32_t option) {
    if (option < 0 || option >= MBRL_OPT_END) return fail(MBRL_EINVAL, "unknown option %d", option);
    return g_opt[option].load();
}

}  // extern "C"
