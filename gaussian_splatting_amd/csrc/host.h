// host.h -- host-side helpers of every translation unit that exports gsr_* functions (include/*.h):
// the error message behind gsr_last_error(), HIP_TRY, the scratch-allocator call and the stage profiler.
// The error buffer and the profiler are defined once, in api.hip.
#pragma once

#include <hip/hip_runtime_api.h>

#include <mutex>
#include <vector>

#include "../../include/gsr.h"

namespace gsr {

// Writes gsr_last_error()'s message (thread-local) and returns `code`.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// Empties the message; every entry point starts with it.
void clear_error();

#define HIP_TRY(expr, stage)                                                                                    \
    do {                                                                                                        \
        hipError_t _e = (expr);                                                                                 \
        if (_e != hipSuccess) return gsr::fail(GSR_ERR_HIP, "%s: %s", stage, hipGetErrorString(_e));            \
    } while (0)

inline void* call_alloc(gsr_alloc_fn fn, void* ctx, size_t bytes) {
    if (!fn) return nullptr;
    return fn(ctx, bytes ? bytes : 1);
}

// ---- stage profiler -----------------------------------------------------------
enum Stage {
    ST_PREPROCESS = 0,
    ST_BIN_COUNT,    // K1 + K2 of binning.hip
    ST_BIN_SCATTER,  // K3
    ST_TILE_SORT,    // K4
    ST_RENDER_FWD,
    ST_RENDER_BWD,
    ST_GAUSS_REDUCE,
    ST_GAUSS_BWD,
    ST_COUNT
};

struct Profiler {
    unsigned mask = 0;  // bit s: record stage s
    std::mutex mu;
    struct Pending {
        int stage;
        hipEvent_t a, b;
    };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;
    double total_ms[ST_COUNT] = {};
    long long calls[ST_COUNT] = {};
    hipEvent_t get() {
        if (!pool.empty()) {
            hipEvent_t e = pool.back();
            pool.pop_back();
            return e;
        }
        hipEvent_t e;
        (void)hipEventCreate(&e);
        return e;
    }
};
extern Profiler g_prof;

struct StageScope {
    int stage;
    hipStream_t stream;
    hipEvent_t a = nullptr;
    StageScope(int s, hipStream_t st) : stage(s), stream(st) {
        if ((g_prof.mask >> s) & 1u) {
            std::lock_guard<std::mutex> lk(g_prof.mu);
            a = g_prof.get();
            (void)hipEventRecord(a, stream);
        }
    }
    ~StageScope() {
        if (a) {
            std::lock_guard<std::mutex> lk(g_prof.mu);
            hipEvent_t b = g_prof.get();
            (void)hipEventRecord(b, stream);
            g_prof.pending.push_back({stage, a, b});
        }
    }
};

}  // namespace gsr
