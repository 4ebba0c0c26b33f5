// api.hip -- the rasterizer's host orchestration and its part of the extern "C" boundary (include/gsr.h):
// the forward and backward, the runtime options, the profile, census and debug entry points, and the one
// definition of the error message and the stage profiler that host.h declares.  The other components' entry
// points are beside their kernels (ssim.hip, knn.hip, adam.hip, densify.hip, views.hip; ply.cpp).
//
// Forward stage order mirrors CudaRasterizer::Rasterizer::forward
// (CR/rasterizer_impl.cu:227-370); the stages themselves are this project's
// (depth pre-sort + 16-bit tile sort instead of one 64-bit sort, footprint
// culling in the blender, atomic-free backward).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdlib>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <chrono>
#include <algorithm>
#include <mutex>
#include <thread>
#include <vector>

#include "camera.h"
#include "host.h"
#include "kernels.h"

namespace {
thread_local char g_err[1024] = "";
}  // namespace

namespace gsr {

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

void clear_error() { (void)fail(GSR_OK, "%s", ""); }  // (fail is the buffer's only writer)

Profiler g_prof;

}  // namespace gsr

using namespace gsr;

namespace {

const char* kStageNames[ST_COUNT] = {"preprocess", "bin_count",  "bin_scatter",  "tile_sort",
                                     "render_fwd", "render_bwd", "gauss_reduce", "gauss_bwd"};

unsigned long long* g_census = nullptr;  // gsr_census_set: device counters of the census render kernels

int check_debug(int debug, hipStream_t stream, const char* stage) {
    if (!debug) return GSR_OK;
    hipError_t e = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return fail(GSR_ERR_HIP, "%s: %s", stage, hipGetErrorString(e));
    return GSR_OK;
}


gsr::GeomState carve_geom(char* base, int P, uint32_t gx, uint32_t gy, size_t* total) {
    using namespace gsr;
    Carver c{base, 0};
    GeomState g{};
    g.rec = c.take<float4>((size_t)kRecRows * P);
    g.depth_key = c.take<uint32_t>(P);
    g.tiles_touched = c.take<uint32_t>(P);
    g.rect = c.take<uint2>(P);
    g.rec_start = c.take<uint32_t>(P);
    g.clamped = c.take<uint8_t>(P);
    g.status = c.take<uint32_t>(4);
    g.fwd_seg_ck = g.status + 2;
    const uint32_t tiles = gx * gy;
    const size_t cells = bin_cell_count(gx, gy);
    // the counters preprocess zeroes in one range (bin_zero_words): tile counts, cell counts, near counts,
    // the depth-mass histogram (8-byte aligned)
    g.tile_cnt = c.take<uint32_t>(bin_zero_words(tiles, cells));
    g.cell_cnt = g.tile_cnt + tiles;
    g.near_cnt = g.cell_cnt + cells;
    g.zhist = reinterpret_cast<unsigned long long*>(g.tile_cnt + ((2 * (size_t)tiles + cells + 1) & ~(size_t)1));
    g.tile_base = c.take<uint32_t>(tiles);
    const size_t chunks = bin_chunk_count(P);
    g.cell_off = c.take<uint32_t>(chunks * cells);
    g.order = c.take<uint4>(P);
    g.n_visible = c.take<uint32_t>(1);

    g.chunk_off = c.take<uint32_t>(chunks * tiles);
    g.cls_list = c.take<uint32_t>(2 * (size_t)tiles);
    g.cls_count = c.take<uint32_t>(2);
    g.chunk_total = c.take<unsigned long long>(chunks);
    g.total = c.take<unsigned long long>(1);
    g.unit_cnt = c.take<uint32_t>((size_t)kUnitLists * kUnitShards * kUnitCntStride);
    g.unit_part = c.take<uint2>((size_t)(kUnitLists - 1) * kUnitShards * unit_part_cap(tiles));
    g.tile_join = c.take<unsigned long long>(tiles);
    g.sorted_len = c.take<uint32_t>(tiles);
    g.redo_flag = c.take<uint32_t>(tiles);
    g.redo_list = c.take<uint32_t>(tiles);
    g.redo_cnt = c.take<uint32_t>(1);
    g.acc = c.take<float4>((size_t)kAccRow4 * P);
    g.touched = c.take<uint32_t>(touched_words((size_t)P));
    g.mass = c.take<uint32_t>(P);
    g.zcut = g.status + 3;
    g.sranges = c.take<uint2>(tiles);
    g.far_cur = c.take<uint32_t>(tiles);
    *total = align_up(c.off);
    return g;
}

}  // namespace

namespace gsr {
// camera.h: the camera backward (camera.hip) reads the forward's SH clamp flags
const uint8_t* geom_clamped(const void* geom_buffer, int P, int width, int height) {
    size_t tmp = 0;
    return carve_geom((char*)geom_buffer, P, (width + kTile - 1) / kTile, (height + kTile - 1) / kTile, &tmp).clamped;
}
}  // namespace gsr

namespace {

gsr::ImageState carve_image(char* base, int W, int H, uint32_t tiles, size_t* total) {
    using namespace gsr;
    Carver c{base, 0};
    ImageState im{};
    const size_t N = (size_t)W * H;
    const size_t NT = (size_t)tiles * 256;  // tile-major pixel planes (gsr_common.h tile_px)
    (void)N;
    im.final_T = c.take<float>(NT);
    im.n_contrib = c.take<uint32_t>(NT);
    im.accum = c.take<float>(4 * NT);
    im.ranges = c.take<uint2>(tiles);
    *total = align_up(c.off);
    return im;
}

gsr::BinningState carve_binning(char* base, size_t C, size_t* total) {
    using namespace gsr;
    Carver c{base, 0};
    BinningState b{};
    b.keys = c.take<unsigned long long>(C);
    b.gid_sorted = c.take<uint32_t>(C);
    b.ckpt = c.take<float>((C / kCkStride + 1) * (size_t)kCkFloats);
    b.unit_full = c.take<uint2>(kUnitShards * unit_full_cap(C));
    b.rec_flag = c.take<uint8_t>(((C + 15) & ~(size_t)15) + 16);  // K3 / gauss_reduce use aligned 16-byte words
    *total = align_up(c.off);
    return b;
}

// The forward's binning capacities are multiples of kCapQuantum (up to INT_MAX).  Over those the
// buffer size is strictly increasing (the keys alone grow by 8 * kCapQuantum bytes a step) and
// every sub-array's length depends on C / kCkStride at most, so the size of the binning buffer
// identifies its layout: the backward recovers the capacity from the tensor's byte count, which
// survives any transport of the saved tensor (saved-tensor hooks, save_on_cpu, clone).
constexpr size_t kCapQuantum = 256;
static_assert(kCapQuantum % gsr::kCkStride == 0, "capacity quantum is a whole number of checkpoint strides");

size_t quantize_capacity(size_t c) { return (c + kCapQuantum - 1) / kCapQuantum * kCapQuantum; }

size_t binning_bytes_for(size_t C) {
    size_t b = 0;
    carve_binning(nullptr, C, &b);
    return b;
}

// Capacity the binning buffer of a forward was laid out for: the explicit value if given,
// else the multiple of kCapQuantum whose layout has exactly `bytes` bytes, else R (the exact
// layout, which the forward keeps past INT_MAX).  Returns false if `bytes` matches no layout holding R.
bool resolve_capacity(int R, int capacity, size_t bytes, size_t* C) {
    if (capacity > 0) {
        *C = (size_t)capacity;
        return bytes == 0 || binning_bytes_for(*C) == bytes;
    }
    if (bytes == 0) {
        *C = (size_t)R;
        return true;
    }
    size_t lo = quantize_capacity((size_t)R) / kCapQuantum, hi = bytes / (8 * kCapQuantum) + 1;
    while (lo < hi) {  // first k in [lo, hi] with bytes_for(k * quantum) >= bytes
        const size_t mid = lo + (hi - lo) / 2;
        if (binning_bytes_for(mid * kCapQuantum) < bytes) lo = mid + 1; else hi = mid;
    }
    if (binning_bytes_for(lo * kCapQuantum) == bytes) {
        *C = lo * kCapQuantum;
        return true;
    }
    *C = (size_t)R;
    return binning_bytes_for((size_t)R) == bytes;
}

// Backward scratch: R per-instance records, P per-Gaussian sums, the live list (the records' content
// bytes are in the binning buffer).
void carve_recs(char* base, size_t R, size_t P, gsr::GradRecs* recs, gsr::GradRecs* sums, uint32_t** live,
                uint32_t** live_count, size_t* total) {
    using namespace gsr;
    Carver c{base, 0};
    {  // interleaved 48-byte records (gsr_common.h kRecAB / kRecC)
        float4* r48 = c.take<float4>(3 * R);
        recs->a = r48;
        recs->b = r48 + 1;
        recs->c = reinterpret_cast<float2*>(r48 + 2);
    }
    recs->flag = nullptr;  // in the binning buffer (BinningState::rec_flag)
    // (per Gaussian, gauss_reduce's; the atomic backward reads its accumulator rows instead)
    sums->a = c.take<float4>(P);
    sums->b = c.take<float4>(P);
    sums->c = c.take<float2>(P);
    sums->flag = nullptr;
    // the Gaussians with a gradient (gauss_reduce appends, gauss_bwd walks), kLiveShards shards
    *live = c.take<uint32_t>((size_t)kLiveShards * live_list_cap((uint32_t)P));
    *live_count = c.take<uint32_t>((size_t)kLiveShards * kLiveCntStride);
    *total = align_up(c.off);
}

// ---- runtime options (include/gsr.h gsr_option_set) ------------------------------
// The library's alternative kernel paths.  Each default comes from GSR_<NAME> in the environment
// at first use; gsr_option_set changes it for later calls (tests/test_gpu_options.py runs every
// path against the oracle).
constexpr uint32_t kFusedFillBlocks = 256;  // one-wave fill blocks in render_bwd's launch (the side-stream kernel: 64 x 4 waves)
// "near_mass": near-first binning (binning.hip) -- only the Gaussians in front of the depth at which the
// screen-averaged opacity mass reaches this value get keys and are sorted; 0 = off.  Capacity-hinted
// forwards with the fused scan only.
// "bwd_atomic": the render backward adds each instance's sums into per-Gaussian rows with float atomics
// (render.hip ATOMIC) and gauss_bwd lists the touched Gaussians itself, instead of per-instance records summed
// by gauss_reduce (deterministic).  The forward zeroes the rows when the option is on at forward time and
// marks its buffer (geom_mark below); a backward adds atomically iff the option is on and its buffer is marked.
constexpr uint32_t kFwdFillBlocks = 256;  // one-wave blocks zeroing the accumulators in render_fwd's launch (a multiple of 8)
static_assert(kFwdFillBlocks % 8 == 0, "the forward's fill blocks keep the tiles' XCD mapping");
enum Opt {
    OPT_FUSED_BIN = 0, OPT_FWD_QUADS, OPT_BWD_SEG_CK, OPT_HOST_TOTAL, OPT_ZERO_FILL, OPT_LIVE_LIST, OPT_SORT_PREFIX,
    OPT_COUNT_WAIT, OPT_BWD_GRID, OPT_BWD_ATOMIC, OPT_NEAR_MASS, OPT_TOUCHED_RUN, OPT_COUNT
};
struct OptionSpec {
    const char* name;
    const char* env;
    int def, lo, hi;
};
const OptionSpec kOptions[OPT_COUNT] = {
    {"fused_bin", "GSR_FUSED_BIN", 1, 0, 1},
    {"fwd_quads", "GSR_FWD_QUADS", 2, 2, 4},
    {"bwd_seg_ck", "GSR_BWD_SEG_CK", 1, 1, 1 << 20},
    {"host_total", "GSR_HOST_TOTAL", 1, 0, 1},
    {"zero_fill", "GSR_ZERO_FILL", 3, 0, 3},
    {"live_list", "GSR_LIVE_LIST", 1, 0, 1},
    {"sort_prefix", "GSR_SORT_PREFIX", 1024, 0, (int)gsr::kSortPrefixMax},
    {"count_wait", "GSR_COUNT_WAIT", 2, 0, 2},
    {"bwd_grid", "GSR_BWD_GRID", 0, 0, 2},
    {"bwd_atomic", "GSR_BWD_ATOMIC", 1, 0, 1},
    {"near_mass", "GSR_NEAR_MASS", 30, 0, 1 << 20},
    {"touched_run", "GSR_TOUCHED_RUN", 0, 0, 32},
};
std::atomic<int> g_opt[OPT_COUNT];
std::once_flag g_opt_once;

void options_init() {
    std::call_once(g_opt_once, [] {
        for (int i = 0; i < OPT_COUNT; i++) {
            const OptionSpec& o = kOptions[i];
            int v = o.def;
            if (const char* e = getenv(o.env)) {
                const int x = atoi(e);
                // out-of-range values clamp (a huge GSR_BWD_SEG_CK means "one unit per tile")
                v = x < o.lo ? o.lo : x > o.hi ? o.hi : x;
                if (i == OPT_FWD_QUADS) v = x == 4 ? 4 : 2;
            }
            g_opt[i].store(v, std::memory_order_relaxed);
        }
    });
}

// Per-thread overrides (gsr_option_set_thread): kOptNone where the process-wide value applies.
constexpr int kOptNone = INT_MIN;
thread_local int t_opt[OPT_COUNT] = {kOptNone, kOptNone, kOptNone, kOptNone, kOptNone, kOptNone, kOptNone, kOptNone,
                                     kOptNone, kOptNone, kOptNone, kOptNone};
static_assert(OPT_COUNT == 12, "one kOptNone per option above");

int option(int id) {
    if (t_opt[id] != kOptNone) return t_opt[id];
    options_init();
    return g_opt[id].load(std::memory_order_relaxed);
}

int option_index(const char* name) {
    if (!name) return -1;
    for (int i = 0; i < OPT_COUNT; i++)
        if (strcmp(name, kOptions[i].name) == 0) return i;
    return -1;
}

// What each geometry buffer's last forward left for its backwards: whether it zeroed the atomic backward's
// accumulator rows ("bwd_atomic" on at forward time) and whether its K3 wrote the record path's inputs (record
// starts, zeroed content bits; skipped when the forward zeroed the rows).  A
// backward adds atomically only into a zeroed buffer, and before a record-path backward of a buffer without
// record inputs it writes them (launch_rec_prep).  A buffer the library never saw (copied in) is neither: the
// record path, after the prep.  Every forward re-marks its buffer, so an address the caching allocator hands
// out again carries its latest forward's state.  Bounded: past kGeomMarksMax entries the table starts over
// (a miss costs a prep, never a wrong result).
struct GeomMark {
    const void* buf;
    bool zeroed, recs;
    bool long_lists;  // the frame's mean tile list is long (kLongMeanList): few of its Gaussians are touched
    // the render ran as half-tile / quadrant units (not the whole-tile kernel of "fwd_quads" 4): the T in its blend
    // checkpoints rounds as contrib.hip's own (gsr_contrib_stats)
    bool half_fwd;
};
std::mutex g_mark_mu;
std::vector<GeomMark> g_marks;
constexpr size_t kGeomMarksMax = 4096;

void geom_mark(const void* geom_buffer, bool zeroed, bool recs, bool long_lists, bool half_fwd) {
    std::lock_guard<std::mutex> lk(g_mark_mu);
    for (auto& m : g_marks)
        if (m.buf == geom_buffer) {
            m.zeroed = zeroed;
            m.recs = recs;
            m.long_lists = long_lists;
            m.half_fwd = half_fwd;
            return;
        }
    if (!zeroed && !recs) return;  // (absent = neither)
    if (g_marks.size() >= kGeomMarksMax) g_marks.clear();
    g_marks.push_back(GeomMark{geom_buffer, zeroed, recs, long_lists, half_fwd});
}

void geom_forget(const void* geom_buffer) {
    std::lock_guard<std::mutex> lk(g_mark_mu);
    for (size_t i = 0; i < g_marks.size(); i++)
        if (g_marks[i].buf == geom_buffer) {
            g_marks[i] = g_marks.back();
            g_marks.pop_back();
            return;
        }
}

GeomMark geom_marked(const void* geom_buffer) {
    std::lock_guard<std::mutex> lk(g_mark_mu);
    for (const auto& m : g_marks)
        if (m.buf == geom_buffer) return m;
    return GeomMark{geom_buffer, false, false, false, false};
}

// A frame whose mean tile list holds at least this many entries is a "long-list" frame: near-first binning
// applies (below) and the atomic backward lists its touched Gaussians over longer runs (few are touched).
constexpr size_t kLongMeanList = 2048;

// K2 folded into K3 in capacity mode.
bool fused_binning_mode() { return option(OPT_FUSED_BIN) != 0; }

// The reachable-prefix sort of long lists ("sort_prefix" option, binning.hip K4) for a binning
// buffer of capacity C: on when the frame's lists are long -- mean length >= 2 L -- where sorting
// only their first L entries saves most of K4 (5M@4K: tile_sort 0.70 -> 0.49 ms); off for shorter
// lists, where it saves nothing and the two redo launches cost ~8 us (1M@1080p, r3c).  Census runs
// sort whole lists (a redone tile's first pass would be counted twice).  The results are the same
// either way.
// L <= kSortPrefixMax (the option's range): the prefix kernel's LDS holds 2 kSortPrefixMax keys, so a
// prefix plus the rest of its last bucket fits (a longer one would send every long list to the
// global-memory fallback sort).
uint32_t sort_prefix_for(size_t C, uint32_t tiles, uint32_t L) {
    L = std::min(L, gsr::kSortPrefixMax);
    if (!L || g_census || tiles == 0) return 0u;
    return C / tiles >= 2ull * L ? L : 0u;
}

// Per (host thread, device): a pinned 8-byte slot that num_rendered is copied into and the
// event recorded behind that copy.  The host waits on the event -- i.e. for the binning
// counts -- and not for the whole stream, so the render kernels queued behind the copy keep
// the GPU busy while the host returns to Python and queues the backward.
// The slot is coherent and mapped, and by default K2 stores the count into it itself
// (`dev`), so no copy is queued behind K2; the "host_total" option 0 selects the copy.
struct TotalReadback {
    unsigned long long* host = nullptr;
    unsigned long long* mapped = nullptr;  // device view of `host`
    unsigned long long* dev = nullptr;     // `mapped` when the kernels store the count, null: copy instead
    hipEvent_t ev = nullptr;
};
bool host_total_store() { return option(OPT_HOST_TOTAL) != 0; }
int total_readback(TotalReadback** out, bool kernel_store) {
    constexpr int kMaxDevices = 64;
    thread_local TotalReadback slots[kMaxDevices];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices)
        return fail(GSR_ERR_HIP, "num_rendered readback: no current device");
    TotalReadback& r = slots[dev];
    if (!r.host) {
        // always mapped + coherent, so the "host_total" option can switch between the kernels'
        // own store (dev) and a queued copy (readback_dev() == null) from one call to the next
        void* h = nullptr;
        if (hipHostMalloc(&h, sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
            return fail(GSR_ERR_HIP, "num_rendered readback: hipHostMalloc failed");
        void* d = nullptr;
        if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
            (void)hipHostFree(h);
            return fail(GSR_ERR_HIP, "num_rendered readback: hipHostGetDevicePointer failed");
        }
        if (hipEventCreateWithFlags(&r.ev, hipEventDisableTiming) != hipSuccess) {
            (void)hipHostFree(h);
            return fail(GSR_ERR_HIP, "num_rendered readback: hipEventCreate failed");
        }
        r.host = (unsigned long long*)h;
        r.mapped = (unsigned long long*)d;
    }
    r.dev = kernel_store ? r.mapped : nullptr;
    *out = &r;
    return GSR_OK;
}

// The forward's wait for its instance count ("count_wait" option).  1: poll the event from this
// thread (up to kCountSpinMs, then block) -- the count lands ~0.6 ms after the call starts, while
// the GPU still has the previous backward and this forward's binning to run, and a blocking wait
// sleeps until the completion interrupt wakes the thread; on a busy host that wake-up was seen to
// take 2 ms (bench slow_steps, r3y4), idling a GPU whose queue holds only the 0.27 ms of sort and
// render behind the count.  0: hipEventSynchronize (HIP's short active wait, then the interrupt).
// The poll spins for kCountSpinUs, then yields the core between queries (std::this_thread::yield:
// returns at once when nothing else wants the core, so a lone rank still sees the count within a
// query's latency, while eight ranks per node plus RCCL proxy and loader threads get the cores
// they need), and after kCountSpinMs falls back to the blocking wait.
constexpr int kCountSpinMs = 20;
constexpr int kCountSpinUs = 100;
hipError_t wait_count_event(hipEvent_t ev, bool poll) {
    if (poll) {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            const hipError_t q = hipEventQuery(ev);
            if (q != hipErrorNotReady) return q;
            const auto dt = std::chrono::steady_clock::now() - t0;
            if (dt > std::chrono::milliseconds(kCountSpinMs)) break;
            if (dt > std::chrono::microseconds(kCountSpinUs)) std::this_thread::yield();
        }
    }
    return hipEventSynchronize(ev);
}

// "count_wait" 2: poll the mapped count slot until it leaves `pending` (the kernel's system-scope
// store), with the same spin-then-yield pacing; after kCountSlotMs the stream itself is waited for
// (a stalled or faulted stream then reports its error instead of the poll spinning on).
constexpr int kCountSlotMs = 2000;
hipError_t wait_count_slot(const unsigned long long* slot, unsigned long long pending, hipStream_t stream) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        if (__atomic_load_n(slot, __ATOMIC_ACQUIRE) != pending) return hipSuccess;
        const auto dt = std::chrono::steady_clock::now() - t0;
        if (dt > std::chrono::milliseconds(kCountSlotMs)) break;
        if (dt > std::chrono::microseconds(kCountSpinUs)) std::this_thread::yield();
    }
    return hipStreamSynchronize(stream);
}

// Forwards whose capacity hint was too small (the binning stage was redone), for gsr_forward_rebuilds().
std::atomic<long long> g_rebuilds{0};
// Host-side statistics (gsr_host_stats): time the forwards waited for their instance count, and
// the host time of whole forward / backward calls.
struct HostStat {
    std::atomic<long long> ns{0}, calls{0}, max_ns{0};
    void add(long long v) {
        ns.fetch_add(v, std::memory_order_relaxed);
        calls.fetch_add(1, std::memory_order_relaxed);
        long long prev = max_ns.load(std::memory_order_relaxed);
        while (v > prev && !max_ns.compare_exchange_weak(prev, v, std::memory_order_relaxed)) {}
    }
    void reset() {
        ns.store(0, std::memory_order_relaxed);
        calls.store(0, std::memory_order_relaxed);
        max_ns.store(0, std::memory_order_relaxed);
    }
};
HostStat g_wait, g_fwd_host, g_bwd_host;
struct HostTimer {  // adds the scope's host time to a HostStat
    HostStat& st;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit HostTimer(HostStat& s) : st(s) {}
    ~HostTimer() {
        st.add((long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0)
                   .count());
    }
};

}  // namespace

extern "C" {

const char* gsr_last_error(void) { return g_err; }

const char* gsr_version(void) { return "gsr 0.2.0 gfx950"; }

#ifndef GSR_BUILD_ID
#define GSR_BUILD_ID "unknown"
#endif
const char* gsr_build_id(void) { return GSR_BUILD_ID; }

long long gsr_forward_rebuilds(void) { return g_rebuilds.load(std::memory_order_relaxed); }

int gsr_host_stats(double* values, int n, int reset) {
    const HostStat* st[3] = {&g_wait, &g_fwd_host, &g_bwd_host};
    for (int k = 0; k < 3; k++)
        for (int j = 0; j < 3; j++) {
            const int i = 3 * k + j;
            if (!values || i >= n) continue;
            values[i] = j == 0 ? (double)st[k]->calls.load(std::memory_order_relaxed)
                               : (double)(j == 1 ? st[k]->ns : st[k]->max_ns).load(std::memory_order_relaxed) * 1e-6;
        }
    if (reset)
        for (auto* p : {&g_wait, &g_fwd_host, &g_bwd_host}) p->reset();
    return GSR_OK;
}

int gsr_option_set(const char* name, int value) {
    clear_error();
    const int i = option_index(name);
    if (i < 0) return fail(GSR_ERR_ARGUMENT, "option_set: unknown option '%s'", name ? name : "(null)");
    const OptionSpec& o = kOptions[i];
    if (value < o.lo || value > o.hi || (i == OPT_FWD_QUADS && value != 2 && value != 4))
        return fail(GSR_ERR_ARGUMENT, "option_set: %s = %d out of range [%d, %d]", name, value, o.lo, o.hi);
    options_init();
    g_opt[i].store(value, std::memory_order_relaxed);
    return GSR_OK;
}

int gsr_option_get(const char* name) {
    const int i = option_index(name);
    return i < 0 ? -1 : option(i);
}

int gsr_option_set_thread(const char* name, int value) {
    clear_error();
    const int i = option_index(name);
    if (i < 0) return fail(GSR_ERR_ARGUMENT, "option_set_thread: unknown option '%s'", name ? name : "(null)");
    const OptionSpec& o = kOptions[i];
    if (value < o.lo || value > o.hi || (i == OPT_FWD_QUADS && value != 2 && value != 4))
        return fail(GSR_ERR_ARGUMENT, "option_set_thread: %s = %d out of range [%d, %d]", name, value, o.lo, o.hi);
    t_opt[i] = value;
    return GSR_OK;
}

int gsr_option_clear_thread(const char* name) {
    clear_error();
    if (!name) {
        for (int i = 0; i < OPT_COUNT; i++) t_opt[i] = kOptNone;
        return GSR_OK;
    }
    const int i = option_index(name);
    if (i < 0) return fail(GSR_ERR_ARGUMENT, "option_clear_thread: unknown option '%s'", name);
    t_opt[i] = kOptNone;
    return GSR_OK;
}

int gsr_geom_forget(const void* geom_buffer) {
    clear_error();
    geom_forget(geom_buffer);
    return GSR_OK;
}

int gsr_census_set(void* device_counters) {
    g_census = reinterpret_cast<unsigned long long*>(device_counters);
    return GSR_OK;
}

int gsr_profile_enable(int stage_mask) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    g_prof.mask = (unsigned)stage_mask;
    return GSR_OK;
}

void gsr_profile_reset(void) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    for (auto& p : g_prof.pending) {
        g_prof.pool.push_back(p.a);
        g_prof.pool.push_back(p.b);
    }
    g_prof.pending.clear();
    for (int i = 0; i < ST_COUNT; i++) {
        g_prof.total_ms[i] = 0;
        g_prof.calls[i] = 0;
    }
}

int gsr_profile_collect(double* total_ms, long long* calls, int max_stages) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    for (auto& p : g_prof.pending) {
        (void)hipEventSynchronize(p.b);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            g_prof.total_ms[p.stage] += ms;
            g_prof.calls[p.stage] += 1;
        }
        g_prof.pool.push_back(p.a);
        g_prof.pool.push_back(p.b);
    }
    g_prof.pending.clear();
    for (int i = 0; i < ST_COUNT && i < max_stages; i++) {
        if (total_ms) total_ms[i] = g_prof.total_ms[i];
        if (calls) calls[i] = g_prof.calls[i];
    }
    return ST_COUNT;
}

const char* gsr_profile_stage_name(int stage) {
    return (stage >= 0 && stage < ST_COUNT) ? kStageNames[stage] : "";
}

int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     unsigned char* present, void* stream) {
    (void)projmatrix;  // checkFrustum computes the projection but only tests view-space z
    clear_error();
    if (P < 0) return fail(GSR_ERR_ARGUMENT, "mark_visible: P must be >= 0");
    if (P == 0) return GSR_OK;
    if (!means3D || !viewmatrix || !present) return fail(GSR_ERR_ARGUMENT, "mark_visible: null pointer");
    HIP_TRY(gsr::launch_mark_visible(P, means3D, viewmatrix, reinterpret_cast<bool*>(present), (hipStream_t)stream),
            "mark_visible");
    return GSR_OK;
}

namespace {
// The struct_size rule of include/gsr.h: nothing but that field is read from a struct of another size.
int check_struct(const char* who, const void* args, size_t got, size_t want) {
    if (!args) return fail(GSR_ERR_ARGUMENT, "%s: null argument struct", who);
    if (got != want)
        return fail(GSR_ERR_ARGUMENT, "%s: struct_size %zu is not this library's %zu (built from another gsr.h?)", who,
                    got, want);
    return GSR_OK;
}

int forward_impl(gsr_forward_args* args) {
    using namespace gsr;
    HostTimer host_time(g_fwd_host);
    clear_error();
    if (int rc = check_struct("rasterize_forward", args, args ? args->struct_size : 0, sizeof(gsr_forward_args)))
        return rc;
    const gsr_scene& scene = args->scene;
    const gsr_view& view = args->view;
    const int P = scene.P, D = scene.D, width = view.width, height = view.height;
    const float *means3D = scene.means3D, *dc = scene.dc, *shs = scene.shs, *colors_precomp = scene.colors_precomp,
                *opacities = scene.opacities, *scales = scene.scales, *rotations = scene.rotations,
                *cov3D_precomp = scene.cov3D_precomp;
    const float scale_modifier = scene.scale_modifier, tan_fovx = view.tan_fovx, tan_fovy = view.tan_fovy;
    const float *background = view.background, *viewmatrix = view.viewmatrix, *projmatrix = view.projmatrix,
                *cam_pos = view.campos;
    const int antialiasing = view.antialiasing, prefiltered = args->prefiltered, debug = args->debug,
              capacity_hint = args->capacity_hint;
    const gsr_alloc_fn geom_alloc = args->geom_alloc, binning_alloc = args->binning_alloc,
                       image_alloc = args->image_alloc;
    void *const geom_ctx = args->geom_ctx, *const binning_ctx = args->binning_ctx, *const image_ctx = args->image_ctx;
    float *const out_color = args->out_color, *const out_invdepth = args->out_invdepth;
    int* const radii = args->radii;
    hipStream_t stream = (hipStream_t)args->stream;
    // every option is read ONCE per call: gsr_option_set may run on another thread, and the launches
    // of one forward (K4's prefix and the redo, the render's part protocol, the work list's segment
    // length) must agree with each other
    const int opt_quads = option(OPT_FWD_QUADS), opt_seg_ck = option(OPT_BWD_SEG_CK);
    const uint32_t opt_prefix = (uint32_t)option(OPT_SORT_PREFIX);
    const bool opt_fused = fused_binning_mode(), opt_host_total = host_total_store();
    const int opt_count_wait = option(OPT_COUNT_WAIT);
    const bool opt_atomic = option(OPT_BWD_ATOMIC) != 0;
    // K3 writes the record path's inputs only when this forward's backwards may take it without a prep
    const bool k3_recs = !opt_atomic;
    const int opt_near_mass = option(OPT_NEAR_MASS);
    // the binning buffer is laid out for a multiple of kCapQuantum (the backward recovers it from the
    // buffer's size); only a capacity whose rounding passes INT_MAX keeps the exact layout
    const auto capacity_for = [](size_t c) {
        const size_t q = quantize_capacity(c);
        return q <= (size_t)INT_MAX ? q : c;
    };
    args->num_rendered = 0;
    args->binning_capacity = 0;
    if (P < 0 || width <= 0 || height <= 0)
        return fail(GSR_ERR_ARGUMENT, "rasterize_forward: invalid sizes P=%d W=%d H=%d", P, width, height);
    if (P >= kMaxGaussians)
        return fail(GSR_ERR_ARGUMENT, "rasterize_forward: P=%d exceeds the tile-list entry limit %d", P,
                    kMaxGaussians - 1);
    if (P == 0) return GSR_OK;  // RI/rasterize_points.cu:108: nothing is launched
    if (!means3D || !opacities || !viewmatrix || !projmatrix || !background || !out_color || !out_invdepth || !radii)
        return fail(GSR_ERR_ARGUMENT, "rasterize_forward: missing required input");
    if (!colors_precomp && !shs && !dc)
        return fail(GSR_ERR_ARGUMENT, "rasterize_forward: provide either SHs or precomputed colours");
    if (dc && scene.M > 0 && !shs)
        return fail(GSR_ERR_ARGUMENT, "rasterize_forward: %d rest SH coefficients but no shs", scene.M);
    const int M = dc ? scene.M + 1 : scene.M;  // split layout: scene.M counts the rest; the kernels see dc as coefficient 0
    if (!cov3D_precomp && (!scales || !rotations))
        return fail(GSR_ERR_ARGUMENT, "rasterize_forward: provide scales+rotations or a precomputed covariance");
    if (!colors_precomp && (D < 0 || D > 3 || (D + 1) * (D + 1) > M))
        return fail(GSR_ERR_ARGUMENT, "rasterize_forward: SH degree %d needs %d coefficients, got %d", D,
                    (D + 1) * (D + 1), M);
    if (!colors_precomp && !cam_pos) return fail(GSR_ERR_ARGUMENT, "rasterize_forward: campos required for SHs");

    const float focal_y = height / (2.0f * tan_fovy);  // CR/rasterizer_impl.cu:253-254
    const float focal_x = width / (2.0f * tan_fovx);
    const uint32_t gx = (width + kTile - 1) / kTile, gy = (height + kTile - 1) / kTile;
    const uint32_t tiles = gx * gy;
    if (gx > 65535u || gy > 65535u)
        return fail(GSR_ERR_ARGUMENT, "rasterize_forward: image of %dx%d has more than 65535 tile columns/rows",
                    width, height);
    // the binning's instance walk divides tile offsets inside a rectangle in fp32 (exact below 2^21,
    // binning.hip for_each_instance): a 536-Mpx frame, far beyond any camera
    constexpr size_t kMaxTiles = size_t(1) << 21;
    if ((size_t)gx * gy >= kMaxTiles)
        return fail(GSR_ERR_ARGUMENT, "rasterize_forward: image of %dx%d has %zu tiles (the limit is %zu)", width,
                    height, (size_t)gx * gy, kMaxTiles - 1);

    size_t geom_bytes = 0, img_bytes = 0;
    carve_geom(nullptr, P, gx, gy, &geom_bytes);
    char* gbase = (char*)call_alloc(geom_alloc, geom_ctx, geom_bytes);
    if (!gbase) return fail(GSR_ERR_ALLOC, "rasterize_forward: geometry buffer allocation failed");
    GeomState geom = carve_geom(gbase, P, gx, gy, &geom_bytes);
    geom_mark(gbase, false, false, false, false);  // (set below once the binning and the render's fill blocks are queued)
    carve_image(nullptr, width, height, tiles, &img_bytes);
    char* ibase = (char*)call_alloc(image_alloc, image_ctx, img_bytes);
    if (!ibase) return fail(GSR_ERR_ALLOC, "rasterize_forward: image buffer allocation failed");
    ImageState img = carve_image(ibase, width, height, tiles, &img_bytes);

    if (prefiltered) HIP_TRY(hipMemsetAsync(geom.status, 0, 4 * sizeof(uint32_t), stream), "status init");
    {
        StageScope sc(ST_PREPROCESS, stream);
        PreprocessArgs pa{};
        pa.P = P; pa.D = D; pa.M = M; pa.W = width; pa.H = height;
        pa.means3D = means3D; pa.scales = scales; pa.scale_modifier = scale_modifier; pa.rotations = rotations;
        pa.opacities = opacities; pa.shs = colors_precomp || M <= (dc ? 1 : 0) ? nullptr : shs;
        pa.dc = colors_precomp ? nullptr : dc; pa.cov3D_precomp = cov3D_precomp;
        pa.colors_precomp = colors_precomp; pa.viewmatrix = viewmatrix; pa.projmatrix = projmatrix;
        pa.campos = cam_pos; pa.tan_fovx = tan_fovx; pa.tan_fovy = tan_fovy; pa.focal_x = focal_x;
        pa.focal_y = focal_y; pa.gx = gx; pa.gy = gy; pa.prefiltered = prefiltered; pa.antialiasing = antialiasing;
        pa.footprint_cull = (width < 32000 && height < 32000) ? 1 : 0;
        pa.radii = radii; pa.geom = geom;
        pa.zero = geom.tile_cnt;  // tile, cell and near counters and the depth-mass histogram (binning.hip), contiguous
        pa.zero_n = (uint32_t)bin_zero_words(tiles, bin_cell_count(gx, gy));
        HIP_TRY(launch_preprocess(pa, stream), "preprocess");
    }
    if (int rc = check_debug(debug, stream, "preprocess")) return rc;
    if (prefiltered) {
        uint32_t st = 0;
        HIP_TRY(hipMemcpyAsync(&st, geom.status, sizeof(uint32_t), hipMemcpyDeviceToHost, stream), "status copy");
        HIP_TRY(hipStreamSynchronize(stream), "status sync");
        if (st & 1u)
            return fail(GSR_ERR_PREFILTERED,
                        "Point is filtered although prefiltered is set. This shouldn't happen! (CR/auxiliary.h:184)");
    }
    // exact mode: counts first (ranges unclamped), then the host reads R
    const size_t kNoCap = ~(size_t)0;
    TotalReadback* rb = nullptr;
    if (int rc = total_readback(&rb, opt_host_total)) return rc;
    // capacity mode: the binning buffer's capacity, known up front (the ranges are clamped to it)
    const size_t C_hint = capacity_hint > 0 ? capacity_for((size_t)capacity_hint) : 0;
    // capacity mode with LDS cursors: K2 folded into K3 (binning.hip FusedScan)
    const bool fused = capacity_hint > 0 && bin_fused_ok(tiles) && opt_fused;
    // near-first binning (binning.hip): the depth cut's target, mass x kMassScale over the image.  Only for frames
    // whose lists are long (a mean of kNearMinMeanList entries by the capacity hint, the reachable-prefix sort's
    // regime): there the blend reaches a small part of each list and the cut pays; with short lists (1M@1080p:
    // 973) the frame's mass stays under the target anyway, and the redo chain's launches (far fill, whole
    // sort, redo render: ~6 us when empty) would only cost (r5d: 0.7305 -> 0.7372-0.7404 ms with no cut made)
    constexpr size_t kNearMinMeanList = kLongMeanList;
    const unsigned long long near_target =
        fused && opt_near_mass > 0 && bin_near_ok(tiles) && C_hint >= kNearMinMeanList * (size_t)tiles
            ? (unsigned long long)opt_near_mass * (unsigned long long)kMassScale * (unsigned long long)width * height
            : 0ull;
    const bool near_first = near_target > 0;
    // "count_wait" 2 (capacity mode, the kernels storing the count into the mapped slot): no event
    // behind the count -- the host polls the slot itself, reset to a sentinel before the launch that
    // stores it, so the stream carries no marker (an event's marker left the GPU idle ~6 us between
    // the scatter and the sort, r4a trace)
    const bool poll_slot = opt_count_wait == 2 && capacity_hint > 0 && rb->dev;
    constexpr unsigned long long kSlotPending = ~0ull;
    if (poll_slot) __atomic_store_n(rb->host, kSlotPending, __ATOMIC_RELEASE);
    {
        StageScope sc(ST_BIN_COUNT, stream);
        HIP_TRY(launch_bin_count(P, geom, gx, gy, img.ranges, capacity_hint > 0 ? C_hint : kNoCap,
                                 fused ? nullptr : rb->dev, stream, fused, near_target),
                "bin_count");
    }
    if (int rc = check_debug(debug, stream, "bin_count")) return rc;

    // Scatter + tile sort + render into a binning buffer of capacity C.  In exact mode
    // C = R is read back first -- the reference's one host synchronisation
    // (CR/rasterizer_impl.cu:313).  In capacity mode (capacity_hint > 0) nothing waits
    // for the host: every stage is queued, then the host waits for the copy of R queued
    // right behind K2 (not for the render behind it), and if R exceeds C the lists are
    // rebuilt into a buffer of exactly R.
    // mark num_rendered (K2 stores it into the host slot, or a copy is queued); wait_total()
    // waits for that mark only
    auto queue_total = [&]() -> int {
        if (poll_slot) return GSR_OK;
        if (!rb->dev)
            HIP_TRY(hipMemcpyAsync(rb->host, geom.total, sizeof(*rb->host), hipMemcpyDeviceToHost, stream),
                    "num_rendered copy");
        HIP_TRY(hipEventRecord(rb->ev, stream), "num_rendered event");
        return GSR_OK;
    };
    auto wait_total = [&](unsigned long long* total) -> int {
        hipError_t we;
        {
            HostTimer ht(g_wait);
            we = poll_slot ? wait_count_slot(rb->host, kSlotPending, stream)
                           : wait_count_event(rb->ev, opt_count_wait != 0);
        }
        HIP_TRY(we, "num_rendered sync");
        *total = __atomic_load_n(rb->host, __ATOMIC_ACQUIRE);
        if (*total == kSlotPending)
            return fail(GSR_ERR_HIP, "rasterize_forward: the stream finished without storing the instance count");
        if (*total > (unsigned long long)INT_MAX)
            return fail(GSR_ERR_OVERFLOW, "rasterize_forward: %llu tile instances exceed INT_MAX", *total);
        return GSR_OK;
    };
    auto bin_and_render = [&](size_t C, bool fused_now) -> int {
        size_t bin_bytes = 0;
        carve_binning(nullptr, C, &bin_bytes);
        char* bbase = (char*)call_alloc(binning_alloc, binning_ctx, bin_bytes);
        if (!bbase) return fail(GSR_ERR_ALLOC, "rasterize_forward: binning buffer allocation failed");
        BinningState bin = carve_binning(bbase, C, &bin_bytes);
        const uint32_t prefix = C > 0 ? sort_prefix_for(C, tiles, opt_prefix) : 0u;  // K4 and the redo agree
        {
            // always launched: besides the keys (none when C == 0) it writes every Gaussian's
            // first record index, which the backward's reduction reads even when nothing
            // was rendered (fused: also the ranges, classes and the count)
            StageScope sc(ST_BIN_SCATTER, stream);
            HIP_TRY(launch_bin_scatter(P, geom, gx, gy, bin, C, stream, img.ranges, fused_now ? rb->dev : nullptr,
                                       fused_now, fused_now && near_first, k3_recs),
                    "bin_scatter");
        }
        if (fused_now)
            if (int rc = queue_total()) return rc;
        if (int rc = check_debug(debug, stream, "bin_scatter")) return rc;
        if (C > 0) {
            {
                StageScope sc(ST_TILE_SORT, stream);
                // (near-first binning: K4 sorts each tile's near entries, GeomState::sranges)
                HIP_TRY(launch_tile_sort(tiles, fused_now && near_first ? geom.sranges : img.ranges, geom, bin, C,
                                         stream, fused_now,
                                         (uint32_t)bin_cell_count(gx, gy), prefix),
                        "tile_sort");
            }
            if (int rc = check_debug(debug, stream, "tile_sort")) return rc;
        }
        {
            StageScope sc(ST_RENDER_FWD, stream);
            RenderFwdArgs ra{};
            ra.W = width; ra.H = height; ra.gx = gx; ra.gy = gy; ra.ranges = img.ranges;
            ra.gid_sorted = bin.gid_sorted; ra.rec = geom.rec; ra.bg = background;
            ra.out_color = out_color; ra.out_invdepth = out_invdepth; ra.ckpt = bin.ckpt; ra.img = img;
            ra.unit_cnt = geom.unit_cnt; ra.unit_part = geom.unit_part; ra.unit_full = bin.unit_full;
            ra.full_cap = (uint32_t)unit_full_cap(C);
            ra.tile_join = geom.tile_join;
            ra.seg_ck = opt_seg_ck;
            ra.seg_ck_out = geom.fwd_seg_ck;
            ra.fault = geom.status + 1;
            ra.census = g_census;
            ra.sorted_len = geom.sorted_len;
            ra.redo_flag = geom.redo_flag;
            ra.redo_list = geom.redo_list;
            ra.redo_cnt = geom.redo_cnt;
            // (C == 0: no lists and no K4, so nothing is prefix-sorted and no redo state was reset)
            if (C == 0) ra.sorted_len = nullptr;
            if (opt_atomic) {  // the atomic backward's accumulator rows and touched bits, zeroed beside the render
                ra.acc = geom.acc;
                ra.touched = geom.touched;
                ra.depth_key = geom.depth_key;
                ra.zcut = geom.zcut;
                ra.n_gauss = (uint32_t)P;
                ra.fill_blocks = kFwdFillBlocks;
            }
            HIP_TRY(launch_render_fwd(ra, stream, opt_quads), "render_fwd");
            // (launch_render_fwd: the whole-tile kernel runs for fwd_quads = 4 without the census only)
            geom_mark(gbase, opt_atomic, k3_recs, (size_t)C >= kLongMeanList * (size_t)tiles,
                      !(opt_quads == 4 && !g_census));
            const bool near_now = fused_now && near_first;
            if ((prefix || near_now) && C > 0) {  // the tiles whose walk passed their sorted prefix (usually none)
                if (near_now)  // their far instances first (none emitted by K3); their accumulator rows zeroed
                    HIP_TRY(launch_far_fill(P, geom, gx, tiles, img.ranges, bin, C, true, stream,
                                            opt_atomic ? geom.acc : nullptr),
                            "render_fwd far fill");
                HIP_TRY(launch_tile_sort_redo(tiles, img.ranges, geom, bin, C, stream), "render_fwd redo sort");
                HIP_TRY(launch_render_fwd_redo(ra, stream, opt_quads), "render_fwd redo");
            }
        }
        return check_debug(debug, stream, "render_fwd");
    };

    unsigned long long total = 0;
    size_t C = 0;
    if (!fused)
        if (int rc = queue_total()) return rc;
    if (capacity_hint <= 0) {
        if (int rc = wait_total(&total)) return rc;
        C = capacity_for((size_t)total);
        if (int rc = bin_and_render(C, false)) return rc;
    } else {
        // everything is queued before the host waits, and it waits for the counts only
        C = C_hint;
        if (int rc = bin_and_render(C, fused)) return rc;
        if (int rc = wait_total(&total)) return rc;
        if (total > C) {  // the hint was too small: recount (resets the cursors) and rebuild exactly
            g_rebuilds.fetch_add(1, std::memory_order_relaxed);
            C = capacity_for((size_t)total);
            if (fused)  // (the fused sort re-zeroes the counters only when it ran: C > 0)
                HIP_TRY(hipMemsetAsync(geom.tile_cnt, 0, sizeof(uint32_t) * bin_zero_words(tiles, bin_cell_count(gx, gy)),
                                       stream),
                        "bin counters");
            HIP_TRY(launch_bin_count(P, geom, gx, gy, img.ranges, C, nullptr, stream), "bin_count");
            if (int rc = bin_and_render(C, false)) return rc;
        }
    }
    args->num_rendered = (int)total;
    args->binning_capacity = (int)C;
    return GSR_OK;
}
}  // namespace

int gsr_rasterize_forward(gsr_forward_args* args) { return forward_impl(args); }

namespace {
// The backward's dense outputs are zero-filled on a side stream that runs beside render_bwd
// (VALU-bound: HBM is two-thirds idle under it); gauss_bwd then writes only the rows of
// Gaussians with a non-zero render gradient (about 14% of a 1M@1080p view).  "zero_fill" option:
// 3 (default) fill blocks in render_bwd's own launch (no events: each fork / join event left the GPU
// idle for 6-7 us, r4a), 1 side stream, 2 main stream right before gauss_bwd, 0 gauss_bwd writes
// every row.
// "live_list": gauss_bwd over the list of Gaussians with a gradient (1, default) or a lane per
// Gaussian (0), when the outputs are zero-filled.
bool live_list_mode() { return option(OPT_LIVE_LIST) != 0; }
int zero_fill_mode() { return option(OPT_ZERO_FILL); }

struct SideStream {
    std::mutex mu;  // one backward at a time per device uses the pair of events
    hipStream_t s = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    bool ok = false;
};

SideStream* side_stream() {
    static SideStream ss[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    SideStream& r = ss[dev];
    std::lock_guard<std::mutex> lk(r.mu);
    if (!r.ok && !r.s) {
        r.ok = hipStreamCreateWithFlags(&r.s, hipStreamNonBlocking) == hipSuccess &&
               hipEventCreateWithFlags(&r.fork, hipEventDisableTiming) == hipSuccess &&
               hipEventCreateWithFlags(&r.join, hipEventDisableTiming) == hipSuccess;
    }
    return r.ok ? &r : nullptr;
}

int backward_impl(const gsr_backward_args* args) {
    using namespace gsr;
    HostTimer host_time(g_bwd_host);
    clear_error();
    if (int rc = check_struct("rasterize_backward", args, args ? args->struct_size : 0, sizeof(gsr_backward_args)))
        return rc;
    const gsr_scene& scene = args->scene;
    const gsr_view& view = args->view;
    const int P = scene.P, D = scene.D, R = args->R, width = view.width, height = view.height;
    const float *means3D = scene.means3D, *dc = scene.dc, *shs = scene.shs, *colors_precomp = scene.colors_precomp,
                *opacities = scene.opacities, *scales = scene.scales, *rotations = scene.rotations,
                *cov3D_precomp = scene.cov3D_precomp;
    const float scale_modifier = scene.scale_modifier, tan_fovx = view.tan_fovx, tan_fovy = view.tan_fovy;
    const float *background = view.background, *viewmatrix = view.viewmatrix, *projmatrix = view.projmatrix,
                *campos = view.campos;
    const int antialiasing = view.antialiasing, debug = args->debug, binning_capacity = args->binning_capacity;
    const size_t binning_bytes = args->binning_bytes;
    const int* radii = args->radii;
    void *const geom_buffer = args->geom_buffer, *const binning_buffer = args->binning_buffer,
                *const image_buffer = args->image_buffer;
    const float *dL_dpix = args->dL_dpix, *dL_dinvdepths = args->dL_dinvdepths, *dL_dalphas = args->dL_dalphas;
    float *const dL_dmean2D = args->dL_dmean2D, *const dL_dmean2D_abs = args->dL_dmean2D_abs,
                 *const dL_dconic = args->dL_dconic, *const dL_dopacity = args->dL_dopacity,
                 *const dL_dcolor = args->dL_dcolor, *const dL_dinvdepth = args->dL_dinvdepth,
                 *const dL_dmean3D = args->dL_dmean3D, *const dL_dcov3D = args->dL_dcov3D,
                 *const dL_ddc = args->dL_ddc, *const dL_dsh = args->dL_dsh, *const dL_dscale = args->dL_dscale,
                 *const dL_drot = args->dL_drot, *const view_block = args->view_block;
    const gsr_alloc_fn scratch_alloc = args->scratch_alloc;
    void* const scratch_ctx = args->scratch_ctx;
    hipStream_t stream = (hipStream_t)args->stream;
    // view_block: screen-space backward only -- the render-gradient sums, flags and camera go into the block
    // (the multi-GPU view exchange) and the per-Gaussian backward, with its outputs, is skipped
    const bool screen = view_block != nullptr;
    if (screen) {
        if ((reinterpret_cast<uintptr_t>(view_block) & 15) != 0)
            return fail(GSR_ERR_ARGUMENT, "rasterize_backward_screen: view block must be 16-byte aligned");
        if (colors_precomp || cov3D_precomp)  // (per view: the exchange's per-Gaussian backward has neither)
            return fail(GSR_ERR_ARGUMENT, "rasterize_backward_screen: precomputed colours / cov3D with a view block");
    }
    if (P < 0 || R < 0 || width <= 0 || height <= 0)
        return fail(GSR_ERR_ARGUMENT, "rasterize_backward: invalid sizes P=%d R=%d W=%d H=%d", P, R, width, height);
    if (P == 0) return GSR_OK;
    if (!geom_buffer || !image_buffer || (R > 0 && !binning_buffer))
        return fail(GSR_ERR_ARGUMENT, "rasterize_backward: missing forward buffers");
    if (!means3D || !opacities || !radii || !dL_dpix || !viewmatrix || !projmatrix || !background || !campos)
        return fail(GSR_ERR_ARGUMENT, "rasterize_backward: missing required pointer");
    if (!screen) {
        if (!dL_dmean2D || !dL_dopacity || !dL_dcolor || !dL_dmean3D || !dL_dcov3D)
            return fail(GSR_ERR_ARGUMENT, "rasterize_backward: missing required output");
        if (!colors_precomp && shs && !dL_dsh)
            return fail(GSR_ERR_ARGUMENT, "rasterize_backward: SH gradient needs dL_dsh");
        if (!colors_precomp && dc && !dL_ddc)
            return fail(GSR_ERR_ARGUMENT, "rasterize_backward: dc gradient needs dL_ddc");
        if (scales && (!rotations || !dL_dscale || !dL_drot))
            return fail(GSR_ERR_ARGUMENT, "rasterize_backward: scale/rotation gradients need outputs");
        if ((dL_dinvdepths == nullptr) != (dL_dinvdepth == nullptr))
            return fail(GSR_ERR_ARGUMENT, "rasterize_backward: dL_dinvdepths and dL_dinvdepth go together");
    }
    if (dc && scene.M > 0 && !shs)
        return fail(GSR_ERR_ARGUMENT, "rasterize_backward: %d rest SH coefficients but no shs", scene.M);
    if (dL_dmean2D_abs && screen)
        return fail(GSR_ERR_ARGUMENT, "rasterize_backward: the view-block backward has no absolute gradient");
    if (dL_dmean2D_abs && g_census)  // (render_bwd has no CENSUS x ABSGRAD instantiation)
        return fail(GSR_ERR_ARGUMENT, "rasterize_backward: dL_dmean2D_abs cannot be combined with the census");
    const int M = dc ? scene.M + 1 : scene.M;  // as in the forward
    if (!colors_precomp && (shs || dc) && (D < 0 || D > 3 || (D + 1) * (D + 1) > M))
        return fail(GSR_ERR_ARGUMENT, "rasterize_backward: SH degree %d needs %d coefficients, got %d", D,
                    (D + 1) * (D + 1), M);

    const float focal_y = height / (2.0f * tan_fovy);
    const float focal_x = width / (2.0f * tan_fovx);
    const uint32_t gx = (width + kTile - 1) / kTile, gy = (height + kTile - 1) / kTile;
    const uint32_t tiles = gx * gy;
    // the binning buffer is laid out for the capacity the forward used (>= R): given, or
    // recovered from the buffer's size (resolve_capacity)
    size_t C = 0;
    if (!resolve_capacity(R, binning_capacity, binning_bytes, &C))
        return fail(GSR_ERR_ARGUMENT,
                    "rasterize_backward: a binning buffer of %zu bytes matches no layout for R=%d (capacity %d)",
                    binning_bytes, R, binning_capacity);
    if (C < (size_t)R) return fail(GSR_ERR_ARGUMENT, "rasterize_backward: binning capacity %zu < R=%d", C, R);
    size_t tmp = 0;
    GeomState geom = carve_geom((char*)geom_buffer, P, gx, gy, &tmp);
    ImageState img = carve_image((char*)image_buffer, width, height, tiles, &tmp);
    BinningState bin = carve_binning((char*)binning_buffer, C, &tmp);
    size_t rec_bytes = 0;
    GradRecs recs{}, sums{};
    // the forward recorded the segment length its work list uses (GeomState::fwd_seg_ck); the grid is
    // sized for the shortest segments (seg_ck = 1), so it covers whatever the forward used
    const size_t max_units = R > 0 ? bwd_max_units((size_t)R, tiles, 1) : 0;
    uint32_t *live = nullptr, *live_count = nullptr;
    // the options, each read once
    const int zmode = screen ? 0 : zero_fill_mode();
    const int grid_mode = option(OPT_BWD_GRID);
    // With the outputs zero-filled, gauss_bwd walks a list of the Gaussians with a gradient
    // (~13% of a 1M@1080p view) that gauss_reduce appends to, instead of a lane per Gaussian.
    const bool use_list = zmode != 0 && live_list_mode();
    // atomic backward: per-Gaussian rows (zeroed by the forward, which marked its buffer) instead of records +
    // gauss_reduce; it needs the live list, or a view block (gauss_live_views writes the block's sums and flags);
    // the record path serves every other mode
    const GeomMark mark = geom_marked(geom_buffer);
    const bool atomic = (screen || use_list) && R > 0 && option(OPT_BWD_ATOMIC) != 0 && mark.zeroed;
    // (the atomic backward writes no per-instance records: no record scratch)
    const size_t R_recs = atomic ? 0 : (size_t)R;
    carve_recs(nullptr, R_recs, (size_t)P, &recs, &sums, &live, &live_count, &rec_bytes);
    char* rbase = (char*)call_alloc(scratch_alloc, scratch_ctx, rec_bytes);
    if (!rbase) return fail(GSR_ERR_ALLOC, "rasterize_backward: scratch allocation failed");
    carve_recs(rbase, R_recs, (size_t)P, &recs, &sums, &live, &live_count, &rec_bytes);
    uint32_t* flags = nullptr;
    if (screen) {  // the sums and flags go to the view block (gsr_common.h "View block")
        float* body = view_block + kViewBlockHeader;
        sums.a = reinterpret_cast<float4*>(body);
        sums.b = reinterpret_cast<float4*>(body + 4 * (size_t)P);
        sums.c = reinterpret_cast<float2*>(body + 8 * (size_t)P);
        flags = reinterpret_cast<uint32_t*>(body + 10 * (size_t)P);
    }

    // dense outputs to zero-fill (gauss_bwd then writes only the non-zero rows)
    FillArgs fill{};
    const int m_rest = dc ? M - 1 : M;
    static_assert(kFillSegs >= 12, "the eleven dense outputs and the absolute gradient");
    auto seg = [&](float* ptr, size_t n) {
        if (ptr && n) {
            fill.ptr[fill.count] = ptr;
            fill.n[fill.count] = n;
            fill.count++;
        }
    };
    if (zmode) {
        seg(dL_dmean2D, 3 * (size_t)P);
        // (the absolute gradient: beside it on the atomic path, whose gauss_bwd writes the touched rows only;
        // on the record path gauss_reduce writes every row and no fill may race it)
        if (atomic) seg(dL_dmean2D_abs, 3 * (size_t)P);
        seg(dL_dconic, 4 * (size_t)P);
        seg(dL_dopacity, (size_t)P);
        seg(dL_dcolor, 3 * (size_t)P);
        seg(dL_dinvdepth, (size_t)P);
        seg(dL_dmean3D, 3 * (size_t)P);
        seg(dL_dcov3D, 6 * (size_t)P);
        if (m_rest > 0) seg(dL_dsh, 3 * (size_t)m_rest * P);
        seg(dc ? dL_ddc : nullptr, 3 * (size_t)P);
        seg(dL_dscale, 3 * (size_t)P);
        seg(dL_drot, 4 * (size_t)P);
    }
    if (!use_list) live = live_count = nullptr;
    if (use_list && R == 0)
        HIP_TRY(hipMemsetAsync(live_count, 0, sizeof(uint32_t) * kLiveShards * kLiveCntStride, stream), "live count");
    SideStream* side = zmode == 1 && !debug && fill.count ? side_stream() : nullptr;
    // Once the fill is queued on the side stream, `stream` must not run ahead of it on ANY return:
    // the caller may free the outputs it writes as soon as this function fails, and the caching
    // allocator would hand their memory to new work on `stream` while the fill still writes it.
    struct SideJoin {
        SideStream* side = nullptr;
        hipStream_t stream = nullptr;
        bool armed = false;
        std::unique_lock<std::mutex> lock;
        void join() {
            if (!armed) return;
            armed = false;
            if (hipStreamWaitEvent(stream, side->join, 0) != hipSuccess) (void)hipStreamSynchronize(side->s);
        }
        ~SideJoin() { join(); }
    } sj;
    if (side) {  // fork: the side stream starts after everything queued so far on `stream`
        sj.lock = std::unique_lock<std::mutex>(side->mu);
        sj.side = side;
        sj.stream = stream;
        HIP_TRY(hipEventRecord(side->fork, stream), "zero fill fork");
        HIP_TRY(hipStreamWaitEvent(side->s, side->fork, 0), "zero fill fork");
        const hipError_t fe = launch_zero_fill(fill, side->s);
        const hipError_t je = hipEventRecord(side->join, side->s);
        if (fe != hipSuccess || je != hipSuccess) {
            (void)hipStreamSynchronize(side->s);  // whatever was queued has finished
            return fail(GSR_ERR_HIP, "zero fill: %s", hipGetErrorString(fe != hipSuccess ? fe : je));
        }
        sj.armed = true;
    }

    // the records' content bytes (zeroed by the forward's K3): render_bwd sets those of the records
    // it writes, gauss_reduce reads them to find the records
    recs.flag = bin.rec_flag;
    // (also with R == 0: gauss_reduce still reads every Gaussian's record start)
    if (!atomic && !mark.recs) {  // a forward that left no record inputs (or a buffer never seen)
        HIP_TRY(launch_rec_prep(P, geom, bin, C, stream), "record prep");
        geom_mark(geom_buffer, mark.zeroed, true, mark.long_lists, mark.half_fwd);
    }
    if (R > 0) {
        StageScope sc(ST_RENDER_BWD, stream);
        RenderBwdArgs ra{};
        ra.W = width; ra.H = height; ra.gx = gx; ra.gy = gy; ra.ranges = img.ranges; ra.gid_sorted = bin.gid_sorted;
        ra.rec = geom.rec;
        ra.bg = background; ra.dL_dpix = dL_dpix; ra.dL_dinvdepth = dL_dinvdepths; ra.img = img; ra.recs = recs;
        ra.dL_dalpha = dL_dalphas;
        ra.absgrad = dL_dmean2D_abs != nullptr;
        ra.ckpt = bin.ckpt; ra.seg_ck = geom.fwd_seg_ck; ra.rec_start = geom.rec_start;
        ra.unit_cnt = geom.unit_cnt; ra.unit_part = geom.unit_part; ra.unit_full = bin.unit_full;
        ra.full_cap = (uint32_t)unit_full_cap(C);
        ra.census = g_census;
        ra.live_count = live_count;  // zeroed by its first workgroup
        if (zmode == 3 && fill.count) {  // the zero fill rides in this launch
            ra.fill = fill;
            ra.fill_blocks = kFusedFillBlocks;
        }
        if (atomic) {
            ra.acc = reinterpret_cast<float*>(geom.acc);
            ra.touched = geom.touched;
        }
        HIP_TRY(launch_render_bwd(ra, max_units, stream, grid_mode), "render_bwd");
    }
    if (int rc = check_debug(debug, stream, "render_bwd")) return rc;
    if (atomic && screen) {  // (stage "gauss_reduce": the step between render_bwd and gauss_bwd / the exchange)
        StageScope sc(ST_GAUSS_REDUCE, stream);
        HIP_TRY(launch_gauss_live_views(P, geom.touched, geom.acc, radii, geom.clamped, sums, flags, stream),
                "gauss_live_views");
    } else if (atomic) {
        // (nothing between render_bwd and gauss_bwd: gauss_bwd lists the touched Gaussians itself)
    } else {
        StageScope sc(ST_GAUSS_REDUCE, stream);
        HIP_TRY(launch_gauss_reduce(P, geom, recs, sums, flags, radii, live, live_count, stream, dL_dmean2D_abs),
                "gauss_reduce");
    }
    if (int rc = check_debug(debug, stream, "gauss_reduce")) return rc;
    if (screen) {
        HIP_TRY(launch_view_header(view_block, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, focal_x, focal_y,
                                   antialiasing, dL_dinvdepths != nullptr, stream),
                "view header");
        return check_debug(debug, stream, "view header");
    }
    {
        StageScope sc(ST_GAUSS_BWD, stream);
        GaussBwdArgs ga{};
        ga.P = P; ga.D = D; ga.M = M; ga.W = width; ga.H = height;
        ga.means3D = means3D; ga.shs = colors_precomp || M <= (dc ? 1 : 0) ? nullptr : shs;
        ga.dc = colors_precomp ? nullptr : dc; ga.opacities = opacities; ga.scales = scales;
        ga.rotations = rotations; ga.cov3D_precomp = cov3D_precomp; ga.scale_modifier = scale_modifier;
        ga.viewmatrix = viewmatrix; ga.projmatrix = projmatrix; ga.campos = campos;
        ga.tan_fovx = tan_fovx; ga.tan_fovy = tan_fovy; ga.focal_x = focal_x; ga.focal_y = focal_y;
        ga.antialiasing = antialiasing; ga.radii = radii; ga.geom = geom; ga.sums = sums;
        ga.have_invdepth = dL_dinvdepths != nullptr;
        ga.dL_dmean2D = dL_dmean2D; ga.dL_dconic = dL_dconic; ga.dL_dopacity = dL_dopacity; ga.dL_dcolor = dL_dcolor;
        ga.dL_dinvdepth = dL_dinvdepth; ga.dL_dmean3D = dL_dmean3D; ga.dL_dcov3D = dL_dcov3D;
        ga.dL_dsh = M > (dc ? 1 : 0) ? dL_dsh : nullptr; ga.dL_ddc = dc ? dL_ddc : nullptr; ga.dL_dscale = dL_dscale; ga.dL_drot = dL_drot;
        if (side) {  // join: gauss_bwd writes over the zeroed outputs
            sj.join();
            sj.lock.unlock();
        } else if (zmode == 1 || zmode == 2 || (zmode == 3 && R == 0)) {  // (3 with R = 0: no render_bwd launch)
            HIP_TRY(launch_zero_fill(fill, stream), "zero fill");
        }
        ga.sparse = zmode ? 1 : 0;
        ga.live = live;
        ga.live_count = live_count;
        ga.live_cap = live_list_cap((uint32_t)P);
        if (atomic) {  // the sums are the accumulator rows of the touched Gaussians (render_bwd ATOMIC)
            ga.touched = geom.touched;
            ga.acc = geom.acc;
            ga.dL_dmean2D_abs = dL_dmean2D_abs;
            // runs of 128 x N touched-bit positions per workgroup (backward.hip gauss_bwd_touched_kernel): N from
            // the option, or by the frame -- 16 where the lists are long (few Gaussians touched: 5M@4K), else 1
            const int opt_run = option(OPT_TOUCHED_RUN);
            const uint32_t run = opt_run > 0 ? (uint32_t)opt_run : mark.long_lists ? 16u : 1u;
            ga.touched_shift = 31u - (uint32_t)__builtin_clz(run);  // (a power of two at most, floor)
        }
        HIP_TRY(launch_gauss_bwd(ga, stream), "gauss_bwd");
    }
    if (int rc = check_debug(debug, stream, "gauss_bwd")) return rc;
    return GSR_OK;
}
}  // namespace

int gsr_rasterize_backward(const gsr_backward_args* args) { return backward_impl(args); }

int gsr_render_alpha(int width, int height, const void* image_buffer, float* out_alpha, void* stream) {
    using namespace gsr;
    clear_error();
    if (width <= 0 || height <= 0)
        return fail(GSR_ERR_ARGUMENT, "render_alpha: invalid sizes W=%d H=%d", width, height);
    if (!image_buffer || !out_alpha) return fail(GSR_ERR_ARGUMENT, "render_alpha: null pointer");
    const uint32_t gx = (width + kTile - 1) / kTile, gy = (height + kTile - 1) / kTile;
    size_t tmp = 0;
    const ImageState img = carve_image((char*)const_cast<void*>(image_buffer), width, height, gx * gy, &tmp);
    HIP_TRY(launch_render_alpha(img.final_T, out_alpha, width, height, (hipStream_t)stream), "render_alpha");
    return GSR_OK;
}

// Every forward path (exact, capacity hint, rebuild after a short hint, redone tiles, the census kernels, any
// fwd_quads / seg_ck / sort_prefix / near_mass / bwd_atomic setting) ends in launch_render_fwd [+ the redo], whose
// waves write the checkpoints, the blend masks, n_contrib and the work list unconditionally: the statistics are
// valid after all of them, and no forward state has to be refused here.
int gsr_contrib_stats(int P, int R, int width, int height, const void* geom_buffer, const void* binning_buffer,
                      const void* image_buffer, int binning_capacity, size_t binning_bytes, const float* pixel_weight,
                      int accumulate, float* stats, void* stream_) {
    using namespace gsr;
    clear_error();
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || R < 0 || width <= 0 || height <= 0)
        return fail(GSR_ERR_ARGUMENT, "contrib_stats: invalid sizes P=%d R=%d W=%d H=%d", P, R, width, height);
    if (P >= kMaxGaussians)
        return fail(GSR_ERR_ARGUMENT, "contrib_stats: P=%d exceeds the tile-list entry limit %d", P, kMaxGaussians - 1);
    if (P == 0) return GSR_OK;
    if (!stats) return fail(GSR_ERR_ARGUMENT, "contrib_stats: null stats");
    if ((reinterpret_cast<uintptr_t>(stats) & 15) != 0)
        return fail(GSR_ERR_ARGUMENT, "contrib_stats: stats must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(pixel_weight) & 3) != 0)
        return fail(GSR_ERR_ARGUMENT, "contrib_stats: pixel_weight must be 4-byte aligned");
    const uint32_t gx = (width + kTile - 1) / kTile, gy = (height + kTile - 1) / kTile;
    const uint32_t tiles = gx * gy;
    size_t C = 0;
    if (R > 0) {
        if (!geom_buffer || !image_buffer || !binning_buffer)
            return fail(GSR_ERR_ARGUMENT, "contrib_stats: missing forward buffers");
        if (!resolve_capacity(R, binning_capacity, binning_bytes, &C))
            return fail(GSR_ERR_ARGUMENT,
                        "contrib_stats: a binning buffer of %zu bytes matches no layout for R=%d (capacity %d)",
                        binning_bytes, R, binning_capacity);
        if (C < (size_t)R) return fail(GSR_ERR_ARGUMENT, "contrib_stats: binning capacity %zu < R=%d", C, R);
    }
    if (!accumulate) HIP_TRY(hipMemsetAsync(stats, 0, 4 * sizeof(float) * (size_t)P, stream), "contrib_stats zero");
    if (R == 0) return GSR_OK;
    size_t tmp = 0;
    const GeomState geom = carve_geom((char*)const_cast<void*>(geom_buffer), P, gx, gy, &tmp);
    const ImageState img = carve_image((char*)const_cast<void*>(image_buffer), width, height, tiles, &tmp);
    const BinningState bin = carve_binning((char*)const_cast<void*>(binning_buffer), C, &tmp);
    ContribArgs ca{};
    ca.W = width; ca.H = height; ca.gx = gx; ca.gy = gy; ca.n_gauss = (uint32_t)P;
    ca.ranges = img.ranges; ca.gid_sorted = bin.gid_sorted; ca.rec = geom.rec; ca.n_contrib = img.n_contrib;
    // the checkpoints only where their T is known to round as the kernel's own (a half-tile forward this library
    // ran into this geometry buffer); after a whole-tile forward, or for buffers it has not seen (copies), each unit
    // re-walks its tile's list for T instead, and weight_max / pixel_count come out the same bits either way
    ca.ckpt = geom_marked(geom_buffer).half_fwd ? bin.ckpt : nullptr; ca.unit_cnt = geom.unit_cnt; ca.unit_part = geom.unit_part; ca.unit_full = bin.unit_full;
    ca.full_cap = (uint32_t)unit_full_cap(C);
    ca.seg_ck = geom.fwd_seg_ck;
    ca.pixel_weight = pixel_weight;
    ca.stats = stats;
    // (sized like the backward's grid: for the shortest segments, whatever the forward used)
    HIP_TRY(launch_contrib_stats(ca, bwd_max_units((size_t)R, tiles, 1), stream, option(OPT_BWD_GRID)), "contrib_stats");
    return GSR_OK;
}

}  // extern "C"

namespace {
// The arguments the two feature calls share, checked, and the walk's view of the three buffers.  Returns GSR_OK with
// *walk false when there is nothing to walk (P == 0 or R == 0).
int features_args(const char* who, int P, int C, int R, int width, int height, const void* geom_buffer,
                  const void* binning_buffer, const void* image_buffer, int binning_capacity, size_t binning_bytes,
                  gsr::FeatureArgs* fa, bool* walk) {
    using namespace gsr;
    *walk = false;
    if (P < 0 || R < 0 || width <= 0 || height <= 0)
        return fail(GSR_ERR_ARGUMENT, "%s: invalid sizes P=%d R=%d W=%d H=%d", who, P, R, width, height);
    if (C <= 0 || (C + kFeatChunk - 1) / kFeatChunk > 65535)
        return fail(GSR_ERR_ARGUMENT, "%s: C=%d channels (1 .. %d)", who, C, 65535 * kFeatChunk);
    if (P >= kMaxGaussians)
        return fail(GSR_ERR_ARGUMENT, "%s: P=%d exceeds the tile-list entry limit %d", who, P, kMaxGaussians - 1);
    const uint32_t gx = (width + kTile - 1) / kTile, gy = (height + kTile - 1) / kTile;
    fa->W = width; fa->H = height; fa->C = C; fa->gx = gx; fa->gy = gy; fa->n_gauss = (uint32_t)P;
    if (P == 0 || R == 0) return GSR_OK;
    if (!geom_buffer || !image_buffer || !binning_buffer)
        return fail(GSR_ERR_ARGUMENT, "%s: missing forward buffers", who);
    size_t cap = 0;
    if (!resolve_capacity(R, binning_capacity, binning_bytes, &cap))
        return fail(GSR_ERR_ARGUMENT, "%s: a binning buffer of %zu bytes matches no layout for R=%d (capacity %d)", who,
                    binning_bytes, R, binning_capacity);
    if (cap < (size_t)R) return fail(GSR_ERR_ARGUMENT, "%s: binning capacity %zu < R=%d", who, cap, R);
    size_t tmp = 0;
    const GeomState geom = carve_geom((char*)const_cast<void*>(geom_buffer), P, gx, gy, &tmp);
    const ImageState img = carve_image((char*)const_cast<void*>(image_buffer), width, height, gx * gy, &tmp);
    const BinningState bin = carve_binning((char*)const_cast<void*>(binning_buffer), cap, &tmp);
    fa->n_entries = (uint32_t)std::min(cap, (size_t)UINT32_MAX);
    fa->ranges = img.ranges; fa->gid_sorted = bin.gid_sorted; fa->rec = geom.rec; fa->n_contrib = img.n_contrib;
    *walk = true;
    return GSR_OK;
}

// The view-block tail the feature and distortion backwards share.  view_block_check: the arguments a view block needs.
int view_block_check(const char* who, const float* view_block, const float* viewmatrix, const float* projmatrix,
                     const float* campos, const int* radii, const void* geom_buffer) {
    using namespace gsr;
    if (!view_block) return GSR_OK;
    if ((reinterpret_cast<uintptr_t>(view_block) & 15) != 0)
        return fail(GSR_ERR_ARGUMENT, "%s: view block must be 16-byte aligned", who);
    if (!viewmatrix || !projmatrix || !campos || !radii || !geom_buffer)
        return fail(GSR_ERR_ARGUMENT, "%s: the view block needs the camera, radii and the geometry buffer", who);
    return GSR_OK;
}

// Scratch accumulator rows and touched bits, zeroed (gauss_live_views leaves them zero again).
int view_scratch(const char* who, int P, gsr_alloc_fn scratch_alloc, void* scratch_ctx, hipStream_t stream,
                 float4** acc, uint32_t** touched) {
    using namespace gsr;
    Carver c{nullptr, 0};
    c.take<float4>((size_t)kAccRow4 * P);
    c.take<uint32_t>(touched_words((size_t)P));
    const size_t bytes = align_up(c.off);
    char* base = (char*)call_alloc(scratch_alloc, scratch_ctx, bytes);
    if (!base) return fail(GSR_ERR_ALLOC, "%s: scratch allocation failed", who);
    Carver d{base, 0};
    *acc = d.take<float4>((size_t)kAccRow4 * P);
    *touched = d.take<uint32_t>(touched_words((size_t)P));
    HIP_TRY(hipMemsetAsync(base, 0, bytes, stream), who);
    return GSR_OK;
}

// The view block of one such loss alone, from the accumulator rows its kernel added into: colour and inverse-depth
// sums zero, the flags from radii and the forward's SH clamp bits, the camera header (no inverse-depth term).
int view_block_finish(const char* who, int P, int width, int height, float* view_block, uint32_t* touched, float4* acc,
                      const int* radii, const void* geom_buffer, const float* viewmatrix, const float* projmatrix,
                      const float* campos, float tan_fovx, float tan_fovy, int antialiasing, hipStream_t stream) {
    using namespace gsr;
    float* body = view_block + kViewBlockHeader;
    GradRecs sums{};
    sums.a = reinterpret_cast<float4*>(body);
    sums.b = reinterpret_cast<float4*>(body + 4 * (size_t)P);
    sums.c = reinterpret_cast<float2*>(body + 8 * (size_t)P);
    uint32_t* flags = reinterpret_cast<uint32_t*>(body + 10 * (size_t)P);
    HIP_TRY(launch_gauss_live_views(P, touched, acc, radii, geom_clamped(geom_buffer, P, width, height), sums, flags,
                                    stream),
            who);
    const float focal_y = height / (2.0f * tan_fovy), focal_x = width / (2.0f * tan_fovx);
    HIP_TRY(launch_view_header(view_block, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, focal_x, focal_y,
                               antialiasing, 0, stream),
            who);
    return GSR_OK;
}
}  // namespace

extern "C" {

// Like gsr_contrib_stats the two feature calls need only what every forward path leaves behind (the sorted lists
// with the blend masks, the records, n_contrib), and they walk whole lists from the head: no checkpoint, no work
// list, no forward state is consulted, so no forward has to be refused.
int gsr_render_features(int P, int C, int R, int width, int height, const void* geom_buffer,
                        const void* binning_buffer, const void* image_buffer, int binning_capacity,
                        size_t binning_bytes, const float* features, float* out_features, void* stream_) {
    using namespace gsr;
    clear_error();
    hipStream_t stream = (hipStream_t)stream_;
    FeatureArgs fa{};
    bool walk = false;
    if (int rc = features_args("render_features", P, C, R, width, height, geom_buffer, binning_buffer, image_buffer,
                               binning_capacity, binning_bytes, &fa, &walk))
        return rc;
    if (!out_features || (P > 0 && !features)) return fail(GSR_ERR_ARGUMENT, "render_features: null pointer");
    if (!walk) {
        HIP_TRY(hipMemsetAsync(out_features, 0, sizeof(float) * (size_t)C * width * height, stream),
                "render_features zero");
        return GSR_OK;
    }
    fa.features = features;
    fa.out = out_features;
    HIP_TRY(launch_features_fwd(fa, stream), "render_features");
    return GSR_OK;
}

int gsr_render_features_backward(int P, int C, int R, int width, int height, const void* geom_buffer,
                                 const void* binning_buffer, const void* image_buffer, int binning_capacity,
                                 size_t binning_bytes, const float* features, const float* out_features,
                                 const float* dL_dout_features, float* dL_dfeatures, float* view_block,
                                 const float* viewmatrix, const float* projmatrix, const float* campos,
                                 float tan_fovx, float tan_fovy, int antialiasing, const int* radii,
                                 gsr_alloc_fn scratch_alloc, void* scratch_ctx, void* stream_) {
    using namespace gsr;
    clear_error();
    hipStream_t stream = (hipStream_t)stream_;
    FeatureArgs fa{};
    bool walk = false;
    if (int rc = features_args("render_features_backward", P, C, R, width, height, geom_buffer, binning_buffer,
                               image_buffer, binning_capacity, binning_bytes, &fa, &walk))
        return rc;
    if (P == 0) return GSR_OK;
    if (!features || !dL_dout_features || !dL_dfeatures || (view_block && !out_features))
        return fail(GSR_ERR_ARGUMENT, "render_features_backward: null pointer");
    if (int rc = view_block_check("render_features_backward", view_block, viewmatrix, projmatrix, campos, radii,
                                  geom_buffer))
        return rc;
    HIP_TRY(hipMemsetAsync(dL_dfeatures, 0, sizeof(float) * (size_t)P * C, stream), "render_features_backward zero");
    float4* acc = nullptr;
    uint32_t* touched = nullptr;
    if (view_block)
        if (int rc = view_scratch("render_features_backward", P, scratch_alloc, scratch_ctx, stream, &acc, &touched))
            return rc;
    if (walk) {
        fa.features = features;
        fa.fmap = out_features;
        fa.dL_dfmap = dL_dout_features;
        fa.dL_dfeatures = dL_dfeatures;
        fa.acc = reinterpret_cast<float*>(acc);
        fa.touched = touched;
        HIP_TRY(launch_features_bwd(fa, stream), "render_features_backward");
    }
    if (view_block)
        return view_block_finish("render_features_backward", P, width, height, view_block, touched, acc, radii,
                                 geom_buffer, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, antialiasing, stream);
    return GSR_OK;
}

int gsr_render_features_chunk(void) { return gsr::kFeatChunk; }

// The distortion pair is the feature pair over one scalar per Gaussian: the same argument rules (features_args with
// C = 1), the same walk, the same view-block tail.
int gsr_render_distortion(int P, int R, int width, int height, const void* geom_buffer, const void* binning_buffer,
                          const void* image_buffer, int binning_capacity, size_t binning_bytes, const float* t,
                          float* out_distortion, float* out_moments, void* stream_) {
    using namespace gsr;
    clear_error();
    hipStream_t stream = (hipStream_t)stream_;
    DistortionArgs da{};
    bool walk = false;
    if (int rc = features_args("render_distortion", P, 1, R, width, height, geom_buffer, binning_buffer, image_buffer,
                               binning_capacity, binning_bytes, &da.walk, &walk))
        return rc;
    if (!out_distortion || !out_moments || (P > 0 && !t))
        return fail(GSR_ERR_ARGUMENT, "render_distortion: null pointer");
    if (!walk) {
        const size_t N = (size_t)width * height;
        HIP_TRY(hipMemsetAsync(out_distortion, 0, sizeof(float) * N, stream), "render_distortion zero");
        HIP_TRY(hipMemsetAsync(out_moments, 0, sizeof(float) * 2 * N, stream), "render_distortion zero");
        return GSR_OK;
    }
    da.walk.features = t;
    da.walk.out = out_distortion;
    da.moments = out_moments;
    HIP_TRY(launch_distortion_fwd(da, stream), "render_distortion");
    return GSR_OK;
}

int gsr_render_distortion_backward(int P, int R, int width, int height, const void* geom_buffer,
                                   const void* binning_buffer, const void* image_buffer, int binning_capacity,
                                   size_t binning_bytes, const float* t, const float* out_distortion,
                                   const float* out_moments, const float* dL_dout_distortion, float* dL_dt,
                                   float* view_block, const float* viewmatrix, const float* projmatrix,
                                   const float* campos, float tan_fovx, float tan_fovy, int antialiasing,
                                   const int* radii, gsr_alloc_fn scratch_alloc, void* scratch_ctx, void* stream_) {
    using namespace gsr;
    clear_error();
    hipStream_t stream = (hipStream_t)stream_;
    DistortionArgs da{};
    bool walk = false;
    if (int rc = features_args("render_distortion_backward", P, 1, R, width, height, geom_buffer, binning_buffer,
                               image_buffer, binning_capacity, binning_bytes, &da.walk, &walk))
        return rc;
    if (P == 0) return GSR_OK;
    if (!t || !out_moments || !dL_dout_distortion || !dL_dt || (view_block && !out_distortion))
        return fail(GSR_ERR_ARGUMENT, "render_distortion_backward: null pointer");
    if (int rc = view_block_check("render_distortion_backward", view_block, viewmatrix, projmatrix, campos, radii,
                                  geom_buffer))
        return rc;
    HIP_TRY(hipMemsetAsync(dL_dt, 0, sizeof(float) * (size_t)P, stream), "render_distortion_backward zero");
    float4* acc = nullptr;
    uint32_t* touched = nullptr;
    if (view_block)
        if (int rc = view_scratch("render_distortion_backward", P, scratch_alloc, scratch_ctx, stream, &acc, &touched))
            return rc;
    if (walk) {
        da.walk.features = t;
        da.walk.fmap = out_distortion;
        da.walk.dL_dfmap = dL_dout_distortion;
        da.walk.dL_dfeatures = dL_dt;
        da.walk.acc = reinterpret_cast<float*>(acc);
        da.walk.touched = touched;
        da.moments = const_cast<float*>(out_moments);  // (read only)
        HIP_TRY(launch_distortion_bwd(da, stream), "render_distortion_backward");
    }
    if (view_block)
        return view_block_finish("render_distortion_backward", P, width, height, view_block, touched, acc, radii,
                                 geom_buffer, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, antialiasing, stream);
    return GSR_OK;
}

// The selections ride the same walk and the same argument rules (features_args with C = 1); their outputs come in
// two groups, each whole or absent.
int gsr_render_select(int P, int R, int width, int height, const void* geom_buffer, const void* binning_buffer,
                      const void* image_buffer, int binning_capacity, size_t binning_bytes, const float* t, int K,
                      float* out_median, int* out_median_ids, int* out_topk_ids, float* out_topk_weights,
                      void* stream_) {
    using namespace gsr;
    clear_error();
    hipStream_t stream = (hipStream_t)stream_;
    SelectArgs sa{};
    bool walk = false;
    if (int rc = features_args("render_select", P, 1, R, width, height, geom_buffer, binning_buffer, image_buffer,
                               binning_capacity, binning_bytes, &sa.walk, &walk))
        return rc;
    if (K < 0 || K > kSelectMaxK) return fail(GSR_ERR_ARGUMENT, "render_select: K=%d (0 .. %d)", K, kSelectMaxK);
    const bool median = out_median != nullptr;
    if ((out_median_ids != nullptr) != median || (P > 0 && (t != nullptr) != median) || (P == 0 && t && !median))
        return fail(GSR_ERR_ARGUMENT, "render_select: t, out_median and out_median_ids go together (all or none)");
    if ((out_topk_ids != nullptr) != (K > 0) || (out_topk_weights != nullptr) != (K > 0))
        return fail(GSR_ERR_ARGUMENT, "render_select: the top-K outputs are set exactly when K > 0 (K=%d)", K);
    if (K == 0 && !median) return fail(GSR_ERR_ARGUMENT, "render_select: nothing to select (K = 0 and no median)");
    if (!walk) {  // ids -1, floats 0
        const size_t N = (size_t)width * height;
        if (median) {
            HIP_TRY(hipMemsetAsync(out_median, 0, sizeof(float) * N, stream), "render_select fill");
            HIP_TRY(hipMemsetAsync(out_median_ids, 0xff, sizeof(int) * N, stream), "render_select fill");
        }
        if (K > 0) {
            HIP_TRY(hipMemsetAsync(out_topk_ids, 0xff, sizeof(int) * N * K, stream), "render_select fill");
            HIP_TRY(hipMemsetAsync(out_topk_weights, 0, sizeof(float) * N * K, stream), "render_select fill");
        }
        return GSR_OK;
    }
    sa.walk.features = t;
    sa.K = K;
    sa.out_median = out_median;
    sa.out_median_ids = out_median_ids;
    sa.out_topk_ids = out_topk_ids;
    sa.out_topk_weights = out_topk_weights;
    HIP_TRY(launch_select_fwd(sa, stream), "render_select");
    return GSR_OK;
}

int gsr_render_select_max_k(void) { return gsr::kSelectMaxK; }

int gsr_render_median_backward(int P, int width, int height, const int* median_ids, const float* dL_dout_median,
                               float* dL_dt, void* stream_) {
    using namespace gsr;
    clear_error();
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || width <= 0 || height <= 0)
        return fail(GSR_ERR_ARGUMENT, "render_median_backward: invalid sizes P=%d W=%d H=%d", P, width, height);
    if (P == 0) return GSR_OK;
    if (!median_ids || !dL_dout_median || !dL_dt)
        return fail(GSR_ERR_ARGUMENT, "render_median_backward: null pointer");
    HIP_TRY(launch_median_bwd(P, width, height, median_ids, dL_dout_median, dL_dt, stream), "render_median_backward");
    return GSR_OK;
}

int gsr_debug_forward_state(int P, int width, int height, int R, int binning_capacity, size_t binning_bytes,
                            const void* geom_buffer, const void* binning_buffer, const void* image_buffer,
                            unsigned int* ranges, unsigned int* point_list, unsigned int* n_contrib, float* final_T,
                            void* stream_) {
    using namespace gsr;
    clear_error();
    hipStream_t stream = (hipStream_t)stream_;
    if (P <= 0 || R < 0 || width <= 0 || height <= 0)
        return fail(GSR_ERR_ARGUMENT, "debug_forward_state: invalid sizes P=%d R=%d W=%d H=%d", P, R, width, height);
    if (!image_buffer || (R > 0 && !binning_buffer))
        return fail(GSR_ERR_ARGUMENT, "debug_forward_state: missing forward buffers");
    size_t C = 0, tmp = 0;
    if (!resolve_capacity(R, binning_capacity, binning_bytes, &C) || C < (size_t)R)
        return fail(GSR_ERR_ARGUMENT, "debug_forward_state: binning buffer of %zu bytes matches no layout for R=%d",
                    binning_bytes, R);
    const uint32_t gx = (width + kTile - 1) / kTile, gy = (height + kTile - 1) / kTile;
    ImageState img = carve_image((char*)image_buffer, width, height, gx * gy, &tmp);
    const size_t N = (size_t)width * height;
    if (ranges) HIP_TRY(hipMemcpyAsync(ranges, img.ranges, sizeof(uint2) * gx * gy, hipMemcpyDeviceToDevice, stream),
                        "debug_forward_state ranges");
    (void)N;
    if (n_contrib)
        HIP_TRY(launch_untile(img.n_contrib, n_contrib, width, height, gx, stream), "debug_forward_state n_contrib");
    if (final_T)
        HIP_TRY(launch_untile(reinterpret_cast<const uint32_t*>(img.final_T), reinterpret_cast<uint32_t*>(final_T),
                              width, height, gx, stream),
                "debug_forward_state final_T");
    if (point_list && R > 0) {
        // the forward's sorted entries (masks included) and, where K4 sorted only a list's reachable
        // prefix, the rest of the list sorted here into the copy
        if (!geom_buffer) return fail(GSR_ERR_ARGUMENT, "debug_forward_state: point_list needs the geometry buffer");
        BinningState bin = carve_binning((char*)binning_buffer, C, &tmp);
        GeomState geom = carve_geom((char*)const_cast<void*>(geom_buffer), P, gx, gy, &tmp);
        HIP_TRY(launch_sorted_lists_copy(gx * gy, img.ranges, geom, bin, C, point_list, stream, P, gx, true),
                "debug_forward_state point_list");
    }
    return GSR_OK;
}

int gsr_debug_sort_state(int P, int width, int height, const void* geom_buffer, unsigned int* sorted_len,
                         unsigned int* redo_count, void* stream_) {
    using namespace gsr;
    clear_error();
    hipStream_t stream = (hipStream_t)stream_;
    if (P <= 0 || width <= 0 || height <= 0 || !geom_buffer)
        return fail(GSR_ERR_ARGUMENT, "debug_sort_state: invalid sizes or no geometry buffer");
    const uint32_t gx = (width + kTile - 1) / kTile, gy = (height + kTile - 1) / kTile;
    size_t tmp = 0;
    GeomState geom = carve_geom((char*)const_cast<void*>(geom_buffer), P, gx, gy, &tmp);
    if (sorted_len)
        HIP_TRY(hipMemcpyAsync(sorted_len, geom.sorted_len, sizeof(uint32_t) * gx * gy, hipMemcpyDeviceToDevice, stream),
                "debug_sort_state sorted_len");
    if (redo_count)
        HIP_TRY(hipMemcpyAsync(redo_count, geom.redo_cnt, sizeof(uint32_t), hipMemcpyDeviceToDevice, stream),
                "debug_sort_state redo_count");
    return GSR_OK;
}

int gsr_debug_near_state(int P, int width, int height, const void* geom_buffer, unsigned int* zcut,
                         unsigned int* near_ranges, void* stream_) {
    using namespace gsr;
    clear_error();
    hipStream_t stream = (hipStream_t)stream_;
    if (P <= 0 || width <= 0 || height <= 0 || !geom_buffer)
        return fail(GSR_ERR_ARGUMENT, "debug_near_state: invalid sizes or no geometry buffer");
    const uint32_t gx = (width + kTile - 1) / kTile, gy = (height + kTile - 1) / kTile;
    size_t tmp = 0;
    GeomState geom = carve_geom((char*)const_cast<void*>(geom_buffer), P, gx, gy, &tmp);
    if (zcut)
        HIP_TRY(hipMemcpyAsync(zcut, geom.zcut, sizeof(uint32_t), hipMemcpyDeviceToDevice, stream), "debug_near_state zcut");
    if (near_ranges)
        HIP_TRY(hipMemcpyAsync(near_ranges, geom.sranges, sizeof(uint2) * gx * gy, hipMemcpyDeviceToDevice, stream),
                "debug_near_state sranges");
    return GSR_OK;
}

}  // extern "C"
