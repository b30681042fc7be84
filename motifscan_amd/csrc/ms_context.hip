// ms_context.hip -- what belongs to no handle: the per-thread error string, the per-device contexts (streams, events, scan scratch), the
// device block pool and the pinned host pool, and the device / NUMA / host-memory entry points of include/motifscan_amd.h.  One HIP
// stream per device owned by the library; no file-scope scan state (contrast cscore.c:26-34), so handles can be used from several
// threads / devices.
#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>

#include "ms_handles.h"

namespace ms {

static thread_local std::string g_err;
static thread_local int g_device = 0;

int current_device() { return g_device; }
void set_current_device(int device) { g_device = device; }

void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

// ------------------------------------------------------------ ms_debug_alloc_fill --

std::atomic<int> g_alloc_fill{-1};

int alloc_fill_device(void *p, size_t bytes, int byte, int device) {
    int here = -1;
    hipError_t e = hipGetDevice(&here);
    const bool move = e == hipSuccess && device >= 0 && device != here;
    if (e == hipSuccess && move) e = hipSetDevice(device);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemset(p, byte, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (move) (void) hipSetDevice(here);
    if (e != hipSuccess) { set_error("ms_debug_alloc_fill: filling %zu bytes failed: %s", bytes, hipGetErrorString(e)); return MS_ERR_RUNTIME; }
    return MS_OK;
}

// ----------------------------------------------------------------- per-device state --

static std::mutex g_ctx_mu;
static std::map<int, std::unique_ptr<DeviceCtx>> g_ctx;

int get_ctx(int device, DeviceCtx **out) {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    auto it = g_ctx.find(device);
    if (it != g_ctx.end()) { *out = it->second.get(); MS_HIP(hipSetDevice(device)); return MS_OK; }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error("no usable HIP device (%s); libmotifscan_amd has no CPU fallback", hipGetErrorString(e));
        return MS_ERR_RUNTIME;
    }
    if (device < 0 || device >= n) { set_error("device %d out of range (%d devices)", device, n); return MS_ERR_INVALID; }
    MS_HIP(hipSetDevice(device));
    std::unique_ptr<DeviceCtx> c(new DeviceCtx());
    c->device = device;
    hipDeviceProp_t prop;
    MS_HIP(hipGetDeviceProperties(&prop, device));
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    int lds_attr = 0;
    if (hipDeviceGetAttribute(&lds_attr, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) lds_attr = 0;
    c->lds_max = std::max<size_t>((size_t) lds_attr, prop.sharedMemPerBlock);
    if (c->lds_max < 65536) c->lds_max = 65536;
    if (c->lds_max > 163840) c->lds_max = 163840;
    MS_HIP(hipStreamCreateWithFlags(&c->stream.whole, hipStreamNonBlocking));
    MS_HIP(hipStreamCreateWithFlags(&c->stream_up.whole, hipStreamNonBlocking));
    MS_HIP(hipStreamCreateWithFlags(&c->stream_down.whole, hipStreamNonBlocking));
    for (StreamSel *s : {&c->stream, &c->stream_up, &c->stream_down}) s->n_streams = &c->n_streams;
    if (measure_env("MS_CU_PARTITION")) {
        // A/B switch (MS_MEASURE=1 MS_CU_PARTITION=1); off by default, see StreamSel.
        // CU mask bit i = CU (i / n_xcc) of XCC (i % n_xcc) (measured, tools/ubench/cumask_probe.hip: the first 8 bits select one
        // CU on each of the 8 XCCs; an XCC without a bit is left unmasked, so the copy share must cover every XCC): the first
        // n_cu / 32 bits go to the copy streams, the rest to the scan.
        const int k = std::max(1, c->n_cu / 32);
        std::vector<uint32_t> m_copy((size_t) (c->n_cu + 31) / 32, 0u), m_scan((size_t) (c->n_cu + 31) / 32, 0u);
        for (int i = 0; i < c->n_cu; i++) (i < k ? m_copy : m_scan)[(size_t) i / 32] |= 1u << (i % 32);
        bool ok = c->n_cu >= 64;
        ok = ok && hipExtStreamCreateWithCUMask(&c->stream.part, (uint32_t) m_scan.size(), m_scan.data()) == hipSuccess;
        ok = ok && hipExtStreamCreateWithCUMask(&c->stream_up.part, (uint32_t) m_copy.size(), m_copy.data()) == hipSuccess;
        ok = ok && hipExtStreamCreateWithCUMask(&c->stream_down.part, (uint32_t) m_copy.size(), m_copy.data()) == hipSuccess;
        if (ok) {
            c->n_cu_copy = k;
        } else {                                   // no masks on this device / runtime: everything stays on the whole-device streams
            (void) hipGetLastError();
            for (StreamSel *s : {&c->stream, &c->stream_up, &c->stream_down}) {
                if (s->part) (void) hipStreamDestroy(s->part);
                s->part = nullptr;
            }
        }
    }
    MS_HIP(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    MS_HIP(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    for (auto &ev : c->ev) MS_HIP(hipEventCreate(&ev));
    MS_HIP(hipMalloc(&c->sc.counters, 8 * sizeof(unsigned long long)));
    MS_HIP(hipMalloc(&c->sc.bucket_tab, kBucketTabWords * sizeof(unsigned long long)));
    MS_HIP(hipHostMalloc(&c->sc.h_counters, 8 * sizeof(unsigned long long)));
    if (const int fill = alloc_fill_setting(); fill >= 0) {      // (not dev_alloc: its out-of-memory path takes g_ctx_mu, held here)
        // (a fill that fails here is let go: the context stays whole, and the first allocation through dev_alloc reports the device's state)
        (void) alloc_fill_device(c->sc.counters, 8 * sizeof(unsigned long long), fill, -1);
        (void) alloc_fill_device(c->sc.bucket_tab, kBucketTabWords * sizeof(unsigned long long), fill, -1);
        memset(c->sc.h_counters, fill, 8 * sizeof(unsigned long long));
    }
    {
        size_t mem_free = 0, mem_total = 0;
        if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess && mem_total > 0) c->pool.max_bytes = mem_total / 3;
        else (void) hipGetLastError();
    }
    *out = c.get();
    g_ctx[device] = std::move(c);
    return MS_OK;
}

// Size class of a request: the next of {8..15} x 2^k at or above it (at most 12.5 % over), 64 KB at least.
static size_t pool_class(size_t bytes) {
    size_t b = std::max<size_t>(bytes, 1u << 16);
    int k = 63 - __builtin_clzll((unsigned long long) b);          // 2^k <= b
    const size_t step = (size_t) 1 << (k - 3);
    return (b + step - 1) & ~(step - 1);
}

static uint64_t now_ns() {
    return (uint64_t) std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int pool_alloc(DeviceCtx *c, size_t bytes, void **out, size_t *got) {
    const size_t want = pool_class(bytes);
    bool hit = false;
    {
        std::lock_guard<std::mutex> lk(c->pool.mu);
        size_t best = (size_t) -1;
        for (size_t i = 0; i < c->pool.free_.size(); i++) {
            const size_t sz = c->pool.free_[i].second;
            if (sz >= want && sz <= want + want / 2 && (best == (size_t) -1 || sz < c->pool.free_[best].second)) best = i;
        }
        if (best != (size_t) -1) {
            *out = c->pool.free_[best].first;
            *got = c->pool.free_[best].second;
            c->pool.bytes -= *got;
            c->pool.free_.erase(c->pool.free_.begin() + (long) best);
            c->pool.n_hit++;
            hit = true;
        }
    }
    if (hit) {
        const int fill = alloc_fill_setting();
        if (fill < 0) return MS_OK;
        const int rc = alloc_fill_device(*out, *got, fill, c->device);
        if (rc) { pool_free(c, *out, *got); *out = nullptr; *got = 0; }      // a failed call hands nothing out
        return rc;
    }
    const uint64_t t0 = now_ns();
    char *p = nullptr;
    int rc = dev_alloc(&p, want);               // (dev_alloc itself drops the cache and retries once when the device is full)
    if (rc) return rc;
    {
        std::lock_guard<std::mutex> lk(c->pool.mu);
        c->pool.n_miss++;
        c->pool.ns_driver += now_ns() - t0;
    }
    *out = p;
    *got = want;
    return MS_OK;
}

// Pinned host blocks are even dearer to create than device blocks (page-locking ~0.25 ms per MB, and hipHostFree waits for the whole device):
// kept for reuse in the device pool's SIZE CLASSES (round 6).  Rounds 2-5 matched a request to any free block of 1 ... 2 x its size, at most 16
// blocks: the 14 batches of a configs[3] pass ask for 14 different sizes, a small request took the block a larger one needed, the largest
// went to the driver, the list ran over and a block went back to the driver -- episodes of 80-ms passes among 48-ms ones
// (profiles/r06f_e2e_cli_probe.log).  With classes a pass's blocks come back to exactly the requests that made them.
static std::mutex g_pin_mu;
static std::vector<std::pair<void *, size_t>> g_pin_free;
static uint64_t g_pin_stats[4] = {0, 0, 0, 0};            // served from the list, went to hipHostMalloc, returned to the driver, ns inside the driver

void *pinned_alloc(size_t bytes, size_t *got) {
    const size_t want = pool_class(bytes);
    void *hit = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        for (size_t i = g_pin_free.size(); i-- > 0;)
            if (g_pin_free[i].second == want) {
                void *p = g_pin_free[i].first;
                *got = want;
                g_pin_free.erase(g_pin_free.begin() + (long) i);
                g_pin_stats[0]++;
                hit = p;
                break;
            }
    }
    if (hit) {
        if (const int fill = alloc_fill_setting(); fill >= 0) memset(hit, fill, want);
        return hit;
    }
    void *p = nullptr;
    const uint64_t t0 = now_ns();
    const bool ok = hipHostMalloc(&p, want) == hipSuccess;
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        g_pin_stats[1]++;
        g_pin_stats[3] += now_ns() - t0;
    }
    if (!ok) { (void) hipGetLastError(); return nullptr; }
    if (const int fill = alloc_fill_setting(); fill >= 0) memset(p, fill, want);
    *got = want;
    return p;
}

void pinned_free(void *p, size_t bytes) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        size_t total = bytes;
        for (auto &b : g_pin_free) total += b.second;
        if (g_pin_free.size() < 96 && total <= (24ull << 30)) { g_pin_free.emplace_back(p, bytes); return; }
    }
    const uint64_t t0 = now_ns();
    (void) hipHostFree(p);
    std::lock_guard<std::mutex> lk(g_pin_mu);
    g_pin_stats[2]++;
    g_pin_stats[3] += now_ns() - t0;
}

void pinned_pool_stats(uint64_t out[4]) {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (int i = 0; i < 4; i++) out[i] = g_pin_stats[i];
}

size_t pool_trim_current_device() {
    DeviceCtx *c = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_ctx_mu);
        auto it = g_ctx.find(g_device);
        if (it == g_ctx.end()) return 0;
        c = it->second.get();
    }
    std::vector<std::pair<void *, size_t>> victims;
    {
        std::lock_guard<std::mutex> lk(c->pool.mu);
        victims.swap(c->pool.free_);
        c->pool.bytes = 0;
        c->pool.n_driver_free += victims.size();
    }
    size_t freed = 0;
    for (auto &b : victims) { (void) hipFree(b.first); freed += b.second; }
    return freed;
}

void pool_free(DeviceCtx *c, void *p, size_t bytes) {
    if (!p) return;
    std::unique_lock<std::mutex> lk(c->pool.mu);
    if (c->pool.bytes + bytes <= c->pool.max_bytes && c->pool.free_.size() < BlockPool::kMaxBlocks) {
        c->pool.free_.emplace_back(p, bytes);
        c->pool.bytes += bytes;
        return;
    }
    // full.  By BYTES (the cache holds a third of the device): give the driver the SMALLEST cached block that is smaller than this one, or
    // this one -- the large blocks are the dear ones to make again (~100 ms per GB-sized hipMalloc), and a sweep that cycles through more
    // result blocks than fit keeps missing the cheap ones, not the dear ones (an LRU rule, tried in round 5, cost the 3 Gbp sweep with all
    // sites copied out 300 ms of driver time per pass: profiles/r05_bench_c5_3000mbp.json against r04e_).  By COUNT (kMaxBlocks, 512 since
    // round 5: 64 large blocks of a sweep once filled the list and every block of a later stream of small batches went back to the driver
    // and came from hipMalloc again, forever): the stalest block leaves -- the list is in order of return, its front is the stalest.
    std::vector<void *> victims;
    void *keep = p;
    if (c->pool.free_.size() >= BlockPool::kMaxBlocks) {
        victims.push_back(c->pool.free_.front().first);
        c->pool.bytes -= c->pool.free_.front().second;
        c->pool.free_.erase(c->pool.free_.begin());
    }
    if (c->pool.bytes + bytes > c->pool.max_bytes) {
        size_t small = (size_t) -1;
        for (size_t i = 0; i < c->pool.free_.size(); i++)
            if (c->pool.free_[i].second < bytes && (small == (size_t) -1 || c->pool.free_[i].second < c->pool.free_[small].second)) small = i;
        if (small != (size_t) -1 && c->pool.bytes - c->pool.free_[small].second + bytes <= c->pool.max_bytes) {
            victims.push_back(c->pool.free_[small].first);
            c->pool.bytes -= c->pool.free_[small].second;
            c->pool.free_.erase(c->pool.free_.begin() + (long) small);
        } else {
            victims.push_back(p);
            keep = nullptr;
        }
    }
    if (keep) {
        c->pool.free_.emplace_back(keep, bytes);
        c->pool.bytes += bytes;
    }
    c->pool.n_driver_free += victims.size();
    lk.unlock();
    const uint64_t t0 = now_ns();
    for (void *v : victims) (void) hipFree(v);
    lk.lock();
    c->pool.ns_driver += now_ns() - t0;
}

// MS_NUMA_BIND policy (ms_numa.cpp) for the calling thread and `device`; the node is looked up once per device
int numa_bind_for_device(int device, bool force) {
    static std::mutex mu;
    static std::map<int, int> node_of;                      // device -> node (-1 unknown)
    static int policy = -2;                                 // -2 unread, 0 never, 1 always, 2 auto
    static int n_nodes = 0, n_gpus = 0;
    int node = -1;
    {
        std::lock_guard<std::mutex> lk(mu);
        if (policy == -2) {
            const char *e = getenv("MS_NUMA_BIND");
            policy = !e ? 2 : (e[0] == '0' ? 0 : 1);
            n_nodes = numa_node_count("");
            if (hipGetDeviceCount(&n_gpus) != hipSuccess) { n_gpus = 0; (void) hipGetLastError(); }
        }
        if (!force && (policy == 0 || (policy == 2 && !(n_nodes > 1 && n_gpus > 1)))) return -1;
        auto it = node_of.find(device);
        if (it == node_of.end()) {
            char bdf[64] = {0};
            int nd = -1;
            if (hipDeviceGetPCIBusId(bdf, (int) sizeof(bdf), device) == hipSuccess) nd = numa_node_of_bdf(bdf, "");
            else (void) hipGetLastError();
            it = node_of.emplace(device, nd).first;
        }
        node = it->second;
    }
    if (node < 0) return -1;
    return numa_bind_calling_thread(node) > 0 ? node : -1;
}

}  // namespace ms

using namespace ms;

extern "C" {

const char *ms_last_error(void) { return g_err.c_str(); }

int ms_version(void) { return 100; }

int ms_device_count(int *count) {
    if (!count) { set_error("count is NULL"); return MS_ERR_INVALID; }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; set_error("hipGetDeviceCount: %s", hipGetErrorString(e)); return MS_ERR_RUNTIME; }
    *count = n;
    return MS_OK;
}

int ms_set_device(int device) {
    DeviceCtx *c;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    g_device = device;
    return MS_OK;
}

// Bind the CALLING thread to the CPUs of the NUMA node the calling thread's device hangs off (memory it allocates afterwards -- pinned
// buffers included -- is placed there by first touch).  force = 0: only where the policy says so (MS_NUMA_BIND; default: multi-GPU nodes
// with more than one NUMA node); force != 0: always.  *node = the node bound to, -1 if nothing was done (no NUMA information, policy off).
int ms_numa_bind_thread(int force, int *node) {
    DeviceCtx *c;
    int rc = get_ctx(g_device, &c);
    if (rc) return rc;
    const int nd = numa_bind_for_device(c->device, force != 0);
    if (node) *node = nd;
    return MS_OK;
}

int ms_device_name(char *buf, int buflen) {
    if (!buf || buflen <= 0) { set_error("bad buffer"); return MS_ERR_INVALID; }
    DeviceCtx *c;
    int rc = get_ctx(g_device, &c);
    if (rc) return rc;
    hipDeviceProp_t prop;
    MS_HIP(hipGetDeviceProperties(&prop, g_device));
    snprintf(buf, (size_t) buflen, "%s (%s, %d CUs, %zu B LDS/block)", prop.name, prop.gcnArchName, c->n_cu, c->lds_max);
    return MS_OK;
}

int ms_debug_numa_probe(const char *root, const char *bdf, int32_t *node, int32_t *n_cpus, int32_t *n_nodes) {
    if (!root || !bdf) { set_error("NULL argument"); return MS_ERR_INVALID; }
    const int nd = numa_node_of_bdf(bdf, root);
    cpu_set_t set;
    if (node) *node = nd;
    if (n_cpus) *n_cpus = numa_cpus_of_node(nd, root, &set);
    if (n_nodes) *n_nodes = numa_node_count(root);
    return MS_OK;
}

int ms_device_pool_stats(uint64_t out[6]) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    DeviceCtx *c;
    int rc = get_ctx(g_device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->pool.mu);
    out[0] = c->pool.n_hit; out[1] = c->pool.n_miss; out[2] = c->pool.n_driver_free; out[3] = c->pool.ns_driver;
    out[4] = c->pool.bytes; out[5] = c->pool.free_.size();
    return MS_OK;
}

// the pinned-block cache (process-wide): out[0] requests served from the cache, out[1] requests that went to hipHostMalloc, out[2] blocks returned
// to the driver, out[3] nanoseconds inside the driver for [1] and [2].  Steady-state batches should show no [1] / [2].
int ms_host_pool_stats(uint64_t out[4]) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    pinned_pool_stats(out);
    return MS_OK;
}

int ms_host_alloc(size_t bytes, void **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    DeviceCtx *c;
    int rc = get_ctx(g_device, &c);                       // pinned memory needs a live HIP runtime: fails loudly without a device
    if (rc) return rc;
    void *p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1);
    if (e != hipSuccess) { set_error("hipHostMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e)); return MS_ERR_NOMEM; }
    *out = p;
    return MS_OK;
}

void ms_host_free(void *p) { if (p) (void) hipHostFree(p); }

int ms_debug_alloc_fill(int32_t byte, int32_t *previous) {
    if (byte < -1 || byte > 255) { set_error("byte must be -1 (off) or 0..255"); return MS_ERR_INVALID; }
    const int before = g_alloc_fill.exchange((int) byte, std::memory_order_relaxed);
    if (previous) *previous = before;
    return MS_OK;
}

// Every cached block of the calling thread's device back to the driver: the allocations that follow are misses (fresh memory).
int ms_debug_pool_trim(uint64_t *bytes) {
    DeviceCtx *c;
    int rc = get_ctx(g_device, &c);
    if (rc) return rc;
    const size_t freed = pool_trim_current_device();
    if (bytes) *bytes = freed;
    return MS_OK;
}

// Free the calling thread's device work buffers (they are grow-only otherwise); lets a test
// exercise the "buffer too small -> grow -> second pass" path deterministically.
int ms_debug_release_scratch(void) {
    DeviceCtx *c;
    int rc = get_ctx(g_device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    Scratch &sc = c->sc;
    dev_free(sc.cand); dev_free(sc.keys); dev_free(sc.vals); dev_free(sc.keys_sorted); dev_free(sc.chunk_counters);
    sc.chunk_counters_cap = 0;
    if (sc.sort_tmp) (void) hipFree(sc.sort_tmp);
    sc.sort_tmp = nullptr;
    sc.cand_cap = sc.hit_cap = sc.sort_tmp_bytes = 0;
    return MS_OK;
}

}  // extern "C"
