// ms_kmers.hip -- the k-mer spectrum of a sequence set or of a resident genome (ms_seqset_kmer_counts, ms_genome_kmer_counts): per k-mer
// code the number of windows (occ) and the number of sequences that hold it at least once (nseq).  Integers only: exact in any order.
//
//   kmer_count_kernel    occ.  A block owns tiles of kKmThreads * kKmUnitsPerThread units, as base_count_kernel's (ms_background.hip); a
//                        thread takes one 32-base unit per step with the unit behind it (a window of k <= 12 bases touches two units;
//                        the read of unit u + 1 is guarded: nothing here relies on what lies behind the planes).  The 32-bit mask of valid
//                        starts = (starts of a selected sequence, at least k bases before its end: the chromosome walk of
//                        base_count_kernel) & ~(OR of k shifts of the 64-bit non-ACGT mask pair).  Per valid start the window's 2k bits
//                        in the planes' order (first base lowest) are the reverse complement's code once complemented; the forward code
//                        is the same bits with their 2-bit groups reversed (__brevll, then the two bits of every group swapped).  Equal
//                        codes of a thread's starts are merged into one add: a homopolymer run is one add per thread, not one per
//                        start, and in the global tier (four (code, count) register pairs) so is a microsatellite of a period up to four.
//                        k <= kKmLdsK: the adds go to a block table of 4^k 32-bit LDS counters, flushed with one 64-bit global atomic per
//                        non-zero entry (a block walks several tiles between flushes); above: 64-bit global atomics directly.
//   kmer_sort_kernel     nseq of the sequences of at most kKmSortWindows windows: one block per sequence, the codes in LDS (a left-out
//                        window is a sentinel that sorts last), a bitonic sort, and the head of every run of equal codes adds 1.
//   kmer_bitmap_kernel   nseq of the longer sequences: a bitmap of 4^k bits per sequence in pooled scratch, cleared per batch of
//                        sequences whose bitmaps fit the budget.  The blocks of a sequence's tiles set bits with a RETURNING atomicOr: of
//                        all the threads that meet a code of the sequence exactly one sees the bit clear, whatever the order, and that one
//                        adds 1.  (A plain read in front skips the atomic where the bit is seen set: bits are only ever set within a batch, so
//                        a stale read can only send a thread to the atomic, which decides.)
#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <vector>

#include "ms_handles.h"

namespace ms {
namespace {

constexpr int kKmThreads = 256;
constexpr int kKmUnitsPerThread = 16;            // a block's tile: 4096 units = 131072 bases
constexpr int kKmLdsK = 7;                       // 4^7 counters x 4 B = 64 KiB: two blocks per CU of 160 KiB
constexpr int kKmSlots = 4;                      // (code, count) pairs a thread of the global tier merges its adds through
constexpr int kKmFlushTiles = 8192;             // tiles between two flushes of the LDS table: 2^30 windows, no 32-bit counter can wrap
constexpr int kKmSortWindows = 4096;             // 16 KiB of codes per block
constexpr int kKmSortSeqs = 1;                   // sequences per block of the sort tier
constexpr int kKmBitmapStarts = 64;              // window starts per thread of the bitmap tier: a block's tile is 16384 starts
constexpr int64_t kKmBitmapBudgetMiB = 64;       // 32 bitmaps at k = 12: the chromosomes of a genome are one batch
constexpr uint64_t kKmEven = 0x5555555555555555ull;
constexpr uint32_t kKmNoCode = 0xFFFFFFFFu;

std::atomic<int64_t> g_km_budget{0};             // ms_debug_kmer_bitmap_budget: 0 = kKmBitmapBudgetMiB

struct KmArgs {
    const uint32_t *codes;
    const uint32_t *nmask;
    const int64_t *off;
    int64_t R, n_bases;
    const uint8_t *sel;                          // [R] or nullptr: all
    int k;
    int canonical;
};

// the last r with off[r] <= g (off[0] = 0 <= g < off[n]): the sequence holding base g, never an empty one
__device__ __forceinline__ int64_t km_seq_of(const int64_t *__restrict__ off, int64_t n, int64_t g) {
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// the code of the window of k bases at base i (0 .. 31) of the unit pair (w0, w1); the window holds no non-ACGT base
__device__ __forceinline__ uint32_t km_code(uint64_t w0, uint64_t w1, int i, int k, int canonical) {
    const uint64_t kmask = (1ull << (2 * k)) - 1ull;
    const uint64_t nat = ((w0 >> (2 * i)) | (i ? w1 << (64 - 2 * i) : 0ull)) & kmask;     // base j of the window at bits [2j, 2j + 2)
    uint64_t r = __brevll(nat);                                                         // group j -> group 31 - j, its two bits swapped
    r = ((r >> 1) & kKmEven) | ((r & kKmEven) << 1);
    const uint32_t fwd = (uint32_t) (r >> (64 - 2 * k));
    const uint32_t rc = (uint32_t) (~nat & kmask);
    return canonical && rc < fwd ? rc : fwd;
}

// bits [lo, hi) of a 32-bit word, 0 <= lo < hi <= 32
__device__ __forceinline__ uint32_t km_range(int lo, int hi) {
    return (uint32_t) ((hi == 32 ? 0xFFFFFFFFull : (1ull << hi) - 1ull) & ~((1ull << lo) - 1ull));
}

template <bool kLds>
__global__ __launch_bounds__(kKmThreads) void kmer_count_kernel(KmArgs A, int64_t n_tiles, unsigned long long *__restrict__ occ,
                                                               unsigned long long *__restrict__ n_counted) {
    extern __shared__ unsigned long long km_dyn[];          // the block's window count, then [4^k] 32-bit counters when kLds
    unsigned long long &s_counted = km_dyn[0];
    uint32_t *km_tab = reinterpret_cast<uint32_t *>(km_dyn + 1);
    const int tid = threadIdx.x, k = A.k;
    const int64_t n_units = (A.n_bases + 31) >> 5;
    const uint32_t n_codes = 1u << (2 * k);
    if (kLds) for (uint32_t i = tid; i < n_codes; i += kKmThreads) km_tab[i] = 0;
    if (tid == 0) s_counted = 0;
    __syncthreads();
    auto flush_table = [&]() {                   // all threads
        __syncthreads();
        for (uint32_t i = tid; i < n_codes; i += kKmThreads) {
            const uint32_t v = km_tab[i];
            if (v) { atomicAdd(&occ[i], (unsigned long long) v); km_tab[i] = 0; }
        }
        __syncthreads();
    };
    unsigned long long counted = 0;
    // Equal codes of a thread's starts are merged before the add, through kSlots (code, count) pairs in registers: a homopolymer run is
    // one add per thread, not one per start, and with the global tier's four pairs so is a microsatellite of a period up to four (its
    // codes take turns; two hot global words took 222 ms per 10^8 bases of poly-A + (AC)n with one pair, 1.8 ms with four).  A code
    // that is in no pair takes the place of the oldest one, which is added then.  The LDS tier keeps one pair: the compares cost more
    // there than the LDS adds they save (250 Mbase at k = 7: 0.46 ms with one pair, 1.10 ms with four).  Indices are constants after unrolling.
    constexpr int kSlots = kLds ? 1 : kKmSlots;
    uint32_t slot_code[kSlots], slot_n[kSlots];
#pragma unroll
    for (int j = 0; j < kSlots; ++j) slot_code[j] = slot_n[j] = 0;
    int victim = 0;
    auto add = [&](uint32_t code, uint32_t n) {
        if (kLds) atomicAdd(&km_tab[code], n); else atomicAdd(&occ[code], (unsigned long long) n);
    };
    auto count = [&](uint32_t code) {
        bool hit = false;
#pragma unroll
        for (int j = 0; j < kSlots; ++j)
            if (!hit && slot_n[j] && slot_code[j] == code) { ++slot_n[j]; hit = true; }
        if (hit) return;
#pragma unroll
        for (int j = 0; j < kSlots; ++j)
            if (j == victim) {
                if (slot_n[j]) add(slot_code[j], slot_n[j]);
                slot_code[j] = code;
                slot_n[j] = 1;
            }
        victim = (victim + 1) % kSlots;
    };
    auto emit = [&]() {
#pragma unroll
        for (int j = 0; j < kSlots; ++j) {
            if (slot_n[j]) add(slot_code[j], slot_n[j]);
            slot_n[j] = 0;
        }
    };
    int since_flush = 0;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t tile0 = t * kKmThreads * kKmUnitsPerThread;
        int64_t cur = -1, cur_end = 0;
        bool cur_sel = false;
        for (int s = 0; s < kKmUnitsPerThread; ++s) {
            const int64_t u = tile0 + (int64_t) s * kKmThreads + tid;
            if (u >= n_units) break;
            const uint2 a2 = reinterpret_cast<const uint2 *>(A.codes)[u];
            const uint64_t w0 = (uint64_t) a2.x | ((uint64_t) a2.y << 32);
            uint64_t w1 = 0, nm = A.nmask[u];
            if (u + 1 < n_units) {               // the unit behind: guarded, the planes promise nothing past the last unit
                const uint2 b2 = reinterpret_cast<const uint2 *>(A.codes)[u + 1];
                w1 = (uint64_t) b2.x | ((uint64_t) b2.y << 32);
                nm |= (uint64_t) A.nmask[u + 1] << 32;
            }
            int64_t g = 32 * u;
            const int64_t ue = std::min<int64_t>(g + 32, A.n_bases);
            if (cur < 0 || g >= cur_end) {       // first unit of the thread in this tile, or past its sequence
                cur = km_seq_of(A.off, A.R, g);
                cur_end = A.off[cur + 1];
                cur_sel = !A.sel || A.sel[cur];
            }
            uint32_t starts = 0;
            while (true) {
                const int64_t e = std::min<int64_t>(ue, cur_end);
                if (cur_sel) {
                    const int64_t hi = std::min<int64_t>(e, cur_end - k + 1);      // the last start of the sequence is its end - k
                    if (hi > g) starts |= km_range((int) (g - 32 * u), (int) (hi - 32 * u));
                }
                if (e >= ue) break;              // the unit ends inside sequence cur
                g = e;                           // a boundary inside the unit: on to the next non-empty sequence
                while (A.off[cur + 1] <= g) ++cur;
                cur_end = A.off[cur + 1];
                cur_sel = !A.sel || A.sel[cur];
            }
            uint64_t bad = 0;
            for (int j = 0; j < k; ++j) bad |= nm >> j;
            uint32_t valid = starts & ~(uint32_t) bad;
            counted += (unsigned) __popc(valid);
            while (valid) {
                const int i = __ffs((int) valid) - 1;
                valid &= valid - 1;
                count(km_code(w0, w1, i, k, A.canonical));
            }
        }
        if (kLds && ++since_flush == kKmFlushTiles) { emit(); flush_table(); since_flush = 0; }
    }
    emit();
    if (counted) atomicAdd(&s_counted, counted);
    if (kLds) flush_table(); else __syncthreads();
    if (tid == 0 && s_counted) atomicAdd(n_counted, s_counted);
}

// the code of the window at base g of the planes, or false when it holds a non-ACGT base
__device__ __forceinline__ bool km_window(const KmArgs &A, int64_t n_units, int64_t g, uint32_t *code) {
    const int64_t u = g >> 5;
    const int i = (int) (g & 31);
    const uint2 a2 = reinterpret_cast<const uint2 *>(A.codes)[u];
    const uint64_t w0 = (uint64_t) a2.x | ((uint64_t) a2.y << 32);
    uint64_t w1 = 0, nm = A.nmask[u];
    if (i + A.k > 32 && u + 1 < n_units) {
        const uint2 b2 = reinterpret_cast<const uint2 *>(A.codes)[u + 1];
        w1 = (uint64_t) b2.x | ((uint64_t) b2.y << 32);
        nm |= (uint64_t) A.nmask[u + 1] << 32;
    }
    if ((nm >> i) & ((1ull << A.k) - 1ull)) return false;
    *code = km_code(w0, w1, i, A.k, A.canonical);
    return true;
}

// block r: sequence r, if it is selected and has 1 .. kKmSortWindows windows
__global__ __launch_bounds__(kKmThreads) void kmer_sort_kernel(KmArgs A, unsigned long long *__restrict__ nseq) {
    __shared__ uint32_t s[kKmSortWindows];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    if (A.sel && !A.sel[r]) return;
    const int64_t b = A.off[r], nw64 = A.off[r + 1] - b - A.k + 1;
    if (nw64 < 1 || nw64 > kKmSortWindows) return;
    const int nw = (int) nw64;
    const int64_t n_units = (A.n_bases + 31) >> 5;
    int n_pad = 2;
    while (n_pad < nw) n_pad <<= 1;
    for (int i = tid; i < n_pad; i += kKmThreads) {
        uint32_t code = kKmNoCode;
        if (i < nw && !km_window(A, n_units, b + i, &code)) code = kKmNoCode;
        s[i] = code;
    }
    __syncthreads();
    for (int size = 2; size <= n_pad; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (n_pad >> 1); t += kKmThreads) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const uint32_t x = s[lo], y = s[hi];
                if ((x > y) == ((lo & size) == 0)) { s[lo] = y; s[hi] = x; }
            }
            __syncthreads();
        }
    for (int i = tid; i < nw; i += kKmThreads) {
        const uint32_t c = s[i];
        if (c != kKmNoCode && (i == 0 || s[i - 1] != c)) atomicAdd(&nseq[c], 1ull);
    }
}

// block t: tile t - tile_first[j] of the j-th sequence of the batch (tile_first[0] = 0, tile_first[nb] = the grid)
__global__ __launch_bounds__(kKmThreads) void kmer_bitmap_kernel(KmArgs A, const int64_t *__restrict__ bseq, const int64_t *__restrict__ tile_first, int nb,
                                                                uint32_t *__restrict__ bitmaps, int64_t words_per_map, unsigned long long *__restrict__ nseq) {
    const int64_t t = blockIdx.x;
    int lo = 0, hi = nb;                         // invariant: tile_first[lo] <= t < tile_first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile_first[mid] <= t) lo = mid; else hi = mid;
    }
    const int64_t r = bseq[lo], b = A.off[r], nw = A.off[r + 1] - b - A.k + 1;
    const int64_t tile = (int64_t) kKmThreads * kKmBitmapStarts;
    const int64_t s0 = (t - tile_first[lo]) * tile, s1 = std::min<int64_t>(s0 + tile, nw);
    const int64_t n_units = (A.n_bases + 31) >> 5;
    uint32_t *bm = bitmaps + (int64_t) lo * words_per_map;
    uint32_t last = kKmNoCode;
    for (int64_t s = s0 + threadIdx.x; s < s1; s += kKmThreads) {
        uint32_t code;
        if (!km_window(A, n_units, b + s, &code) || code == last) continue;
        last = code;
        const uint32_t bit = 1u << (code & 31);
        uint32_t *w = bm + (code >> 5);
        if (*w & bit) continue;
        if (!(atomicOr(w, bit) & bit)) atomicAdd(&nseq[code], 1ull);
    }
}

// host or device memory of `device`?  -1: a device pointer of another device
int km_where(const void *p, int device, bool *on_device) {
    hipPointerAttribute_t attr;
    std::memset(&attr, 0, sizeof(attr));
    *on_device = hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeDevice;
    (void) hipGetLastError();                    // a pageable host pointer is "not found" here, which is no error
    if (*on_device && attr.device != device) { set_error("output lives on device %d, the sequences on device %d", attr.device, device); return -1; }
    return 0;
}

int kmer_counts(const ms_seqset *seqs, const char *what, int32_t k, uint32_t flags, const uint8_t *sel, int64_t *occ, int64_t *nseq, int64_t *totals,
                double *device_ms) {
    if (!require_device()) return MS_ERR_RUNTIME;
    if (device_ms) *device_ms = 0.0;
    if (!seqs) { set_error("NULL handle"); return MS_ERR_INVALID; }
    if (!occ) { set_error("NULL occ"); return MS_ERR_INVALID; }
    if (k < 1 || k > MS_KMER_MAX_K) { set_error("k must be in [1, %d]", MS_KMER_MAX_K); return MS_ERR_INVALID; }
    if (flags & ~MS_KMER_CANONICAL) { set_error("unknown k-mer flags 0x%x", flags); return MS_ERR_INVALID; }
    if (!seqs->built || seqs->pack_pending || !seqs->block) { set_error("the set's planes are not on the device yet (packed by its first scan)"); return MS_ERR_INVALID; }
    const int64_t R = seqs->R, n_bases = seqs->n_bases;
    if (R > 0x7FFFFFFFLL) { set_error("too many %ss for one launch", what); return MS_ERR_INVALID; }
    bool occ_dev = false, nseq_dev = false;
    if (km_where(occ, seqs->device, &occ_dev)) return MS_ERR_INVALID;
    if (nseq && km_where(nseq, seqs->device, &nseq_dev)) return MS_ERR_INVALID;
    const size_t n_codes = (size_t) 1 << (2 * k), out_bytes = 8 * n_codes;
    const int64_t words_per_map = (int64_t) ((n_codes + 31) / 32);

    // ---- the plan, on the host: the totals that need no device, the long sequences and their batches
    const int64_t *off = seqs->offsets.data();
    int64_t n_sel = 0, n_windows = 0, n_short = 0;
    bool any_sort = false;
    std::vector<int64_t> lseq, ltile;            // the long sequences; per batch nb + 1 tile offsets
    std::vector<int64_t> batch_first;            // [batches + 1] into lseq
    const int64_t tile = (int64_t) kKmThreads * kKmBitmapStarts;
    int64_t budget = g_km_budget.load();
    if (budget <= 0) budget = kKmBitmapBudgetMiB << 20;
    const int64_t per_batch = std::max<int64_t>(1, budget / (4 * words_per_map));
    int64_t max_nb = 0;
    try {
        for (int64_t r = 0; r < R; r++) {
            if (sel && !sel[r]) continue;
            n_sel++;
            const int64_t nw = off[r + 1] - off[r] - k + 1;
            if (nw < 1) { n_short++; continue; }
            n_windows += nw;
            if (nw <= kKmSortWindows) any_sort = true;
            else if (nseq) lseq.push_back(r);
        }
        batch_first.push_back(0);
        for (size_t i = 0; i < lseq.size();) {
            const size_t j = std::min(lseq.size(), i + (size_t) per_batch);
            int64_t tiles = 0;
            for (size_t q = i; q < j; q++) {
                ltile.push_back(tiles);
                tiles += (off[lseq[q] + 1] - off[lseq[q]] - k + 1 + tile - 1) / tile;
            }
            ltile.push_back(tiles);
            if (tiles > 0x7FFFFFFFLL) { set_error("too many tiles for one launch"); return MS_ERR_INVALID; }
            max_nb = std::max<int64_t>(max_nb, (int64_t) (j - i));
            batch_first.push_back((int64_t) j);
            i = j;
        }
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    const size_t n_batches = batch_first.size() - 1;
    const bool run = n_windows > 0;

    DeviceCtx *c;
    int rc = get_ctx(seqs->device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk_dev(c->mu);
    MS_HIP(hipSetDevice(c->device));
    const size_t b_occ = occ_dev ? 0 : up256(out_bytes), b_nseq = (!nseq || nseq_dev) ? 0 : up256(out_bytes), b_sel = (sel && run) ? up256((size_t) R) : 0,
                 b_lseq = up256(8 * std::max<size_t>(lseq.size(), 1)), b_ltile = up256(8 * std::max<size_t>(ltile.size(), 1)),
                 b_maps = up256(4 * (size_t) words_per_map * (size_t) max_nb);
    void *wblk = nullptr;
    size_t wgot = 0;
    if ((rc = pool_alloc(c, 256 + b_occ + b_nseq + b_sel + b_lseq + b_ltile + b_maps, &wblk, &wgot))) return rc;      // nothing is launched before this
    auto fail = [&](int code) { (void) hipStreamSynchronize(c->stream); pool_free(c, wblk, wgot); return code; };
    auto hip_fail = [&](hipError_t e, const char *w) { set_error("%s failed: %s", w, hipGetErrorString(e)); return fail(e == hipErrorOutOfMemory ? MS_ERR_NOMEM : MS_ERR_RUNTIME); };
    char *p = static_cast<char *>(wblk);
    unsigned long long *d_counted = reinterpret_cast<unsigned long long *>(p); p += 256;
    unsigned long long *d_occ = occ_dev ? reinterpret_cast<unsigned long long *>(occ) : reinterpret_cast<unsigned long long *>(p); p += b_occ;
    unsigned long long *d_nseq = !nseq ? nullptr : nseq_dev ? reinterpret_cast<unsigned long long *>(nseq) : reinterpret_cast<unsigned long long *>(p); p += b_nseq;
    uint8_t *d_sel = reinterpret_cast<uint8_t *>(p); p += b_sel;
    int64_t *d_lseq = reinterpret_cast<int64_t *>(p); p += b_lseq;
    int64_t *d_ltile = reinterpret_cast<int64_t *>(p); p += b_ltile;
    uint32_t *d_maps = reinterpret_cast<uint32_t *>(p);

    const hipStream_t st = c->stream;
    hipError_t he = hipMemsetAsync(d_occ, 0, out_bytes, st);
    if (he == hipSuccess && d_nseq) he = hipMemsetAsync(d_nseq, 0, out_bytes, st);
    if (he == hipSuccess) he = hipMemsetAsync(d_counted, 0, 8, st);
    if (he != hipSuccess) return hip_fail(he, "clearing the counts");
    unsigned long long counted = 0;
    float ms01 = 0;
    if (run) {
        if (sel) he = hipMemcpyAsync(d_sel, sel, (size_t) R, hipMemcpyHostToDevice, st);
        if (he == hipSuccess && !lseq.empty()) he = hipMemcpyAsync(d_lseq, lseq.data(), 8 * lseq.size(), hipMemcpyHostToDevice, st);
        if (he == hipSuccess && !ltile.empty()) he = hipMemcpyAsync(d_ltile, ltile.data(), 8 * ltile.size(), hipMemcpyHostToDevice, st);
        if (he != hipSuccess) return hip_fail(he, "upload of the plan");
        KmArgs A;
        A.codes = seqs->d_codes; A.nmask = seqs->d_nmask; A.off = seqs->d_offsets; A.R = R; A.n_bases = n_bases;
        A.sel = sel ? d_sel : nullptr;
        A.k = k;
        A.canonical = (flags & MS_KMER_CANONICAL) ? 1 : 0;
        const int64_t n_units = (n_bases + 31) / 32, per_tile = (int64_t) kKmThreads * kKmUnitsPerThread;
        const int64_t n_tiles = (n_units + per_tile - 1) / per_tile;
        const int n_cu = std::max(c->n_cu, 1);
        (void) hipEventRecord(c->ev[0], st);
        if (k <= kKmLdsK) {
            const size_t lds = 8 + 4 * n_codes;
            if (lds > 48 * 1024) {
                he = hipFuncSetAttribute(reinterpret_cast<const void *>(kmer_count_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int) (8 + (4u << (2 * kKmLdsK))));
                if (he != hipSuccess) return hip_fail(he, "raising the LDS limit");
            }
            const int per_cu = (int) std::max<size_t>(1, std::min<size_t>(4, (size_t) (160 * 1024) / (lds + 64)));
            const unsigned grid = (unsigned) std::min<int64_t>(n_tiles, (int64_t) n_cu * per_cu);
            hipLaunchKernelGGL(kmer_count_kernel<true>, dim3(grid), dim3(kKmThreads), lds, st, A, n_tiles, d_occ, d_counted);
        } else {
            const unsigned grid = (unsigned) std::min<int64_t>(n_tiles, (int64_t) n_cu * 8);
            hipLaunchKernelGGL(kmer_count_kernel<false>, dim3(grid), dim3(kKmThreads), 8, st, A, n_tiles, d_occ, d_counted);
        }
        if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "k-mer count kernel");
        if (d_nseq && any_sort) {
            hipLaunchKernelGGL(kmer_sort_kernel, dim3((unsigned) R), dim3(kKmThreads), 0, st, A, d_nseq);
            if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "k-mer presence kernel (sorted)");
        }
        if (d_nseq) {
            size_t t0 = 0;                       // the batch's tile offsets in ltile
            for (size_t bi = 0; bi < n_batches; bi++) {
                const int64_t q0 = batch_first[bi], nb = batch_first[bi + 1] - q0;
                const int64_t tiles = ltile[t0 + (size_t) nb];
                he = hipMemsetAsync(d_maps, 0, 4 * (size_t) words_per_map * (size_t) nb, st);
                if (he != hipSuccess) return hip_fail(he, "clearing the bitmaps");
                if (tiles > 0) {
                    hipLaunchKernelGGL(kmer_bitmap_kernel, dim3((unsigned) tiles), dim3(kKmThreads), 0, st, A, d_lseq + q0, d_ltile + t0, (int) nb, d_maps, words_per_map,
                                       d_nseq);
                    if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "k-mer presence kernel (bitmaps)");
                }
                t0 += (size_t) nb + 1;
            }
        }
        (void) hipEventRecord(c->ev[1], st);
        he = hipMemcpyAsync(&counted, d_counted, 8, hipMemcpyDeviceToHost, st);
        if (he != hipSuccess) return hip_fail(he, "copy of the window count");
    }
    if (!occ_dev) he = hipMemcpyAsync(occ, d_occ, out_bytes, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess && nseq && !nseq_dev) he = hipMemcpyAsync(nseq, d_nseq, out_bytes, hipMemcpyDeviceToHost, st);
    if (he != hipSuccess) return hip_fail(he, "copy of the counts");
    he = hipStreamSynchronize(st);
    if (he != hipSuccess) return hip_fail(he, "k-mer counts");
    if (run) (void) hipEventElapsedTime(&ms01, c->ev[0], c->ev[1]);
    if (device_ms) *device_ms = ms01;
    pool_free(c, wblk, wgot);
    if (totals) {
        totals[0] = n_sel;
        totals[1] = (int64_t) counted;
        totals[2] = n_windows - (int64_t) counted;
        totals[3] = n_short;
    }
    return MS_OK;
}

}  // namespace
}  // namespace ms

using namespace ms;

extern "C" {

int ms_debug_kmer_dims(int32_t out[8]) {
    if (!out) { set_error("NULL output"); return MS_ERR_INVALID; }
    out[0] = kKmThreads;
    out[1] = kKmThreads * kKmUnitsPerThread * 32;
    out[2] = kKmLdsK;
    out[3] = kKmSortWindows;
    out[4] = kKmSortSeqs;
    out[5] = (int32_t) kKmBitmapBudgetMiB;
    out[6] = out[7] = 0;
    return MS_OK;
}

int ms_debug_kmer_bitmap_budget(int64_t bytes, int64_t *previous) {
    if (bytes < 0) { set_error("budget must be >= 0 (0 = the library's own)"); return MS_ERR_INVALID; }
    const int64_t old = g_km_budget.exchange(bytes);
    if (previous) *previous = old;
    return MS_OK;
}

int ms_debug_seqset_upload_only(const char *bases, const int64_t *offsets, int64_t n_seqs, ms_seqset **out) {
    if (!require_device()) return MS_ERR_RUNTIME;
    return seqset_create_upload_only(bases, offsets, n_seqs, out);
}

int ms_seqset_kmer_counts(const ms_seqset *seqs, int32_t k, uint32_t flags, const uint8_t *sel, int64_t *occ, int64_t *nseq, int64_t *totals, double *device_ms) {
    return kmer_counts(seqs, "sequence", k, flags, sel, occ, nseq, totals, device_ms);
}

int ms_genome_kmer_counts(const ms_genome *genome, int32_t k, uint32_t flags, const uint8_t *sel_chrom, int64_t *occ, int64_t *nseq, int64_t *totals,
                          double *device_ms) {
    return kmer_counts(reinterpret_cast<const ms_seqset *>(genome), "chromosome", k, flags, sel_chrom, occ, nseq, totals, device_ms);
}

}  // extern "C"
