// ms_background.hip -- the two jobs of `motifscan motif --build` / `genome --install` that read the whole genome, on the resident one.
//
//   base_count_kernel    cal_bg_freq (genome/__init__.py:179-220): A / C / G / T per chromosome, both cases.  Every 32-base unit is read
//                        once (8 B of codes + 4 B of nmask).  A non-ACGT base holds code 0 (ms_genome_create_packed validates it), so
//                        C, G and T are popcounts of 2-bit equality masks and A = (code-0 bases) - (nmask bits).  Chromosome boundaries
//                        fall anywhere inside a unit and are masked.  A block owns a contiguous tile of units: each thread keeps the
//                        counts of its current chromosome in registers, flushes them into LDS counters of the block's first kLdsChroms
//                        chromosomes (global atomics past those: genomes of many tiny contigs), and the block adds its LDS counters to
//                        the [n_chroms][4] totals with one 64-bit atomic per non-zero entry.  Integer adds: exact in any order.
//   window_flag_kernel   Genome.random_sequences' N filter (genome/__init__.py:170-175) for candidate windows in attempt order: the
//                        nmask bits of the window minus the exception positions inside it (binary search) -- nmask marks every
//                        non-ACGT byte, the reference counts only N and n -- then one 64-bit ballot per wave of candidates.
//   window_take_kernel   the stable compaction: the first n_want accepted candidates by rank = exclusive prefix of the per-word
//                        popcounts (rocPRIM, exclusive_sum_u32) + popcount of the word below the lane.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "ms_handles.h"

namespace ms {
namespace {

constexpr int kCountThreads = 256;
constexpr int kUnitsPerThread = 16;              // a block's tile: 4096 units = 131072 bases
constexpr int kLdsChroms = 32;
constexpr int kFilterThreads = 256;
constexpr uint64_t kEven = 0x5555555555555555ull;

// the last c with off[c] <= g (off[0] = 0 <= g < off[n]): the chromosome holding base g, never an empty one
__device__ __forceinline__ int64_t chrom_of(const int64_t *__restrict__ off, int64_t n, int64_t g) {
    int64_t lo = 0, hi = n;                      // invariant: off[lo] <= g < off[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// counts of bases [lo, hi) of one unit (0 <= lo < hi <= 32) into a[0..3]
__device__ __forceinline__ void unit_counts(uint64_t cw, uint32_t nm, int lo, int hi, uint32_t a[4]) {
    const uint64_t m = (hi == 32 ? ~0ull : (1ull << (2 * hi)) - 1ull) & ~((1ull << (2 * lo)) - 1ull) & kEven;
    const uint64_t l = cw & kEven, h = (cw >> 1) & kEven;
    const uint32_t nmm = nm & (uint32_t) ((hi == 32 ? 0xFFFFFFFFull : (1ull << hi) - 1ull) & ~((1ull << lo) - 1ull));
    const uint32_t c = (uint32_t) __popcll(l & ~h & m), g = (uint32_t) __popcll(~l & h & m), t = (uint32_t) __popcll(l & h & m);
    a[0] += (uint32_t) (hi - lo) - c - g - t - (uint32_t) __popc(nmm);
    a[1] += c;
    a[2] += g;
    a[3] += t;
}

__global__ __launch_bounds__(kCountThreads) void base_count_kernel(const uint32_t *__restrict__ codes, const uint32_t *__restrict__ nmask,
                                                                  const int64_t *__restrict__ off, int64_t n_chroms, int64_t n_bases,
                                                                  unsigned long long *__restrict__ counts) {
    __shared__ uint32_t lds[kLdsChroms][4];
    const int tid = threadIdx.x;
    const int64_t n_units = (n_bases + 31) >> 5;
    const int64_t tile0 = (int64_t) blockIdx.x * kCountThreads * kUnitsPerThread;
    for (int i = tid; i < kLdsChroms * 4; i += kCountThreads) lds[i >> 2][i & 3] = 0;
    const int64_t cb = chrom_of(off, n_chroms, 32 * tile0);
    __syncthreads();
    uint32_t acc[4] = {0, 0, 0, 0};
    int64_t cur = -1, cur_end = 0;
    auto flush = [&]() {
        if (cur < 0) return;
        if (cur - cb < kLdsChroms) {
            for (int b = 0; b < 4; ++b) if (acc[b]) atomicAdd(&lds[cur - cb][b], acc[b]);
        } else {
            for (int b = 0; b < 4; ++b) if (acc[b]) atomicAdd(&counts[4 * cur + b], (unsigned long long) acc[b]);
        }
        acc[0] = acc[1] = acc[2] = acc[3] = 0;
    };
    for (int i = 0; i < kUnitsPerThread; ++i) {
        const int64_t u = tile0 + (int64_t) i * kCountThreads + tid;
        if (u >= n_units) break;
        const uint2 cw2 = reinterpret_cast<const uint2 *>(codes)[u];
        const uint64_t cw = (uint64_t) cw2.x | ((uint64_t) cw2.y << 32);
        const uint32_t nm = nmask[u];
        int64_t g = 32 * u;
        const int64_t ue = std::min<int64_t>(g + 32, n_bases);
        if (cur < 0 || g >= cur_end) {           // first unit of the thread, or past its chromosome: find the chromosome of base g
            flush();
            cur = chrom_of(off, n_chroms, g);
            cur_end = off[cur + 1];
        }
        while (true) {
            const int64_t e = std::min(ue, cur_end);
            if (e > g) unit_counts(cw, nm, (int) (g - 32 * u), (int) (e - 32 * u), acc);
            if (e >= ue) break;                  // the unit ends inside chromosome cur
            flush();                             // a boundary inside the unit: the rest belongs to the next non-empty chromosomes
            g = e;
            while (off[cur + 1] <= g) ++cur;
            cur_end = off[cur + 1];
        }
    }
    flush();
    __syncthreads();
    for (int i = tid; i < kLdsChroms * 4; i += kCountThreads) {
        const int64_t c = cb + (i >> 2);
        const uint32_t v = lds[i >> 2][i & 3];
        if (v && c < n_chroms) atomicAdd(&counts[4 * c + (i & 3)], (unsigned long long) v);
    }
}

// one thread per candidate k; words[k >> 6] = the wave's ballot of accepted candidates, pop[k >> 6] its popcount
__global__ __launch_bounds__(kFilterThreads) void window_flag_kernel(const uint32_t *__restrict__ nmask, const int64_t *__restrict__ gstart,
                                                                    int64_t n_cand, int32_t length, int32_t max_n,
                                                                    const int64_t *__restrict__ exc_pos, int64_t n_exc,
                                                                    unsigned long long *__restrict__ words, uint32_t *__restrict__ pop) {
    const int64_t k = (int64_t) blockIdx.x * kFilterThreads + threadIdx.x;
    bool ok = false;
    if (k < n_cand) {
        const int64_t g0 = gstart[k], g1 = g0 + length;
        int64_t n = 0;
        for (int64_t u = g0 >> 5; u <= (g1 - 1) >> 5 && g1 > g0; ++u) {
            const int lo = (int) std::max<int64_t>(g0 - 32 * u, 0), hi = (int) std::min<int64_t>(g1 - 32 * u, 32);
            const uint32_t m = (uint32_t) ((hi == 32 ? 0xFFFFFFFFull : (1ull << hi) - 1ull) & ~((1ull << lo) - 1ull));
            n += __popc(nmask[u] & m);
        }
        if (n > max_n && n_exc > 0) {            // exceptions in [g0, g1): lower_bound(g1) - lower_bound(g0)
            int64_t a = 0, b = n_exc;
            while (a < b) { const int64_t mid = (a + b) >> 1; if (exc_pos[mid] < g0) a = mid + 1; else b = mid; }
            int64_t c = a, d = n_exc;
            while (c < d) { const int64_t mid = (c + d) >> 1; if (exc_pos[mid] < g1) c = mid + 1; else d = mid; }
            n -= c - a;
        }
        ok = n <= max_n;
    }
    const unsigned long long bal = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && k < n_cand) {
        words[k >> 6] = bal;
        pop[k >> 6] = (uint32_t) __popcll(bal);
    }
}

__global__ __launch_bounds__(kFilterThreads) void window_take_kernel(const unsigned long long *__restrict__ words, const uint64_t *__restrict__ prefix,
                                                                    int64_t n_cand, int64_t n_want, int64_t *__restrict__ taken) {
    const int64_t k = (int64_t) blockIdx.x * kFilterThreads + threadIdx.x;
    if (k >= n_cand) return;
    const unsigned long long w = words[k >> 6];
    const int s = (int) (k & 63);
    if (!((w >> s) & 1ull)) return;
    const int64_t rank = (int64_t) prefix[k >> 6] + (s ? __popcll(w & ((1ull << s) - 1ull)) : 0);
    if (rank < n_want) taken[rank] = k;
}

}  // namespace
}  // namespace ms

using namespace ms;

extern "C" {

int ms_debug_genome_dims(int32_t out[8]) {
    if (!out) { set_error("NULL out"); return MS_ERR_INVALID; }
    out[0] = kCountThreads * kUnitsPerThread * 32;
    out[1] = kLdsChroms;
    out[2] = kFilterThreads;
    out[3] = seqset_block_bases();
    annotation_dims(out + 4);
    out[7] = (int32_t) score_rank_budget_default();
    return MS_OK;
}

int ms_genome_base_counts(const ms_genome *g, int64_t *counts) {
    if (!g) { set_error("NULL genome"); return MS_ERR_INVALID; }
    const ms_seqset *G = reinterpret_cast<const ms_seqset *>(g);
    const int64_t R = G->R, n = G->n_bases;
    if (R > 0 && !counts) { set_error("NULL counts"); return MS_ERR_INVALID; }
    if (R == 0) return MS_OK;
    std::memset(counts, 0, sizeof(int64_t) * 4 * (size_t) R);
    if (n == 0) return MS_OK;
    DeviceCtx *c;
    int rc = get_ctx(G->device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk_dev(c->mu);
    void *blk = nullptr;
    size_t got = 0;
    const size_t bytes = 8 * 4 * (size_t) R;
    if ((rc = pool_alloc(c, bytes, &blk, &got))) return rc;
    unsigned long long *d_counts = static_cast<unsigned long long *>(blk);
    const hipStream_t st = c->stream;
    const int64_t n_units = (n + 31) / 32, per_block = (int64_t) kCountThreads * kUnitsPerThread;
    hipError_t he = hipMemsetAsync(d_counts, 0, bytes, st);
    if (he == hipSuccess) {
        hipLaunchKernelGGL(base_count_kernel, dim3((unsigned) ((n_units + per_block - 1) / per_block)), dim3(kCountThreads), 0, st, G->d_codes,
                           G->d_nmask, G->d_offsets, R, n, d_counts);
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpyAsync(counts, d_counts, bytes, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    pool_free(c, blk, got);
    if (he != hipSuccess) { set_error("base counts failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    return MS_OK;
}

int ms_genome_window_filter(const ms_genome *g, const int64_t *gstart, int64_t n_cand, int32_t length, int32_t max_n,
                            const int64_t *exc_pos, int64_t n_exc, int64_t n_want, int64_t *taken_idx, int64_t *n_taken) {
    if (!g || !n_taken) { set_error("NULL argument"); return MS_ERR_INVALID; }
    *n_taken = 0;
    if (n_cand < 0 || n_exc < 0 || n_want < 0) { set_error("negative count"); return MS_ERR_INVALID; }
    if (length < 1 || max_n < 0) { set_error("length must be >= 1 and max_n >= 0"); return MS_ERR_INVALID; }
    if ((n_cand > 0 && !gstart) || (n_exc > 0 && !exc_pos) || (n_want > 0 && !taken_idx)) { set_error("NULL array"); return MS_ERR_INVALID; }
    if (n_cand == 0 || n_want == 0) return MS_OK;
    if (n_cand >= (1LL << 40)) { set_error("too many candidates"); return MS_ERR_INVALID; }
    const ms_seqset *G = reinterpret_cast<const ms_seqset *>(g);
    const int64_t n = G->n_bases;
    for (int64_t k = 0; k < n_cand; ++k)          // the kernel reads the nmask words of every window: each must lie inside the genome
        if (gstart[k] < 0 || gstart[k] > n - length) {
            set_error("window %lld: [%lld, %lld) is outside the genome of %lld bases", (long long) k, (long long) gstart[k],
                      (long long) gstart[k] + length, (long long) n);
            return MS_ERR_INVALID;
        }
    for (int64_t i = 1; i < n_exc; ++i)
        if (exc_pos[i] <= exc_pos[i - 1]) { set_error("exc_pos must be strictly ascending (entry %lld)", (long long) i); return MS_ERR_INVALID; }
    DeviceCtx *c;
    int rc = get_ctx(G->device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk_dev(c->mu);
    const hipStream_t st = c->stream;
    const int64_t nw = (n_cand + 63) / 64;
    size_t scan_tmp = 0;
    if ((rc = exclusive_sum_u32(nullptr, &scan_tmp, nullptr, nullptr, (size_t) nw + 1, st))) return rc;
    auto up = [](size_t x) { return (x + 255) & ~(size_t) 255; };
    const size_t b_start = up(8 * (size_t) n_cand), b_exc = up(8 * (size_t) std::max<int64_t>(n_exc, 1)), b_words = up(8 * (size_t) nw),
                 b_pop = up(4 * ((size_t) nw + 1)), b_pre = up(8 * ((size_t) nw + 1)), b_take = up(8 * (size_t) std::min(n_want, n_cand)),
                 b_tmp = up(std::max<size_t>(scan_tmp, 1));
    void *blk = nullptr;
    size_t got = 0;
    if ((rc = pool_alloc(c, b_start + b_exc + b_words + b_pop + b_pre + b_take + b_tmp, &blk, &got))) return rc;
    char *b = static_cast<char *>(blk);
    int64_t *d_start = reinterpret_cast<int64_t *>(b);
    int64_t *d_exc = reinterpret_cast<int64_t *>(b + b_start);
    unsigned long long *d_words = reinterpret_cast<unsigned long long *>(b + b_start + b_exc);
    uint32_t *d_pop = reinterpret_cast<uint32_t *>(b + b_start + b_exc + b_words);
    uint64_t *d_pre = reinterpret_cast<uint64_t *>(b + b_start + b_exc + b_words + b_pop);
    int64_t *d_take = reinterpret_cast<int64_t *>(b + b_start + b_exc + b_words + b_pop + b_pre);
    void *d_tmp = b + b_start + b_exc + b_words + b_pop + b_pre + b_take;
    const unsigned grid = (unsigned) ((n_cand + kFilterThreads - 1) / kFilterThreads);
    hipError_t he = hipMemcpyAsync(d_start, gstart, 8 * (size_t) n_cand, hipMemcpyHostToDevice, st);
    if (he == hipSuccess && n_exc > 0) he = hipMemcpyAsync(d_exc, exc_pos, 8 * (size_t) n_exc, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemsetAsync(d_pop + nw, 0, 4, st);        // pop[nw] = 0: prefix[nw] = the number accepted
    if (he == hipSuccess) {
        hipLaunchKernelGGL(window_flag_kernel, dim3(grid), dim3(kFilterThreads), 0, st, G->d_nmask, d_start, n_cand, length, max_n, d_exc, n_exc,
                           d_words, d_pop);
        he = hipGetLastError();
    }
    if (he != hipSuccess) { pool_free(c, blk, got); set_error("window filter failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    if ((rc = exclusive_sum_u32(d_tmp, &scan_tmp, d_pop, d_pre, (size_t) nw + 1, st))) { pool_free(c, blk, got); return rc; }
    hipLaunchKernelGGL(window_take_kernel, dim3(grid), dim3(kFilterThreads), 0, st, d_words, d_pre, n_cand, n_want, d_take);
    he = hipGetLastError();
    uint64_t accepted = 0;
    if (he == hipSuccess) he = hipMemcpyAsync(&accepted, d_pre + nw, 8, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    const int64_t nt = std::min<int64_t>((int64_t) accepted, n_want);
    if (he == hipSuccess && nt > 0) he = hipMemcpyAsync(taken_idx, d_take, 8 * (size_t) nt, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess && nt > 0) he = hipStreamSynchronize(st);
    pool_free(c, blk, got);
    if (he != hipSuccess) { set_error("window filter failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    *n_taken = nt;
    return MS_OK;
}

int ms_randint_replay_host(const uint32_t *words, int64_t n_words, const int64_t *high, int64_t n_att, int64_t *start,
                           int64_t *words_used, int64_t *n_done) {
    if (!n_done || n_words < 0 || n_att < 0 || (n_words > 0 && !words) || (n_att > 0 && (!high || !start || !words_used))) {
        set_error("bad arguments");
        return MS_ERR_INVALID;
    }
    *n_done = 0;
    int64_t pos = 0;
    for (int64_t k = 0; k < n_att; ++k) {
        if (high[k] < 1 || high[k] > (1LL << 32)) { set_error("attempt %lld: high = %lld outside [1, 2^32]", (long long) k, (long long) high[k]); return MS_ERR_INVALID; }
        const uint32_t rng = (uint32_t) (high[k] - 1);
        uint32_t v = 0;
        if (rng != 0) {
            uint32_t mask = rng;                 // numpy's gen_mask: all bits up to the highest set bit of rng
            mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
            do {
                if (pos >= n_words) return MS_OK;
                v = words[pos++] & mask;
            } while (v > rng);
        }
        start[k] = v;
        words_used[k] = pos;
        *n_done = k + 1;
    }
    return MS_OK;
}

}  // extern "C"
