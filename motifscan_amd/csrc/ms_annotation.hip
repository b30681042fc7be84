// ms_annotation.hip -- the gene-annotation work of `motifscan scan` in front of the scan: region/utils.py's per-region walks over a
// chromosome's genes, on the device, and the seeded draws of generate_control_regions replayed on the host.
//
//   nearest_tss_kernel       dis_to_nearest_gene (region/utils.py:148-180) for every region: NOT the nearest TSS but the reference's
//                            recurrence over the chromosome's genes IN FILE ORDER -- m = cutoff; for each gene d = start - tss;
//                            |d| < m: m = d (signed), target = gene.  The entry groups the regions by chromosome on the host, so a
//                            block's 256 regions share one gene list: the list goes through LDS in tiles of kGeneTile keys
//                            (key = tss << 1 | minus strand, one 64-bit word per gene) and every lane of a wave reads the same key, a
//                            broadcast.  A lane whose m is <= 0 can never accept again (|d| < m is false for good): a wave of such
//                            lanes skips the tile's walk, a block of them leaves the gene loop.
//   promoter_overlap_kernel  overlap_with (region/utils.py:16-48) as subset_by_location calls it: the LITERAL binary search, one
//                            region per lane, over its chromosome's promoter intervals sorted as Python sorts lists of pairs.
//   ms_control_regions_replay_host   generate_control_regions' draws (region/utils.py:112-145) from the raw 32-bit words Python's
//                            generator would give: randint / choice are a + _randbelow(n), _randbelow(n) = words >> (32 - bitlen(n))
//                            until one is < n.  No device.
#include <algorithm>
#include <climits>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

#include "ms_handles.h"

struct ms_genes {
    int32_t n_chroms = 0;
    std::vector<int64_t> off;        // [n_chroms + 1] into the arrays below: a chromosome's genes in file order
    std::vector<int64_t> tss;
    std::vector<int8_t> strand;      // MS_STRAND_FWD / MS_STRAND_REV
    std::mutex mu;                   // the device copies below (taken before DeviceCtx::mu)
    int device = -1;                 // bound by the first device call
    int64_t *d_off = nullptr;
    int64_t *d_key = nullptr;        // tss << 1 | (strand == '-')
    bool prom_valid = false;         // the promoter table of (prom_up, prom_down) is on the device
    int64_t prom_up = 0, prom_down = 0;
    int64_t *d_plo = nullptr, *d_phi = nullptr;
};

namespace ms {
namespace {

constexpr int kNearThreads = 256;
constexpr int kGeneTile = 2048;                  // 16 KiB of LDS per block
constexpr int kOverlapThreads = 256;
constexpr int64_t kCoordMax = 1LL << 60;         // |tss|, |start|, |end|, cutoff, upstream, downstream below this: no difference overflows

struct NearBlock {                               // one block of nearest_tss_kernel: `count` (<= kNearThreads) regions of one chromosome
    int64_t first;                               // ... at [first, first + count) of the grouped arrays
    int32_t chrom;
    int32_t count;
};

__global__ __launch_bounds__(kNearThreads) void nearest_tss_kernel(const int64_t *__restrict__ key, const int64_t *__restrict__ off,
                                                                  const NearBlock *__restrict__ blocks, const int64_t *__restrict__ start,
                                                                  int64_t cutoff, int64_t *__restrict__ distance, uint8_t *__restrict__ found) {
    __shared__ int64_t tile[kGeneTile];
    const NearBlock b = blocks[blockIdx.x];
    const int tid = threadIdx.x;
    const bool live = tid < b.count;
    const int64_t g0 = off[b.chrom], g1 = off[b.chrom + 1];
    const int64_t s = live ? start[b.first + tid] : 0;
    int64_t m = live ? cutoff : 0;               // an idle lane is frozen from the start
    int64_t minus = 0;
    bool hit = false;
    for (int64_t t0 = g0; t0 < g1; t0 += kGeneTile) {
        if (!__syncthreads_or(m > 0)) break;     // (also the barrier between the last tile's reads and this tile's writes)
        const int n = (int) std::min<int64_t>(kGeneTile, g1 - t0);
        for (int i = tid; i < n; i += kNearThreads) tile[i] = key[t0 + i];
        __syncthreads();
        if (__ballot(m > 0) == 0) continue;      // every lane of the wave is frozen
#pragma unroll 8
        for (int i = 0; i < n; ++i) {
            const int64_t k = tile[i];           // the same address in every lane: a broadcast
            const int64_t d = s - (k >> 1);
            const int64_t a = d < 0 ? -d : d;
            if (a < m) {                         // never true again once m <= 0
                m = d;
                minus = k & 1;
                hit = true;
            }
        }
    }
    if (live) {
        distance[b.first + tid] = hit ? (minus ? -m : m) : 0;
        found[b.first + tid] = hit ? 1 : 0;
    }
}

__global__ __launch_bounds__(kOverlapThreads) void promoter_overlap_kernel(const int64_t *__restrict__ plo, const int64_t *__restrict__ phi,
                                                                          const int64_t *__restrict__ off, int32_t n_chroms,
                                                                          const int32_t *__restrict__ chrom, const int64_t *__restrict__ start,
                                                                          const int64_t *__restrict__ end, int64_t n, uint8_t *__restrict__ overlap) {
    const int64_t r = (int64_t) blockIdx.x * kOverlapThreads + threadIdx.x;
    if (r >= n) return;
    const int32_t c = chrom[r];
    uint8_t res = 0;
    if (c >= 0 && c < n_chroms) {
        const int64_t base = off[c], s = start[r], e = end[r];
        int64_t left = 0, right = off[c + 1] - base - 1;
        while (left <= right) {
            const int64_t mid = (left + right) >> 1;             // both >= 0: the reference's floor division
            const int64_t lo = plo[base + mid], hi = phi[base + mid];
            if (!(e <= lo || s >= hi)) { res = 1; break; }
            if (s >= hi) left = mid + 1; else right = mid - 1;   // the reference tests start >= end_ref first
        }
    }
    overlap[r] = res;
}

// the handle's gene table on its device (the calling thread's device at the first call); the caller holds g->mu
int genes_upload(ms_genes *g, DeviceCtx **ctx) {
    const int device = g->device >= 0 ? g->device : current_device();
    int rc = get_ctx(device, ctx);
    if (rc) return rc;
    if (g->d_key) return MS_OK;
    const size_t n = g->tss.size();
    std::vector<int64_t> key(std::max<size_t>(n, 1), 0);
    for (size_t i = 0; i < n; ++i) key[i] = g->tss[i] * 2 + (g->strand[i] == MS_STRAND_REV ? 1 : 0);
    if ((rc = dev_alloc(&g->d_off, g->off.size()))) return rc;
    if ((rc = dev_alloc(&g->d_key, key.size()))) { dev_free(g->d_off); return rc; }
    hipError_t he = hipMemcpy(g->d_off, g->off.data(), 8 * g->off.size(), hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(g->d_key, key.data(), 8 * key.size(), hipMemcpyHostToDevice);
    if (he != hipSuccess) {
        dev_free(g->d_off);
        dev_free(g->d_key);
        set_error("gene table upload failed: %s", hipGetErrorString(he));
        return MS_ERR_RUNTIME;
    }
    g->device = device;
    return MS_OK;
}

// the promoter intervals of (up, down), per chromosome in the order of Python's sort of [lo, hi] lists; the caller holds g->mu
int promoters_upload(ms_genes *g, int64_t up, int64_t down) {
    if (g->prom_valid && g->prom_up == up && g->prom_down == down) return MS_OK;
    const size_t n = g->tss.size();
    std::vector<std::pair<int64_t, int64_t>> iv(n);
    for (size_t i = 0; i < n; ++i)
        iv[i] = g->strand[i] == MS_STRAND_REV ? std::make_pair(g->tss[i] - down, g->tss[i] + up) : std::make_pair(g->tss[i] - up, g->tss[i] + down);
    for (int32_t c = 0; c < g->n_chroms; ++c) std::sort(iv.begin() + g->off[c], iv.begin() + g->off[c + 1]);
    std::vector<int64_t> lo(std::max<size_t>(n, 1), 0), hi(std::max<size_t>(n, 1), 0);
    for (size_t i = 0; i < n; ++i) { lo[i] = iv[i].first; hi[i] = iv[i].second; }
    int rc;
    if (!g->d_plo && (rc = dev_alloc(&g->d_plo, lo.size()))) return rc;
    if (!g->d_phi && (rc = dev_alloc(&g->d_phi, hi.size()))) return rc;
    g->prom_valid = false;
    hipError_t he = hipMemcpy(g->d_plo, lo.data(), 8 * lo.size(), hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(g->d_phi, hi.data(), 8 * hi.size(), hipMemcpyHostToDevice);
    if (he != hipSuccess) { set_error("promoter table upload failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    g->prom_valid = true;
    g->prom_up = up;
    g->prom_down = down;
    return MS_OK;
}

inline bool coord_ok(int64_t v) { return v > -kCoordMax && v < kCoordMax; }

// Python's Random._randbelow(n) for 1 <= n < 2^32 from raw words: k = n.bit_length(), r = word >> (32 - k) until r < n
inline bool randbelow(const uint32_t *words, int64_t n_words, int64_t &pos, uint32_t n, int64_t *out) {
    int k = 0;
    for (uint32_t v = n; v; v >>= 1) ++k;
    uint32_t r;
    do {
        if (pos >= n_words) return false;
        r = words[pos++] >> (32 - k);
    } while (r >= n);
    *out = r;
    return true;
}

}  // namespace

void annotation_dims(int32_t out[3]) { out[0] = kNearThreads; out[1] = kGeneTile; out[2] = kOverlapThreads; }

}  // namespace ms

using namespace ms;

extern "C" {

int ms_genes_create(const int64_t *chrom_offsets, int32_t n_chroms, const int64_t *tss, const int8_t *strand, ms_genes **out) {
    if (!out) { set_error("NULL out"); return MS_ERR_INVALID; }
    *out = nullptr;
    if (n_chroms < 0 || !chrom_offsets) { set_error("need chrom_offsets[n_chroms + 1]"); return MS_ERR_INVALID; }
    if (chrom_offsets[0] != 0) { set_error("chrom_offsets[0] must be 0"); return MS_ERR_INVALID; }
    for (int32_t c = 0; c < n_chroms; ++c)
        if (chrom_offsets[c + 1] < chrom_offsets[c]) { set_error("chrom_offsets must not decrease (entry %d)", c + 1); return MS_ERR_INVALID; }
    const int64_t n = chrom_offsets[n_chroms];
    if (n > 0 && (!tss || !strand)) { set_error("NULL gene arrays"); return MS_ERR_INVALID; }
    for (int64_t i = 0; i < n; ++i) {
        if (strand[i] != MS_STRAND_FWD && strand[i] != MS_STRAND_REV) { set_error("gene %lld: strand must be MS_STRAND_FWD or MS_STRAND_REV", (long long) i); return MS_ERR_INVALID; }
        if (!coord_ok(tss[i])) { set_error("gene %lld: tss %lld out of range", (long long) i, (long long) tss[i]); return MS_ERR_INVALID; }
    }
    ms_genes *g = new (std::nothrow) ms_genes();
    if (!g) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    g->n_chroms = n_chroms;
    g->off.assign(chrom_offsets, chrom_offsets + n_chroms + 1);
    g->tss.assign(tss, tss + n);
    g->strand.assign(strand, strand + n);
    *out = g;
    return MS_OK;
}

void ms_genes_free(ms_genes *g) {
    if (!g) return;
    if (g->device >= 0) {
        DeviceCtx *c;
        if (get_ctx(g->device, &c) == MS_OK) {
            dev_free(g->d_off);
            dev_free(g->d_key);
            dev_free(g->d_plo);
            dev_free(g->d_phi);
        }
    }
    delete g;
}

int ms_genes_nearest_tss(const ms_genes *genes, const int32_t *chrom, const int64_t *start, int64_t n, int64_t cutoff, int64_t *distance,
                         uint8_t *found) {
    if (!genes) { set_error("NULL genes"); return MS_ERR_INVALID; }
    if (n < 0 || (n > 0 && (!chrom || !start || !distance || !found))) { set_error("bad region arrays"); return MS_ERR_INVALID; }
    if (cutoff >= kCoordMax) { set_error("distance cutoff %lld out of range", (long long) cutoff); return MS_ERR_INVALID; }
    if (n == 0) return MS_OK;
    ms_genes *g = const_cast<ms_genes *>(genes);
    std::lock_guard<std::mutex> lk(g->mu);
    DeviceCtx *c;
    int rc = genes_upload(g, &c);
    if (rc) return rc;
    // group the regions by chromosome: a block walks ONE gene list.  Regions with no genes to walk never reach the device.
    std::vector<int64_t> first((size_t) g->n_chroms + 1, 0);
    for (int64_t r = 0; r < n; ++r) {
        if (!coord_ok(start[r])) { set_error("region %lld: start %lld out of range", (long long) r, (long long) start[r]); return MS_ERR_INVALID; }
        const int32_t ch = chrom[r];
        if (ch >= 0 && ch < g->n_chroms && g->off[ch + 1] > g->off[ch]) ++first[(size_t) ch + 1];
    }
    std::vector<NearBlock> blocks;
    for (int32_t ch = 0; ch < g->n_chroms; ++ch) {
        const int64_t cnt = first[(size_t) ch + 1];
        first[(size_t) ch + 1] += first[ch];
        for (int64_t k = 0; k < cnt; k += kNearThreads)
            blocks.push_back(NearBlock{first[ch] + k, ch, (int32_t) std::min<int64_t>(kNearThreads, cnt - k)});
    }
    const int64_t m = first[g->n_chroms];
    std::vector<int64_t> idx((size_t) m), s_grouped((size_t) m);
    {
        std::vector<int64_t> fill(first.begin(), first.end() - 1);
        for (int64_t r = 0; r < n; ++r) {
            const int32_t ch = chrom[r];
            distance[r] = 0;
            found[r] = 0;
            if (ch >= 0 && ch < g->n_chroms && g->off[ch + 1] > g->off[ch]) {
                const int64_t k = fill[ch]++;
                idx[(size_t) k] = r;
                s_grouped[(size_t) k] = start[r];
            }
        }
    }
    if (m == 0) return MS_OK;
    if (blocks.size() > (size_t) INT_MAX) { set_error("too many regions"); return MS_ERR_INVALID; }
    std::lock_guard<std::mutex> lk_dev(c->mu);
    const hipStream_t st = c->stream;
    auto up = [](size_t x) { return (x + 255) & ~(size_t) 255; };
    const size_t b_start = up(8 * (size_t) m), b_blocks = up(sizeof(NearBlock) * blocks.size()), b_dist = up(8 * (size_t) m), b_found = up((size_t) m);
    void *blk = nullptr;
    size_t got = 0;
    if ((rc = pool_alloc(c, b_start + b_blocks + b_dist + b_found, &blk, &got))) return rc;
    char *p = static_cast<char *>(blk);
    int64_t *d_start = reinterpret_cast<int64_t *>(p);
    NearBlock *d_blocks = reinterpret_cast<NearBlock *>(p + b_start);
    int64_t *d_dist = reinterpret_cast<int64_t *>(p + b_start + b_blocks);
    uint8_t *d_found = reinterpret_cast<uint8_t *>(p + b_start + b_blocks + b_dist);
    std::vector<int64_t> h_dist((size_t) m);
    std::vector<uint8_t> h_found((size_t) m);
    hipError_t he = hipMemcpyAsync(d_start, s_grouped.data(), 8 * (size_t) m, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(d_blocks, blocks.data(), sizeof(NearBlock) * blocks.size(), hipMemcpyHostToDevice, st);
    if (he == hipSuccess) {
        hipLaunchKernelGGL(nearest_tss_kernel, dim3((unsigned) blocks.size()), dim3(kNearThreads), 0, st, g->d_key, g->d_off, d_blocks, d_start,
                           cutoff, d_dist, d_found);
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpyAsync(h_dist.data(), d_dist, 8 * (size_t) m, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipMemcpyAsync(h_found.data(), d_found, (size_t) m, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    else (void) hipStreamSynchronize(st);         // whatever was queued still reads the block and writes the host buffers: let it end first
    pool_free(c, blk, got);
    if (he != hipSuccess) { set_error("nearest TSS failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    for (int64_t k = 0; k < m; ++k) {
        distance[idx[(size_t) k]] = h_dist[(size_t) k];
        found[idx[(size_t) k]] = h_found[(size_t) k];
    }
    return MS_OK;
}

int ms_genes_promoter_overlap(const ms_genes *genes, int64_t upstream, int64_t downstream, const int32_t *chrom, const int64_t *start,
                              const int64_t *end, int64_t n, uint8_t *overlap) {
    if (!genes) { set_error("NULL genes"); return MS_ERR_INVALID; }
    if (n < 0 || (n > 0 && (!chrom || !start || !end || !overlap))) { set_error("bad region arrays"); return MS_ERR_INVALID; }
    if (!coord_ok(upstream) || !coord_ok(downstream)) { set_error("promoter extent out of range"); return MS_ERR_INVALID; }
    if (n == 0) return MS_OK;
    if ((n + kOverlapThreads - 1) / kOverlapThreads > INT_MAX) { set_error("too many regions"); return MS_ERR_INVALID; }
    ms_genes *g = const_cast<ms_genes *>(genes);
    std::lock_guard<std::mutex> lk(g->mu);
    DeviceCtx *c;
    int rc = genes_upload(g, &c);
    if (rc) return rc;
    if ((rc = promoters_upload(g, upstream, downstream))) return rc;
    std::lock_guard<std::mutex> lk_dev(c->mu);
    const hipStream_t st = c->stream;
    auto up = [](size_t x) { return (x + 255) & ~(size_t) 255; };
    const size_t b8 = up(8 * (size_t) n), b4 = up(4 * (size_t) n), b1 = up((size_t) n);
    void *blk = nullptr;
    size_t got = 0;
    if ((rc = pool_alloc(c, 2 * b8 + b4 + b1, &blk, &got))) return rc;
    char *p = static_cast<char *>(blk);
    int64_t *d_start = reinterpret_cast<int64_t *>(p), *d_end = reinterpret_cast<int64_t *>(p + b8);
    int32_t *d_chrom = reinterpret_cast<int32_t *>(p + 2 * b8);
    uint8_t *d_out = reinterpret_cast<uint8_t *>(p + 2 * b8 + b4);
    hipError_t he = hipMemcpyAsync(d_start, start, 8 * (size_t) n, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(d_end, end, 8 * (size_t) n, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(d_chrom, chrom, 4 * (size_t) n, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) {
        hipLaunchKernelGGL(promoter_overlap_kernel, dim3((unsigned) ((n + kOverlapThreads - 1) / kOverlapThreads)), dim3(kOverlapThreads), 0, st,
                           g->d_plo, g->d_phi, g->d_off, g->n_chroms, d_chrom, d_start, d_end, n, d_out);
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpyAsync(overlap, d_out, (size_t) n, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    else (void) hipStreamSynchronize(st);         // as above
    pool_free(c, blk, got);
    if (he != hipSuccess) { set_error("promoter overlap failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    return MS_OK;
}

int ms_control_regions_replay_host(const uint32_t *words, int64_t n_words, int64_t n_regions, const int64_t *chrom_size, const int64_t *length,
                                   const int64_t *gene_lo, const int64_t *gene_hi, const int64_t *distance, const uint8_t *found,
                                   const int64_t *tss, const int8_t *strand, int32_t n_random, int64_t max_attempts, int64_t *start_out,
                                   int64_t *words_used, int64_t *attempts, int64_t *n_done, int32_t *stop, int64_t *stop_words) {
    if (!n_done || !stop || !stop_words || n_words < 0 || n_regions < 0 || n_random < 0 || (n_words > 0 && !words)) {
        set_error("bad arguments");
        return MS_ERR_INVALID;
    }
    const bool annotated = tss != nullptr;
    if (n_regions > 0 && (!chrom_size || !length || !words_used || (n_random > 0 && !start_out) ||
                          (annotated && (!strand || !gene_lo || !gene_hi || !distance || !found)))) {
        set_error("NULL array");
        return MS_ERR_INVALID;
    }
    if (annotated && max_attempts < 1) { set_error("max_attempts must be >= 1"); return MS_ERR_INVALID; }
    *n_done = 0;
    *stop = MS_REPLAY_DONE;
    *stop_words = 0;
    int64_t pos = 0;
    for (int64_t r = 0; r < n_regions; ++r) {
        int64_t p = pos, tried = 0;              // the region's own words: it counts only once it is complete
        int64_t *dst = n_random > 0 ? start_out + r * (int64_t) n_random : nullptr;
        if (!annotated) {
            if (n_random > 0) {
                if (chrom_size[r] == MS_REPLAY_SIZE_MISSING) { *stop = MS_REPLAY_NO_SIZE; *stop_words = p; return MS_OK; }
                const int64_t width = chrom_size[r] - length[r] + 1;        // randint(0, size - length) = _randbelow(width)
                if (width <= 0) { *stop = MS_REPLAY_EMPTY_RANGE; *stop_words = p; return MS_OK; }
                if (width >= (1LL << 32)) { *stop = MS_REPLAY_WIDE; *stop_words = p; return MS_OK; }
                for (int32_t j = 0; j < n_random; ++j, ++tried)
                    if (!randbelow(words, n_words, p, (uint32_t) width, &dst[j])) { *stop = MS_REPLAY_WORDS; *stop_words = pos; return MS_OK; }
            }
        } else if (gene_hi[r] > gene_lo[r] && n_random > 0) {
            const int64_t n_genes = gene_hi[r] - gene_lo[r];
            if (n_genes >= (1LL << 32)) { set_error("region %lld: too many genes", (long long) r); return MS_ERR_INVALID; }
            int64_t dist = distance[r];
            if (!found[r]) {                     // once per region, in front of the first choice: randint(10000, 100000)
                if (!randbelow(words, n_words, p, 90001u, &dist)) { *stop = MS_REPLAY_WORDS; *stop_words = pos; return MS_OK; }
                dist += 10000;
            }
            for (int32_t kept = 0; kept < n_random;) {
                if (tried >= max_attempts) { *stop = MS_REPLAY_ATTEMPTS; *stop_words = p; return MS_OK; }
                int64_t pick;
                if (!randbelow(words, n_words, p, (uint32_t) n_genes, &pick)) { *stop = MS_REPLAY_WORDS; *stop_words = pos; return MS_OK; }
                ++tried;
                const int64_t gi = gene_lo[r] + pick;
                const int64_t s = strand[gi] == MS_STRAND_REV ? tss[gi] - dist : tss[gi] + dist;
                if (s < 0) continue;             // the reference's `and` never looks the size up for these
                if (chrom_size[r] == MS_REPLAY_SIZE_MISSING) { *stop = MS_REPLAY_NO_SIZE; *stop_words = p; return MS_OK; }
                if (s + length[r] <= chrom_size[r]) dst[kept++] = s;
            }
        }
        pos = p;
        words_used[r] = pos;
        if (attempts) attempts[r] = tried;
        *n_done = r + 1;
        *stop_words = pos;
    }
    return MS_OK;
}

}  // extern "C"
