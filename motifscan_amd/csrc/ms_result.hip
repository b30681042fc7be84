// ms_result.hip -- the result handle: its one pooled device block, the hit accessors and their pinned host copies, region counts,
// de-duplication on the device (and its host restatement, ms_dedup_hits), the site tables.
#include <algorithm>
#include <cmath>
#include <climits>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>

#include "ms_device.h"
#include "ms_handles.h"

namespace ms {

// -------------------------------------------------------------- de-dup / site tables --

// scanner.py:156-193 on the sorted hit arrays.  The thread of the FIRST hit of a (motif, region)
// segment walks the segment once with one "current site" per strand: a later same-strand site
// closer than the motif width either loses (score <=: tie keeps the earlier one) or replaces it.
// The kept hits are already in the order the reference returns (start ascending, '+' first).
__global__ void __launch_bounds__(256) dedup_kernel(int64_t n, const int64_t *__restrict__ motif_off, int32_t P,
                                                    const int32_t *__restrict__ width, const int64_t *__restrict__ seq_idx,
                                                    const int64_t *__restrict__ pos, const double *__restrict__ score,
                                                    const int8_t *__restrict__ strand, uint32_t *__restrict__ keep) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t p = motif_of_hit(motif_off, P, i);
    const int64_t r = seq_idx[i];
    if (i > motif_off[p] && seq_idx[i - 1] == r) return;            // not the head of its segment
    const int64_t end = motif_off[p + 1];
    const int64_t W = width[p];
    int64_t cur[2] = {-1, -1};
    for (int64_t j = i; j < end && seq_idx[j] == r; j++) {
        const int s = strand[j] == 1 ? 0 : 1;
        uint32_t kj = 1;
        if (cur[s] >= 0 && pos[j] - pos[cur[s]] < W) {
            if (score[cur[s]] >= score[j]) kj = 0;                   // scanner.py:163-164
            else { keep[cur[s]] = 0; cur[s] = j; }                   // scanner.py:165-166
        } else {
            cur[s] = j;
        }
        keep[j] = kj;
    }
}

__global__ void __launch_bounds__(256) compact_hits_kernel(int64_t n, const uint32_t *__restrict__ keep,
                                                           const uint64_t *__restrict__ dst,
                                                           const int64_t *__restrict__ seq_in, const int64_t *__restrict__ pos_in,
                                                           const double *__restrict__ score_in, const int8_t *__restrict__ strand_in,
                                                           int64_t *__restrict__ seq_out, int64_t *__restrict__ pos_out,
                                                           double *__restrict__ score_out, int8_t *__restrict__ strand_out) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const uint64_t d = dst[i];
    seq_out[d] = seq_in[i]; pos_out[d] = pos_in[i]; score_out[d] = score_in[i]; strand_out[d] = strand_in[i];
}

// new per-motif offsets after compaction: off_out[p] = dst[off_in[p]] (or the kept total at the end)
__global__ void remap_offsets_kernel(const int64_t *__restrict__ off_in, int32_t P, int64_t n, const uint64_t *__restrict__ dst,
                                     const uint32_t *__restrict__ keep, int64_t *__restrict__ off_out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p > P) return;
    const int64_t o = off_in[p];
    off_out[p] = o < n ? (int64_t) dst[o] : (n > 0 ? (int64_t) dst[n - 1] + keep[n - 1] : 0);
}

// io/__init__.py:23-33: per (motif, region) the number of sites and the maximum score
__global__ void __launch_bounds__(256) site_tables_kernel(int64_t n, const int64_t *__restrict__ motif_off, int32_t P, int64_t R,
                                                          const int64_t *__restrict__ seq_idx, const double *__restrict__ score,
                                                          int32_t *__restrict__ n_sites, double *__restrict__ max_score) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t p = motif_of_hit(motif_off, P, i);
    const int64_t r = seq_idx[i];
    if (i > motif_off[p] && seq_idx[i - 1] == r) return;
    const int64_t end = motif_off[p + 1];
    int32_t cnt = 0;
    double best = score[i];
    for (int64_t j = i; j < end && seq_idx[j] == r; j++) {
        cnt++;
        if (score[j] > best) best = score[j];
    }
    n_sites[(int64_t) p * R + r] = cnt;
    max_score[(int64_t) p * R + r] = best;
}

__global__ void fill_nan_kernel(double *__restrict__ a, int64_t n) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = __longlong_as_double(0x7FF8000000000000LL);
}

static int launch_dedup(int64_t n, const int64_t *motif_off, int32_t P, const int32_t *width, const int64_t *seq_idx,
                        const int64_t *pos, const double *score, const int8_t *strand, uint32_t *keep, hipStream_t st) {
    if (n == 0) return MS_OK;
    hipLaunchKernelGGL(dedup_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, st, n, motif_off, P, width, seq_idx,
                       pos, score, strand, keep);
    MS_HIP(hipGetLastError());
    return MS_OK;
}

static int launch_compact_hits(int64_t n, const uint32_t *keep, const uint64_t *dst, const int64_t *seq_in, const int64_t *pos_in,
                               const double *score_in, const int8_t *strand_in, int64_t *seq_out, int64_t *pos_out,
                               double *score_out, int8_t *strand_out, const int64_t *off_in, int32_t P, int64_t *off_out,
                               hipStream_t st) {
    hipLaunchKernelGGL(remap_offsets_kernel, dim3((unsigned) ((P + 1 + 255) / 256)), dim3(256), 0, st, off_in, P, n, dst, keep, off_out);
    MS_HIP(hipGetLastError());
    if (n == 0) return MS_OK;
    hipLaunchKernelGGL(compact_hits_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, st, n, keep, dst, seq_in, pos_in,
                       score_in, strand_in, seq_out, pos_out, score_out, strand_out);
    MS_HIP(hipGetLastError());
    return MS_OK;
}

static int launch_site_tables(int64_t n, const int64_t *motif_off, int32_t P, int64_t R, const int64_t *seq_idx,
                              const double *score, int32_t *n_sites, double *max_score, hipStream_t st) {
    const int64_t cells = (int64_t) P * R;
    if (cells == 0) return MS_OK;
    MS_HIP(hipMemsetAsync(n_sites, 0, (size_t) cells * sizeof(int32_t), st));
    hipLaunchKernelGGL(fill_nan_kernel, dim3((unsigned) ((cells + 255) / 256)), dim3(256), 0, st, max_score, cells);
    MS_HIP(hipGetLastError());
    if (n == 0) return MS_OK;
    hipLaunchKernelGGL(site_tables_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, st, n, motif_off, P, R, seq_idx,
                       score, n_sites, max_score);
    MS_HIP(hipGetLastError());
    return MS_OK;
}

// ---------------------------------------------------------------- compact copy-out --

// coord = seq_idx << 32 | pos << 1 | (strand - 1): 8 bytes per hit on the host link instead of 17 (ms_result_hits_packed_host).
// shift > 0: the 4-byte form, coord32 = seq_idx << shift | pos << 1 | (strand - 1) (ms_result_hits_packed12_host: the caller has
// checked that every region index and position of the set fits).  bad[0] is set if a hit does not fit the format.
__global__ void __launch_bounds__(256) pack_hits_kernel(int64_t n, const unsigned long long *__restrict__ n_dev, const int64_t *__restrict__ seq_idx,
                                                        const int64_t *__restrict__ pos, const int8_t *__restrict__ strand,
                                                        uint64_t *__restrict__ coord, unsigned int *__restrict__ bad, int shift) {
    if (n_dev) { const unsigned long long nd = *n_dev; if ((unsigned long long) n > nd) n = (int64_t) nd; }     // (finalize_kernel: a predicted-size scan)
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t sq = (uint64_t) seq_idx[i], ps = (uint64_t) pos[i];
    if (shift > 0) {
        if ((ps >> (shift - 1)) != 0 || (sq >> (32 - shift)) != 0) *bad = 1u;
        reinterpret_cast<uint32_t *>(coord)[i] = (uint32_t) ((sq << shift) | (ps << 1) | (uint64_t) (strand[i] == 2 ? 1 : 0));
        return;
    }
    if ((sq >> 32) != 0 || (ps >> 31) != 0) *bad = 1u;
    coord[i] = (sq << 32) | ((ps & 0x7FFFFFFFull) << 1) | (uint64_t) (strand[i] == 2 ? 1 : 0);
}

int launch_pack_hits(int64_t n, const unsigned long long *n_dev, const int64_t *seq_idx, const int64_t *pos, const int8_t *strand, uint64_t *coord,
                     unsigned int *bad, hipStream_t st, int shift) {
    if (n == 0) return MS_OK;
    hipLaunchKernelGGL(pack_hits_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, st, n, n_dev, seq_idx, pos, strand, coord, bad, shift);
    MS_HIP(hipGetLastError());
    return MS_OK;
}

// Lay the result arrays out in one device block: [counts P+1][offsets P+1][seq_idx n][pos n][score n][strand n]
size_t result_block_bytes(int32_t P, size_t n) {
    const size_t n_round = (n + 65535) & ~(size_t) 65535;
    return 8 * (2 * ((size_t) P + 1) + 3 * n_round) + n_round + 256;
}

void result_carve(ms_result *r, void *blk, size_t n) {
    const size_t P1 = (size_t) r->P + 1, n_round = (n + 65535) & ~(size_t) 65535;
    char *b = static_cast<char *>(blk);
    r->d_region_counts = reinterpret_cast<unsigned long long *>(b);
    r->d_motif_first = reinterpret_cast<int64_t *>(b + 8 * P1);
    r->d_seq_idx = reinterpret_cast<int64_t *>(b + 16 * P1);
    r->d_pos = r->d_seq_idx + n_round;
    r->d_score = reinterpret_cast<double *>(r->d_pos + n_round);
    r->d_strand = reinterpret_cast<int8_t *>(r->d_score + n_round);
}

int result_block_alloc(DeviceCtx *c, ms_result *r, size_t n) {
    void *blk = nullptr;
    size_t got = 0;
    const int rc = pool_alloc(c, result_block_bytes(r->P, n), &blk, &got);
    if (rc) return rc;
    r->block = blk;
    r->block_bytes = got;
    result_carve(r, blk, n);
    return MS_OK;
}

// The counts onto the host on the copy-out stream (a batch stream's third stage: the consumer's ms_result_region_counts then never issues a
// blocking device copy of its own -- 14 of those per configs[3] pass, each queued behind the copy engine's hit arrays, cost the reference
// CLI's job 5-7 ms per pass in round 6's first measurements)
int result_fetch_region_counts(ms_result *r) {
    if (!r || r->P == 0) return MS_OK;
    DeviceCtx *c;
    int rc = get_ctx(r->device, &c);
    if (rc) return rc;
    if (r->h_region_counts.size() == (size_t) r->P) return MS_OK;      // (a queued scan brought them along: scan_complete)
    try { r->h_region_counts.assign((size_t) r->P, 0); } catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    const hipStream_t down = c->stream_down;
    hipError_t he = hipMemcpyAsync(r->h_region_counts.data(), r->d_region_counts, (size_t) r->P * sizeof(int64_t), hipMemcpyDeviceToHost, down);
    if (he == hipSuccess) he = hipStreamSynchronize(down);
    if (he != hipSuccess) { r->h_region_counts.clear(); set_error("copy of the region counts failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    return MS_OK;
}

}  // namespace ms

using namespace ms;

extern "C" {

int ms_result_num_hits(const ms_result *r, int64_t *n_hits) {
    if (!r || !n_hits) { set_error("NULL argument"); return MS_ERR_INVALID; }
    *n_hits = r->n_hits;
    return MS_OK;
}

int ms_result_motif_offsets(const ms_result *r, int64_t *out) {
    if (!r || !out) { set_error("NULL argument"); return MS_ERR_INVALID; }
    std::memcpy(out, r->motif_offsets.data(), r->motif_offsets.size() * sizeof(int64_t));
    return MS_OK;
}

int ms_result_hits(const ms_result *r, int64_t *seq_idx, int64_t *pos, double *score, int8_t *strand) {
    if (!r) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (r->counts_only) { set_error("a counts-only result (MS_SCAN_COUNTS_ONLY, a counts-only batch or sweep span of a stream) holds the per-motif region counts and site numbers, no site arrays"); return MS_ERR_INVALID; }
    if (r->n_hits == 0) return MS_OK;
    MS_HIP(hipSetDevice(r->device));
    const size_t n = (size_t) r->n_hits;
    if (seq_idx) MS_HIP(hipMemcpy(seq_idx, r->d_seq_idx, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (pos) MS_HIP(hipMemcpy(pos, r->d_pos, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (score) MS_HIP(hipMemcpy(score, r->d_score, n * sizeof(double), hipMemcpyDeviceToHost));
    if (strand) MS_HIP(hipMemcpy(strand, r->d_strand, n * sizeof(int8_t), hipMemcpyDeviceToHost));
    return MS_OK;
}

// Hit arrays in library-owned PINNED host memory (one D2H copy at PCIe rate instead of four copies
// into pageable buffers).  The result has ONE pinned buffer, shared with the two compact accessors below and holding one form at a
// time: the pointers stay valid until the result is freed or de-duplicated or another form is asked for (a refused request included).
// The copy runs on the device's copy-out stream, beside whatever scan is running.
int ms_result_hits_host(ms_result *r, const int64_t **seq_idx, const int64_t **pos, const double **score,
                        const int8_t **strand) {
    if (!r) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (r->counts_only) { set_error("a counts-only result (MS_SCAN_COUNTS_ONLY, a counts-only batch or sweep span of a stream) holds the per-motif region counts and site numbers, no site arrays"); return MS_ERR_INVALID; }
    const size_t n = (size_t) r->n_hits;
    const size_t n_round = (n + 65535) & ~(size_t) 65535;
    const size_t bytes = 25 * n_round + 64;
    if (r->h_pinned_hits != r->n_hits || !r->h_pinned || r->h_packed) {
        r->h_pinned_hits = -1;                            // refilled from here on: whatever the buffer held is void, the flags are set on success
        if (r->h_pinned && r->h_pinned_bytes < bytes) { pinned_free(r->h_pinned, r->h_pinned_bytes); r->h_pinned = nullptr; }
        if (!r->h_pinned) {
            r->h_pinned = pinned_alloc(bytes, &r->h_pinned_bytes);
            if (!r->h_pinned) { set_error("pinned host allocation of %zu bytes failed", bytes); return MS_ERR_NOMEM; }
        }
        if (n > 0) {
            DeviceCtx *c;
            int rc = get_ctx(r->device, &c);
            if (rc) return rc;
            // the device block may have been carved for more hits than there are (a predicted-size scan sizes it by a bound):
            // four copies, packed n_round elements apart on the host
            char *hb = static_cast<char *>(r->h_pinned);
            const hipStream_t down = c->stream_down;
            MS_HIP(hipMemcpyAsync(hb, r->d_seq_idx, 8 * n, hipMemcpyDeviceToHost, down));
            MS_HIP(hipMemcpyAsync(hb + 8 * n_round, r->d_pos, 8 * n, hipMemcpyDeviceToHost, down));
            MS_HIP(hipMemcpyAsync(hb + 16 * n_round, r->d_score, 8 * n, hipMemcpyDeviceToHost, down));
            MS_HIP(hipMemcpyAsync(hb + 24 * n_round, r->d_strand, n, hipMemcpyDeviceToHost, down));
            MS_HIP(hipStreamSynchronize(down));
        }
        r->h_pinned_hits = r->n_hits;
        r->h_packed = false;
    }
    char *b = static_cast<char *>(r->h_pinned);
    if (seq_idx) *seq_idx = reinterpret_cast<const int64_t *>(b);
    if (pos) *pos = reinterpret_cast<const int64_t *>(b + 8 * n_round);
    if (score) *score = reinterpret_cast<const double *>(b + 16 * n_round);
    if (strand) *strand = reinterpret_cast<const int8_t *>(b + 24 * n_round);
    return MS_OK;
}

// The same in 16 bytes per hit: coord = seq_idx << 32 | pos << 1 | (strand - 1), score.  The device packs the three
// coordinate arrays into one word per hit first, so only 16 of the 25 bytes cross the host link.
int ms_result_hits_packed_host(ms_result *r, const uint64_t **coord, const double **score) {
    if (!r) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (r->counts_only) { set_error("a counts-only result (MS_SCAN_COUNTS_ONLY, a counts-only batch or sweep span of a stream) holds the per-motif region counts and site numbers, no site arrays"); return MS_ERR_INVALID; }
    if (r->d_coord && r->coord_shift) { set_error("this result holds the 12-byte compact form (MS_STREAM_PACKED12): read it with ms_result_hits_packed12_host"); return MS_ERR_INVALID; }
    const size_t n = (size_t) r->n_hits;
    const size_t n_round = (n + 65535) & ~(size_t) 65535;
    const size_t bytes = 16 * n_round + 64;
    if (r->h_pinned_hits != r->n_hits || !r->h_pinned || !r->h_packed || r->h_coord_shift) {
        r->h_pinned_hits = -1;                            // refilled from here on: whatever the buffer held is void, the flags are set on success
        if (r->h_pinned && r->h_pinned_bytes < bytes) { pinned_free(r->h_pinned, r->h_pinned_bytes); r->h_pinned = nullptr; }
        if (!r->h_pinned) {
            r->h_pinned = pinned_alloc(bytes, &r->h_pinned_bytes);
            if (!r->h_pinned) { set_error("pinned host allocation of %zu bytes failed", bytes); return MS_ERR_NOMEM; }
        }
        if (n > 0 && r->d_coord) {                      // the scan made the coordinate words already: copies only
            DeviceCtx *c;
            int rc = get_ctx(r->device, &c);
            if (rc) return rc;
            unsigned int bad = 0;
            const hipStream_t down = c->stream_down;
            char *hb = static_cast<char *>(r->h_pinned);
            hipError_t he = hipMemcpyAsync(hb, r->d_coord, 8 * n, hipMemcpyDeviceToHost, down);
            if (he == hipSuccess) he = hipMemcpyAsync(hb + 8 * n_round, r->d_score, 8 * n, hipMemcpyDeviceToHost, down);
            if (he == hipSuccess) he = hipMemcpyAsync(&bad, r->d_coord_bad, sizeof(unsigned int), hipMemcpyDeviceToHost, down);
            const hipError_t hs = hipStreamSynchronize(down);
            if (he != hipSuccess || hs != hipSuccess) { set_error("compact copy-out failed: %s", hipGetErrorString(he != hipSuccess ? he : hs)); return MS_ERR_RUNTIME; }
            if (bad) { set_error("a hit does not fit the compact form (needs seq_idx < 2^32 and pos < 2^31): use ms_result_hits_host"); return MS_ERR_INVALID; }
        } else if (n > 0) {
            DeviceCtx *c;
            int rc = get_ctx(r->device, &c);
            if (rc) return rc;
            void *blk = nullptr;
            size_t got = 0;
            if ((rc = pool_alloc(c, 8 * n_round + 256, &blk, &got))) return rc;
            uint64_t *d_coord = static_cast<uint64_t *>(blk);
            unsigned int *d_bad = reinterpret_cast<unsigned int *>(d_coord + n_round);
            unsigned int bad = 0;
            const hipStream_t down = c->stream_down;
            hipError_t he = hipMemsetAsync(d_bad, 0, sizeof(unsigned int), down);
            if (he == hipSuccess) rc = launch_pack_hits((int64_t) n, nullptr, r->d_seq_idx, r->d_pos, r->d_strand, d_coord, d_bad, down);
            char *hb = static_cast<char *>(r->h_pinned);
            if (he == hipSuccess && !rc) he = hipMemcpyAsync(hb, d_coord, 8 * n, hipMemcpyDeviceToHost, down);
            if (he == hipSuccess && !rc) he = hipMemcpyAsync(hb + 8 * n_round, r->d_score, 8 * n, hipMemcpyDeviceToHost, down);
            if (he == hipSuccess && !rc) he = hipMemcpyAsync(&bad, d_bad, sizeof(unsigned int), hipMemcpyDeviceToHost, down);
            const hipError_t hs = hipStreamSynchronize(down);
            pool_free(c, blk, got);
            if (rc) return rc;
            if (he != hipSuccess || hs != hipSuccess) { set_error("compact copy-out failed: %s", hipGetErrorString(he != hipSuccess ? he : hs)); return MS_ERR_RUNTIME; }
            if (bad) { set_error("a hit does not fit the compact form (needs seq_idx < 2^32 and pos < 2^31): use ms_result_hits_host"); return MS_ERR_INVALID; }
        }
        r->h_pinned_hits = r->n_hits;
        r->h_packed = true;
        r->h_coord_shift = 0;
    }
    char *b = static_cast<char *>(r->h_pinned);
    if (coord) *coord = reinterpret_cast<const uint64_t *>(b);
    if (score) *score = reinterpret_cast<const double *>(b + 8 * n_round);
    return MS_OK;
}

// The 12-byte form: coord32[i] = seq_idx << shift | pos << 1 | (strand - 1) and score[i].  A batch stream made with MS_STREAM_PACKED12 has
// produced the words during the scan when the batch fits (copies only here); a result that holds none is packed now if it fits.
int ms_result_hits_packed12_host(ms_result *r, const uint32_t **coord, const double **score, int32_t *shift_out) {
    if (!r) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (r->counts_only) { set_error("a counts-only result (MS_SCAN_COUNTS_ONLY, a counts-only batch or sweep span of a stream) holds the per-motif region counts and site numbers, no site arrays"); return MS_ERR_INVALID; }
    if (r->d_coord && !r->coord_shift) { set_error("this result holds the 16-byte compact form (its batch did not fit 31 bits of region index and position): read it with ms_result_hits_packed_host"); return MS_ERR_INVALID; }
    const size_t n = (size_t) r->n_hits;
    const size_t n_round = (n + 65535) & ~(size_t) 65535;
    const size_t bytes = 12 * n_round + 64;
    if (r->h_pinned_hits != r->n_hits || !r->h_pinned || !r->h_packed || !r->h_coord_shift) {
        r->h_pinned_hits = -1;                            // refilled from here on: whatever the buffer held is void, the flags are set on success
        if (r->h_pinned && r->h_pinned_bytes < bytes) { pinned_free(r->h_pinned, r->h_pinned_bytes); r->h_pinned = nullptr; }
        if (!r->h_pinned) {
            r->h_pinned = pinned_alloc(bytes, &r->h_pinned_bytes);
            if (!r->h_pinned) { set_error("pinned host allocation of %zu bytes failed", bytes); return MS_ERR_NOMEM; }
        }
        int shift = r->coord_shift;
        DeviceCtx *c = nullptr;
        int rc = n > 0 ? get_ctx(r->device, &c) : MS_OK;
        if (rc) return rc;
        void *blk = nullptr;
        size_t got = 0;
        const uint64_t *d_words = r->d_coord;
        const unsigned int *d_bad = r->d_coord_bad;
        if (n > 0 && !r->d_coord) {                     // no words yet: the shift from the hits themselves (largest region index / position)
            const hipStream_t down = c->stream_down;
            int64_t last_seq = 0;
            // the hits of a motif are ordered by region: the largest region index is the maximum over the motifs' last hits -- P small
            // copies would do; R is known to the result, so the bound is R - 1 whatever the hits are
            last_seq = std::max<int64_t>(r->R - 1, 0);
            int rb = 1;
            while ((1LL << rb) <= last_seq) rb++;
            if (rb >= 31) { set_error("the result's region indices need %d bits: the 12-byte compact form does not fit (use ms_result_hits_packed_host)", rb); return MS_ERR_INVALID; }
            shift = 32 - rb;                            // positions get every remaining bit; the kernel flags a position that does not fit
            if ((rc = pool_alloc(c, 4 * n_round + 256, &blk, &got))) return rc;
            unsigned int *bad_w = reinterpret_cast<unsigned int *>(static_cast<char *>(blk) + 4 * n_round);
            hipError_t he = hipMemsetAsync(bad_w, 0, sizeof(unsigned int), down);
            if (he == hipSuccess) rc = launch_pack_hits((int64_t) n, nullptr, r->d_seq_idx, r->d_pos, r->d_strand, static_cast<uint64_t *>(blk), bad_w, down, shift);
            if (he != hipSuccess || rc) { pool_free(c, blk, got); if (!rc) { set_error("memset failed: %s", hipGetErrorString(he)); rc = MS_ERR_RUNTIME; } return rc; }
            d_words = static_cast<const uint64_t *>(blk);
            d_bad = bad_w;
        }
        if (n > 0) {
            unsigned int bad = 0;
            const hipStream_t down = c->stream_down;
            char *hb = static_cast<char *>(r->h_pinned);
            hipError_t he = hipMemcpyAsync(hb, d_words, 4 * n, hipMemcpyDeviceToHost, down);
            if (he == hipSuccess) he = hipMemcpyAsync(hb + 4 * n_round, r->d_score, 8 * n, hipMemcpyDeviceToHost, down);
            if (he == hipSuccess) he = hipMemcpyAsync(&bad, d_bad, sizeof(unsigned int), hipMemcpyDeviceToHost, down);
            const hipError_t hs = hipStreamSynchronize(down);
            if (blk) pool_free(c, blk, got);
            if (he != hipSuccess || hs != hipSuccess) { set_error("compact copy-out failed: %s", hipGetErrorString(he != hipSuccess ? he : hs)); return MS_ERR_RUNTIME; }
            if (bad) { set_error("a hit does not fit the 12-byte compact form (region index and position beside the strand bit need more than 32 bits): use ms_result_hits_packed_host"); return MS_ERR_INVALID; }
        }
        if (n == 0 && shift == 0) shift = 1;
        r->h_pinned_hits = r->n_hits;
        r->h_packed = true;
        r->h_coord_shift = shift;
    }
    char *b = static_cast<char *>(r->h_pinned);
    if (coord) *coord = reinterpret_cast<const uint32_t *>(b);
    if (score) *score = reinterpret_cast<const double *>(b + 4 * n_round);
    if (shift_out) *shift_out = r->h_coord_shift;
    return MS_OK;
}

// which compact form a batch stream left in a result: 16 (coord64 | score), 12 (coord32 | score), 0 (none: the plain arrays)
int ms_result_packed_form(const ms_result *r, int32_t *bytes_per_hit) {
    if (!r || !bytes_per_hit) { set_error("NULL argument"); return MS_ERR_INVALID; }
    *bytes_per_hit = r->h_packed && r->h_pinned_hits == r->n_hits ? (r->h_coord_shift ? 12 : 16) : (r->d_coord ? (r->coord_shift ? 12 : 16) : 0);
    return MS_OK;
}

int ms_result_region_counts(const ms_result *r, int64_t *out) {
    if (!r || (!out && r->P > 0)) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (r->P == 0) return MS_OK;
    if (r->h_region_counts.size() == (size_t) r->P) { std::memcpy(out, r->h_region_counts.data(), (size_t) r->P * sizeof(int64_t)); return MS_OK; }
    MS_HIP(hipSetDevice(r->device));
    MS_HIP(hipMemcpy(out, r->d_region_counts, (size_t) r->P * sizeof(int64_t), hipMemcpyDeviceToHost));
    return MS_OK;
}

int ms_result_region_counts_device(const ms_result *r, void **d_counts) {
    if (!r || !d_counts) { set_error("NULL argument"); return MS_ERR_INVALID; }
    *d_counts = r->d_region_counts;
    return MS_OK;
}

int ms_result_stats(const ms_result *r, ms_scan_stats *out) {
    if (!r || !out) { set_error("NULL argument"); return MS_ERR_INVALID; }
    *out = r->stats;
    return MS_OK;
}

// scanner.py:156-193 on the device, in place: afterwards the result holds only the kept sites (same
// order), with new per-motif offsets.  The per-motif region counts do not change (a region never
// loses its last site).
int ms_result_dedup(ms_result *r, const ms_pwmset *pwms_c) {
    if (!r || !pwms_c) { set_error("NULL handle"); return MS_ERR_INVALID; }
    ms_pwmset *pwms = const_cast<ms_pwmset *>(pwms_c);
    if (pwms->P != r->P) { set_error("result and PWM set disagree on the number of PWMs"); return MS_ERR_INVALID; }
    if (r->counts_only) { set_error("a counts-only result (MS_SCAN_COUNTS_ONLY, a counts-only batch or sweep span of a stream) holds the per-motif region counts and site numbers, no site arrays"); return MS_ERR_INVALID; }
    if (r->deduped || r->n_hits == 0) { r->deduped = true; return MS_OK; }
    if (r->coord_blk) {                                  // coordinate words of the hits before de-duplication: void
        DeviceCtx *c0;
        if (get_ctx(r->device, &c0) == MS_OK) pool_free(c0, r->coord_blk, r->coord_bytes); else (void) hipFree(r->coord_blk);
        r->coord_blk = nullptr; r->d_coord = nullptr; r->d_coord_bad = nullptr; r->coord_shift = 0;
    }
    DeviceCtx *c;
    int rc = get_ctx(r->device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk_dev(c->mu);
    std::lock_guard<std::mutex> lk_pwm(pwms->mu);
    if ((rc = pwmset_upload(pwms, c->device, c->stream))) return rc;
    const size_t n = (size_t) r->n_hits;
    // keep flags, destinations and the prefix sum's work space in ONE pooled block: hipMalloc / hipFree stall every stage of a
    // batch stream (hipFree waits for the whole device), and this runs per batch under MS_STREAM_DEDUP
    void *wblk = nullptr, *blk = nullptr;
    size_t tmp_bytes = 0, got = 0, wgot = 0;
    auto cleanup = [&]() { if (wblk) pool_free(c, wblk, wgot); wblk = nullptr; };
    const size_t n8 = (n + 31) & ~(size_t) 31;
    if ((rc = exclusive_sum_u32(nullptr, &tmp_bytes, nullptr, nullptr, n, c->stream))) return rc;
    if ((rc = pool_alloc(c, 12 * n8 + tmp_bytes + 256, &wblk, &wgot))) return rc;
    uint64_t *d_dst = static_cast<uint64_t *>(wblk);
    uint32_t *d_keep = reinterpret_cast<uint32_t *>(d_dst + n8);
    void *d_tmp = d_keep + n8;
    rc = launch_dedup((int64_t) n, r->d_motif_first, r->P, pwms->d_width, r->d_seq_idx, r->d_pos, r->d_score, r->d_strand,
                      d_keep, c->stream);
    if (!rc) rc = exclusive_sum_u32(d_tmp, &tmp_bytes, d_keep, d_dst, n, c->stream);
    uint64_t last_dst = 0;
    uint32_t last_keep = 0;
    if (!rc) {
        hipError_t he = hipMemcpyAsync(&last_dst, d_dst + (n - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream);
        if (he == hipSuccess) he = hipMemcpyAsync(&last_keep, d_keep + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
        if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
        if (he != hipSuccess) { set_error("de-dup kernels failed: %s", hipGetErrorString(he)); rc = MS_ERR_RUNTIME; }
    }
    if (rc) { cleanup(); return rc; }
    const size_t n_kept = (size_t) last_dst + last_keep;
    if ((rc = pool_alloc(c, result_block_bytes(r->P, n_kept), &blk, &got))) { cleanup(); return rc; }
    ms_result nr;                                   // carve the new block with the same layout
    nr.P = r->P;
    result_carve(&nr, blk, n_kept);
    const size_t P1 = (size_t) r->P + 1;
    hipError_t he = hipMemcpyAsync(nr.d_region_counts, r->d_region_counts, 8 * P1, hipMemcpyDeviceToDevice, c->stream);
    rc = launch_compact_hits((int64_t) n, d_keep, d_dst, r->d_seq_idx, r->d_pos, r->d_score, r->d_strand, nr.d_seq_idx,
                             nr.d_pos, nr.d_score, nr.d_strand, r->d_motif_first, r->P, nr.d_motif_first, c->stream);
    std::vector<int64_t> off(P1);
    if (!rc && he == hipSuccess) he = hipMemcpyAsync(off.data(), nr.d_motif_first, 8 * P1, hipMemcpyDeviceToHost, c->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
    cleanup();
    if (rc || he != hipSuccess) {
        pool_free(c, blk, got);
        if (!rc) { set_error("compaction failed: %s", hipGetErrorString(he)); rc = MS_ERR_RUNTIME; }
        return rc;
    }
    pool_free(c, r->block, r->block_bytes);
    r->block = blk; r->block_bytes = got;
    result_carve(r, blk, n_kept);
    r->n_hits = (int64_t) n_kept;
    r->motif_offsets = off;
    r->deduped = true;
    r->h_pinned_hits = -1;                            // host copy (if any) is stale
    return MS_OK;
}

// io/__init__.py:23-33: what the site tables need per (motif, region): number of sites, max score
// (NaN where the writer prints 'NA').  Host buffers [P][R].
int ms_result_site_tables(const ms_result *r, int32_t *n_sites, double *max_score) {
    if (!r) { set_error("NULL handle"); return MS_ERR_INVALID; }
    const size_t cells = (size_t) r->P * (size_t) r->R;
    if (cells == 0) return MS_OK;
    if (r->counts_only) { set_error("a counts-only result (MS_SCAN_COUNTS_ONLY, a counts-only batch or sweep span of a stream) holds the per-motif region counts and site numbers, no site arrays"); return MS_ERR_INVALID; }
    if (!n_sites || !max_score) { set_error("NULL output"); return MS_ERR_INVALID; }
    DeviceCtx *c;
    int rc = get_ctx(r->device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk_dev(c->mu);
    int32_t *d_n = nullptr;
    double *d_m = nullptr;
    if ((rc = dev_alloc(&d_n, cells)) || (rc = dev_alloc(&d_m, cells))) { dev_free(d_n); dev_free(d_m); return rc; }
    rc = launch_site_tables(r->n_hits, r->d_motif_first, r->P, r->R, r->d_seq_idx, r->d_score, d_n, d_m, c->stream);
    hipError_t he = hipSuccess;
    if (!rc) he = hipMemcpyAsync(n_sites, d_n, cells * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
    if (!rc && he == hipSuccess) he = hipMemcpyAsync(max_score, d_m, cells * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
    dev_free(d_n); dev_free(d_m);
    if (rc) return rc;
    if (he != hipSuccess) { set_error("site table kernels failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    return MS_OK;
}

void ms_result_free(ms_result *r) {
    if (!r) return;
    (void) hipSetDevice(r->device);
    if (r->h_pinned) pinned_free(r->h_pinned, r->h_pinned_bytes);
    DeviceCtx *c = nullptr;
    const bool have = (r->block || r->coord_blk) && get_ctx(r->device, &c) == MS_OK;
    if (r->block) { if (have) pool_free(c, r->block, r->block_bytes); else (void) hipFree(r->block); }
    if (r->coord_blk) { if (have) pool_free(c, r->coord_blk, r->coord_bytes); else (void) hipFree(r->coord_blk); }
    delete r;
}

// --------------------------------------------------------------------------- dedup --

// scanner.py:156-193 on the flat hit arrays.  Within one (motif, region) the reference splits
// the sites by strand, runs the greedy pass on each strand, and re-merges by a stable sort on
// start with '+' first -- which is the order the hits already have, so de-dup is a filter.
int ms_dedup_hits(const int64_t *motif_offsets, int32_t n_pwms, const int32_t *widths, const int64_t *seq_idx,
                  const int64_t *pos, const double *score, const int8_t *strand, uint8_t *keep) {
    if (n_pwms < 0 || !motif_offsets) { set_error("bad arguments"); return MS_ERR_INVALID; }
    const int64_t n = motif_offsets[n_pwms];
    if (n > 0 && (!widths || !seq_idx || !pos || !score || !strand || !keep)) { set_error("NULL array"); return MS_ERR_INVALID; }
    for (int64_t i = 0; i < n; i++) keep[i] = 1;
    for (int32_t p = 0; p < n_pwms; p++) {
        const int64_t W = widths[p];
        int64_t a = motif_offsets[p];
        const int64_t end = motif_offsets[p + 1];
        while (a < end) {
            int64_t b = a;
            while (b < end && seq_idx[b] == seq_idx[a]) b++;
            for (int8_t sd = 1; sd <= 2; sd++) {
                int64_t cur = -1;                        // index of the site currently kept (scanner.py:160)
                for (int64_t i = a; i < b; i++) {
                    if (strand[i] != sd) continue;
                    if (cur < 0) { cur = i; continue; }
                    if (pos[i] - pos[cur] < W) {
                        if (score[cur] >= score[i]) keep[i] = 0;           // tie keeps the earlier site
                        else { keep[cur] = 0; cur = i; }
                    } else {
                        cur = i;
                    }
                }
            }
            a = b;
        }
    }
    return MS_OK;
}

}  // extern "C"
