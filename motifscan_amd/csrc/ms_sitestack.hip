// ms_sitestack.hip -- what the sites of a result LOOK like: for every motif, how often A, C, G and T stand under each motif column (and
// under `flank` columns either side) over the motif's sites, in the motif's orientation, and the dinucleotide counts of adjacent
// columns (ms_result_site_base_counts).  No reference counterpart: the reference hands its hit lists to the caller, who slices the
// sequences in Python.  Here the hit arrays and the packed sequence are both resident, and the answer is a few KB of integers per
// motif: an exact integer reduction, additive over shards of the regions.
//
//   sitestack_kernel     grid y = motif row, x = blocks over chunks of kStackChunk hits of the motif's slice (a block takes every
//                        gridDim.x-th chunk).  A lane owns one hit at a time: region, position, strand, the region's two offsets; then
//                        the W + 2 * flank columns in steps of 32 -- one code_window + one n_window per step, brought into the motif's
//                        orientation in registers ('-': reversed within the step and complemented).  A window is fetched only when one
//                        of its bases lies INSIDE the region, so no address is formed below word 0 of a plane (the first region's left
//                        flank: the fetch starts at base 0 and is shifted) and none past the last base's words + 2 (the pad holds
//                        kPadWords); which columns are outside is decided by the region's bounds alone.
//                        Counting is per WAVE: a column's slot is the same in most lanes (the consensus base), so one ballot +
//                        popcount per (column, slot) replaces 64 adds to one counter; lane s keeps slot s's count and lanes 16 .. 31 the
//                        16 dinucleotide counts of (previous column, this column), and ONE add instruction per column puts them into
//                        the block's 32-bit LDS counters (or, for C above kStackLdsC, into global memory with 64-bit atomics).  The
//                        LDS counters are flushed once per block with 64-bit global adds: integer addition commutes, the bytes are the
//                        same on every run.  A site outside its region (a result of caller-supplied arrays, or the wrong sequence set)
//                        is not counted and raises a flag; the call then fails.
//                        Dinucleotides by ballot as well (16 v_cmp + s_bcnt1 per column and wave, against one LDS atomic per LANE
//                        into per-wave histograms that would need four times the LDS): chosen on the instruction count of the ISA,
//                        the two have not been timed against each other.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "ms_device.h"
#include "ms_handles.h"

namespace ms {
namespace {

constexpr int kStackThreads = 256;
constexpr int kStackChunk = 1024;                  // hits per chunk (4 per lane)
constexpr int kStackMaxBlocksX = 1024;
constexpr int kStackGridY = 32768;                 // motif rows per launch
constexpr int kStackColCells = 6 + 16;             // counters per column: 6 slots + 16 dinucleotides
constexpr int kStackLdsC = 65536 / (4 * kStackColCells);   // 744 columns: 65 472 B, inside the 64 KB a launch gets without asking
constexpr int64_t kStackMaxChunksPerBlock = 1LL << 21;     // x kStackChunk hits = 2^31: a block's 32-bit counters cannot overflow

static_assert(kPadWords >= 2, "a window that starts at the set's last base reads two code words and one mask word past it");
static_assert(kStackThreads % 64 == 0 && kStackChunk % kStackThreads == 0, "whole waves, whole trips");

struct StackArgs {
    const int64_t *motif_first, *seq_idx, *pos;
    const int8_t *strand;
    const uint32_t *codes, *nmask;
    const int64_t *offsets;
    int64_t R;
    const int32_t *width;                          // [rows]
    int32_t m0, row0, flank, C;
    unsigned long long *counts, *dinuc;            // [rows][C][6], [rows][C][16] (kDinuc), zeroed by the caller
    unsigned int *bad;                             // set when a site does not lie inside its region
};

// Dynamic LDS (kLds): 24 * C bytes of slot counters, then 64 * C bytes of dinucleotide counters when kDinuc.
template <bool kLds, bool kDinuc>
__global__ __launch_bounds__(kStackThreads) void sitestack_kernel(StackArgs A) {
    extern __shared__ unsigned int h[];
    const int row = A.row0 + (int) blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int64_t a0 = A.motif_first[A.m0 + row], a1 = A.motif_first[A.m0 + row + 1];
    const int64_t n_chunks = (a1 - a0 + kStackChunk - 1) / kStackChunk;
    if ((int64_t) blockIdx.x >= n_chunks) return;                             // uniform over the block
    const int C = A.C, flank = A.flank, W = A.width[row], ncol = W + 2 * flank;
    const int n_cnt = 6 * C, n_cells = n_cnt + (kDinuc ? 16 * C : 0);
    unsigned long long *out_c = A.counts + (size_t) row * (size_t) n_cnt;
    unsigned long long *out_d = kDinuc ? A.dinuc + (size_t) row * 16 * (size_t) C : nullptr;
    if (kLds) {
        for (int i = tid; i < n_cells; i += kStackThreads) h[i] = 0;
        __syncthreads();
    }
    for (int64_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        const int64_t c0 = a0 + ch * kStackChunk, c1 = std::min<int64_t>(c0 + kStackChunk, a1);
        for (int64_t k0 = c0; k0 < c1; k0 += kStackThreads) {
            const int64_t k = k0 + tid;
            bool act = k < c1, minus = false;
            int64_t off = 0, L = 0, p = 0;
            if (act) {
                const int64_t r = A.seq_idx[k];
                p = A.pos[k];
                minus = A.strand[k] == 2;
                if (r < 0 || r >= A.R) act = false;
                else {
                    off = A.offsets[r];
                    L = A.offsets[r + 1] - off;
                    if (p < 0 || p > L - W) act = false;
                }
                if (!act) *A.bad = 1u;
            }
            if (__ballot(act) == 0) continue;                                 // uniform over the wave; no barrier below
            int prev = 7;                                                     // the slot of the column before
            for (int j0 = 0; j0 < ncol; j0 += 32) {
                const int n = std::min(32, ncol - j0);
                // the n bases of this step start at q0, relative to the region: columns j0 .. j0 + n - 1 on '+', the same columns from
                // the other end on '-'
                const int64_t q0 = minus ? p + W - 1 + flank - j0 - (n - 1) : p - flank + j0;
                uint64_t cw = 0;
                uint32_t nw = 0, ow = low_mask(n);                            // ow: bit set = outside the region
                const int64_t lo = std::max<int64_t>(q0, 0), hi = std::min<int64_t>(q0 + n, L);      // the bases inside: [lo, hi)
                if (act && lo < hi) {
                    const int64_t g = off + q0;
                    const int sh = g < 0 ? (int) -g : 0;                      // < 32: base lo >= 0 of the region is in the window
                    cw = code_window(A.codes, g + sh) << (2 * sh);
                    const uint32_t in = low_mask((int) (hi - q0)) & ~low_mask((int) (lo - q0));
                    nw = (n_window(A.nmask, g + sh) << sh) & in;
                    ow &= ~in;
                    if (minus) {
                        uint64_t y = __brevll(cw);                            // base i -> 31 - i, the two bits of a code swapped
                        y = ((y >> 1) & 0x5555555555555555ull) | ((y & 0x5555555555555555ull) << 1);
                        cw = ~(y >> (2 * (32 - n)));                          // ... -> n - 1 - i; complement: 3 - b
                        nw = __brev(nw) >> (32 - n);
                        ow = __brev(ow) >> (32 - n);
                    }
                }
                for (int i = 0; i < n; ++i) {
                    const int slot = !act ? 7 : (ow & 1u) ? 5 : (nw & 1u) ? 4 : (int) (cw & 3u);
                    cw >>= 2;
                    nw >>= 1;
                    ow >>= 1;
                    unsigned int mine = 0;
                    int cell = (j0 + i) * 6 + lane;                           // lanes 0 .. 5
#pragma unroll
                    for (int s = 0; s < 6; ++s) {
                        const unsigned int cnt = (unsigned int) __popcll(__ballot(slot == s));
                        if (lane == s) mine = cnt;
                    }
                    if (kDinuc) {
                        const int pair = (prev < 4 && slot < 4) ? 4 * prev + slot : 16;      // column 0: prev = 7, nothing counted
#pragma unroll
                        for (int s = 0; s < 16; ++s) {
                            const unsigned int cnt = (unsigned int) __popcll(__ballot(pair == s));
                            if (lane == 16 + s) mine = cnt;
                        }
                        if (lane >= 16) cell = n_cnt + (j0 + i - 1) * 16 + (lane - 16);
                        prev = slot;
                    }
                    if (mine) {                                               // lanes 0 .. 5 and 16 .. 31 only: cell < n_cells
                        if (kLds) atomicAdd(&h[cell], mine);
                        else if (cell < n_cnt) atomicAdd(&out_c[cell], (unsigned long long) mine);
                        else atomicAdd(&out_d[cell - n_cnt], (unsigned long long) mine);
                    }
                }
            }
        }
    }
    if (!kLds) return;
    __syncthreads();
    for (int i = tid; i < n_cnt; i += kStackThreads)
        if (h[i]) atomicAdd(&out_c[i], (unsigned long long) h[i]);
    if (kDinuc)
        for (int i = tid; i < 16 * C; i += kStackThreads)
            if (h[n_cnt + i]) atomicAdd(&out_d[i], (unsigned long long) h[n_cnt + i]);
}

}  // namespace

// 1: device memory of `device`; 0: host memory; -1: device memory of another device (*other).  Shared with ms_sitesignal.hip (ms_handles.h).
int pointer_place(const void *p, int device, int *other) {
    hipPointerAttribute_t attr;
    std::memset(&attr, 0, sizeof(attr));
    const bool on_device = hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeDevice;
    (void) hipGetLastError();                          // a pageable host pointer is "not found" here, which is no error
    if (!on_device) return 0;
    *other = attr.device;
    return attr.device == device ? 1 : -1;
}

}  // namespace ms

using namespace ms;

extern "C" {

int ms_debug_sitestack_dims(int32_t out[4]) {
    if (!out) { set_error("NULL output"); return MS_ERR_INVALID; }
    out[0] = kStackThreads;
    out[1] = kStackChunk;
    out[2] = kStackLdsC;
    out[3] = kStackLdsC;                               // one limit, asked for or not
    return MS_OK;
}

int ms_result_site_base_counts(const ms_result *r, const ms_pwmset *pwms, const ms_seqset *seqs, int32_t flank, int32_t m0, int32_t m1, uint32_t flags,
                               int64_t *counts, int64_t *dinuc, int64_t *n_sites, double *device_ms) {
    if (!require_device()) return MS_ERR_RUNTIME;
    if (device_ms) *device_ms = 0.0;
    if (!r || !pwms || !seqs) { set_error("NULL handle"); return MS_ERR_INVALID; }
    if (flags != 0) { set_error("unknown site-stack flags 0x%x", flags); return MS_ERR_INVALID; }
    if (flank < 0 || flank > MS_SITESTACK_MAX_FLANK) { set_error("flank must be in [0, %d]", MS_SITESTACK_MAX_FLANK); return MS_ERR_INVALID; }
    if (r->counts_only) { set_error("a counts-only result (MS_SCAN_COUNTS_ONLY, a counts-only batch or sweep span of a stream) holds the per-motif region counts and site numbers, no site arrays"); return MS_ERR_INVALID; }
    if (pwms->P != r->P) { set_error("result and PWM set disagree on the number of PWMs"); return MS_ERR_INVALID; }
    if (m0 < 0 || m1 < m0 || m1 > r->P) { set_error("motif range [%d, %d) outside [0, %d)", m0, m1, r->P); return MS_ERR_INVALID; }
    if (seqs->R != r->R) { set_error("the result was made over %lld regions, the sequence set holds %lld", (long long) r->R, (long long) seqs->R); return MS_ERR_INVALID; }
    if (seqs->device != r->device) { set_error("the sequence set lives on device %d, the result on device %d", seqs->device, r->device); return MS_ERR_INVALID; }
    const int32_t rows = m1 - m0;
    if (rows == 0) return MS_OK;
    if (!counts) { set_error("NULL output"); return MS_ERR_INVALID; }
    const int C = pwms->max_width + 2 * flank;
    void *outs[3] = {counts, dinuc, n_sites};
    const size_t out_bytes[3] = {8 * (size_t) rows * 6 * (size_t) C, 8 * (size_t) rows * 16 * (size_t) C, 8 * (size_t) rows};
    bool on_dev[3] = {false, false, false};
    for (int i = 0; i < 3; ++i) {
        if (!outs[i]) continue;
        int other = -1;
        const int place = pointer_place(outs[i], r->device, &other);
        if (place < 0) { set_error("output lives on device %d, the result on device %d", other, r->device); return MS_ERR_INVALID; }
        on_dev[i] = place > 0;
    }
    DeviceCtx *c;
    int rc = get_ctx(r->device, &c);
    if (rc) return rc;
    std::vector<int32_t> width;
    std::vector<int64_t> sites;
    int64_t most = 0;
    try {
        width.assign(pwms->widths.begin() + m0, pwms->widths.begin() + m1);
        sites.resize((size_t) rows);
        for (int32_t i = 0; i < rows; ++i) {
            sites[(size_t) i] = r->motif_offsets[(size_t) (m0 + i) + 1] - r->motif_offsets[(size_t) (m0 + i)];
            most = std::max(most, sites[(size_t) i]);
        }
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }

    std::lock_guard<std::mutex> lk_dev(c->mu);
    MS_HIP(hipSetDevice(c->device));
    const size_t b_cnt = on_dev[0] ? 0 : up256(out_bytes[0]), b_di = (!dinuc || on_dev[1]) ? 0 : up256(out_bytes[1]), b_w = up256(4 * (size_t) rows);
    void *blk = nullptr;
    size_t got = 0;
    if ((rc = pool_alloc(c, b_cnt + b_di + b_w + 256, &blk, &got))) return rc;
    auto hip_fail = [&](hipError_t e, const char *what) {
        pool_free(c, blk, got);
        set_error("%s failed: %s", what, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? MS_ERR_NOMEM : MS_ERR_RUNTIME;
    };
    char *b = static_cast<char *>(blk);
    unsigned long long *d_counts = on_dev[0] ? reinterpret_cast<unsigned long long *>(counts) : reinterpret_cast<unsigned long long *>(b);
    unsigned long long *d_dinuc = !dinuc ? nullptr : on_dev[1] ? reinterpret_cast<unsigned long long *>(dinuc) : reinterpret_cast<unsigned long long *>(b + b_cnt);
    int32_t *d_width = reinterpret_cast<int32_t *>(b + b_cnt + b_di);
    unsigned int *d_bad = reinterpret_cast<unsigned int *>(b + b_cnt + b_di + b_w);
    unsigned int bad = 0;
    const hipStream_t st = c->stream;
    hipError_t he = hipMemsetAsync(d_counts, 0, out_bytes[0], st);
    if (he == hipSuccess && dinuc) he = hipMemsetAsync(d_dinuc, 0, out_bytes[1], st);
    if (he == hipSuccess) he = hipMemsetAsync(d_bad, 0, 256, st);
    if (he == hipSuccess) he = hipMemcpyAsync(d_width, width.data(), 4 * (size_t) rows, hipMemcpyHostToDevice, st);
    if (he != hipSuccess) return hip_fail(he, "clearing the site stacks");
    const bool launched = most > 0;
    if (launched) {
        if ((rc = seqset_pack_pending(seqs, st))) { pool_free(c, blk, got); return rc; }
        StackArgs A;
        A.motif_first = r->d_motif_first; A.seq_idx = r->d_seq_idx; A.pos = r->d_pos; A.strand = r->d_strand;
        A.codes = seqs->d_codes; A.nmask = seqs->d_nmask; A.offsets = seqs->d_offsets; A.R = seqs->R;
        A.width = d_width;
        A.m0 = m0; A.row0 = 0; A.flank = flank; A.C = C;
        A.counts = d_counts; A.dinuc = d_dinuc; A.bad = d_bad;
        const bool lds = C <= kStackLdsC;
        const size_t lds_bytes = lds ? 4 * (size_t) C * (dinuc ? kStackColCells : 6) : 0;
        const int64_t n_chunks = (most + kStackChunk - 1) / kStackChunk;
        const int64_t gx = std::max<int64_t>(std::min<int64_t>(kStackMaxBlocksX, n_chunks), (n_chunks + kStackMaxChunksPerBlock - 1) / kStackMaxChunksPerBlock);
        (void) hipEventRecord(c->ev[0], st);
        for (int32_t row0 = 0; row0 < rows; row0 += kStackGridY) {
            A.row0 = row0;
            const dim3 grid((unsigned) gx, (unsigned) std::min<int32_t>(kStackGridY, rows - row0)), block(kStackThreads);
            if (lds && dinuc) hipLaunchKernelGGL((sitestack_kernel<true, true>), grid, block, lds_bytes, st, A);
            else if (lds) hipLaunchKernelGGL((sitestack_kernel<true, false>), grid, block, lds_bytes, st, A);
            else if (dinuc) hipLaunchKernelGGL((sitestack_kernel<false, true>), grid, block, 0, st, A);
            else hipLaunchKernelGGL((sitestack_kernel<false, false>), grid, block, 0, st, A);
            if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "site-stack kernel");
        }
        (void) hipEventRecord(c->ev[1], st);
    }
    if (!on_dev[0]) he = hipMemcpyAsync(counts, d_counts, out_bytes[0], hipMemcpyDeviceToHost, st);
    if (he == hipSuccess && dinuc && !on_dev[1]) he = hipMemcpyAsync(dinuc, d_dinuc, out_bytes[1], hipMemcpyDeviceToHost, st);
    if (he == hipSuccess && n_sites && on_dev[2]) he = hipMemcpyAsync(n_sites, sites.data(), out_bytes[2], hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) return hip_fail(he, "site stacks");
    if (n_sites && !on_dev[2]) std::memcpy(n_sites, sites.data(), out_bytes[2]);
    float ms01 = 0;
    if (launched) (void) hipEventElapsedTime(&ms01, c->ev[0], c->ev[1]);
    if (device_ms) *device_ms = ms01;
    if (bad) {
        for (int i = 0; i < 3 && he == hipSuccess; ++i) {
            if (!outs[i]) continue;
            if (on_dev[i]) he = hipMemsetAsync(outs[i], 0, out_bytes[i], st);
            else std::memset(outs[i], 0, out_bytes[i]);
        }
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        if (he != hipSuccess) return hip_fail(he, "clearing the site stacks");
        pool_free(c, blk, got);
        set_error("a site does not lie inside its region (region index outside [0, R), pos < 0 or pos + W > L): the result and the sequence set do not belong together");
        return MS_ERR_INVALID;
    }
    pool_free(c, blk, got);
    return MS_OK;
}

}  // extern "C"
