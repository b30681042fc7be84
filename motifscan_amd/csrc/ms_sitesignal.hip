// ms_sitesignal.hip -- a per-base SIGNAL read over the sites of a result: a resident track (ms_track: one int32 per base of a sequence
// set, laid out by the same offsets) and, for every motif, the sum of the track under each motif column (and under `flank` columns
// either side) over the motif's sites, in the motif's orientation and per strand, with the number of sites that cover the column -- the
// footprint profile -- and per site the sums over its upstream flank, its core and its downstream flank (ms_result_site_signal).  No
// reference counterpart: the reference hands its hit lists to the caller, who slices arrays in Python.  Exact int64 sums, additive over
// shards of the regions, the same bytes on every run.
//
//   sitesignal_kernel    grid y = motif row, x = blocks over chunks of kSigChunk hits of the motif's slice (a block takes every
//                        gridDim.x-th chunk), z = panels of kSigPanel columns (a row of up to kSigPanel columns, flank <= 64 with any
//                        usual motif, is one panel).  The geometry is the site stack's, the access is not: a site reads
//                        W + 2 * flank int32, hundreds of bytes, so a WAVE takes a site and its lanes lie across the columns.  Lane l
//                        owns the panel's columns 4 l .. 4 l + 3: the four are contiguous in the track, so a site is ONE 16-byte load
//                        per lane, 1 KiB per wave, in either orientation ('-' reads the same words from the other end and takes
//                        them in reverse order; nothing is complemented).  The load is aligned to 4 bytes only -- a site starts
//                        anywhere.  A lane loads iff one of its four columns is INSIDE the region (a per-lane compare against the
//                        region's bounds); its load then starts at most 3 values in front of the region and ends at most 3 behind
//                        it: in a neighbour's values, or, for the set's first and last region, in the kTrackPad values the track
//                        keeps at either end.  What was loaded for an outside column is dropped.
//                        A wave reads the coordinates of 64 sites at once, one per lane (coalesced; the two offsets of the region
//                        behind them), and each lane turns its site into three numbers: the track index of column 0 and the range
//                        [cl, cl + len) of columns that are inside (one range, in either orientation).  The wave then walks the 64
//                        with v_readlane: those three and the strand are wave-uniform, inside / outside is one subtract and one
//                        unsigned compare per column, the load address is a uniform base plus the lane's constant share, and the
//                        only memory latency inside the walk is the track's.  The two strands are two copies of the column code
//                        behind a uniform branch; the '-' copy keeps its registers in the order of the loaded words, so no value is
//                        moved to be reversed (the flush turns them round).
//                        Profile: a lane keeps the sums (int64) and covers of its 4 columns x 2 strands in registers over ALL sites
//                        its wave takes -- no atomic until the wave is done; then one LDS add per counter folds the block's four
//                        waves, and the block flushes once with 64-bit global adds.  Integer addition commutes: the bytes are the
//                        same on every run.
//                        Per site: the three partial sums of a lane (upstream, core, downstream; a lane's four columns may straddle a
//                        boundary) are folded over the wave by a butterfly that halves the VALUES with the lanes in its first two
//                        steps -- 7 64-bit exchanges instead of 18 -- and lanes 0, 16 and 32 store the triple; a row of several
//                        panels adds its panels' triples with 64-bit atomics onto a zeroed array instead.
//                        A site outside its region (a result of caller-supplied arrays, or the wrong track) reads nothing, is not
//                        counted and raises a flag; the call then fails with the outputs zeroed.
//                        Registers over LDS counters for the profile: the LDS form costs two LDS atomics per lane and site, the
//                        register form two VALU adds; chosen on that count, the two have not been timed against each other, nor has
//                        a 4-byte load per lane (64 columns a step) against the 16-byte one.  Timed: the walk with
//                        64-bit track indices compared against the region's bounds per column and the '-' words reversed by
//                        selects took 1.29 ms where this form takes 0.88 (profile, flank 64, the benchmark's block).
#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "ms_device.h"
#include "ms_handles.h"

namespace ms {
namespace {

constexpr int kTrackPad = 4;                       // zeroed values in front of a track's first value and behind its last: a 16-byte load that
                                                   // holds one inside column reaches at most 3 values past either end of the block's values
constexpr int kSigThreads = 256;
constexpr int kSigChunk = 1024;                    // hits per chunk: 4 batches of 64 per wave
constexpr int kSigPanel = 256;                     // columns of one block: 4 per lane, one 16-byte load
constexpr int kSigMaxBlocksX = 1024;
constexpr int kSigGridY = 32768;                   // motif rows per launch
constexpr int64_t kSigMaxChunksPerBlock = 1LL << 21;       // x kSigChunk hits = 2^31: a block's 32-bit cover counters cannot overflow

static_assert(kTrackPad >= 3, "a 16-byte load with one inside column starts up to 3 values in front of the first value");
static_assert(kSigPanel == 4 * 64 && kSigThreads % 64 == 0 && kSigChunk % kSigThreads == 0, "four columns per lane, whole waves, whole trips");

struct SigArgs {
    const int64_t *motif_first, *seq_idx, *pos;
    const int8_t *strand;
    const int32_t *values;                         // the track's first value
    const int64_t *offsets;
    int64_t R, k_base;                             // k_base: the first hit of motif m0 (per_site row 0)
    const int32_t *width;                          // [rows]
    int32_t m0, row0, flank, C, panels;
    unsigned long long *sum, *cover;               // [rows][2][C], zeroed by the caller; cover may be NULL
    unsigned long long *n_sites;                   // [rows][2], zeroed by the caller
    long long *per_site;                           // [n_sel][3]; zeroed by the caller when panels > 1
    unsigned int *bad;                             // set when a site does not lie inside its region
};

struct __attribute__((packed, aligned(4))) Quad { int32_t v[4]; };     // four values at any 4-byte boundary

__device__ __forceinline__ int64_t lane_value(int64_t v, int i) {     // lane i's v in every lane; i wave-uniform
    const uint32_t lo = (uint32_t) __builtin_amdgcn_readlane((int) (uint32_t) v, i);
    const uint32_t hi = (uint32_t) __builtin_amdgcn_readlane((int) (uint32_t) ((uint64_t) v >> 32), i);
    return (int64_t) (((uint64_t) hi << 32) | lo);
}

// One site's four columns of a lane.  The inside columns of a site are one range [cl, cl + len) of column space (made where the site's
// coordinates are read), so a column is inside iff (unsigned) (j - cl) < len.  `at` is wave-uniform and voff the lane's share: the four
// values at at[voff .. voff + 3].  On '+' component cc is column j0 + cc; on '-' the same words are read from the other end, component cc
// is column j0 + 3 - cc, and acc / cov are kept in COMPONENT order (the flush turns them round): no value changes its register.
template <bool kMinus, bool kProfile, bool kPerSite>
__device__ __forceinline__ void take_site(const int32_t *at, unsigned int voff, int j0, int cl, unsigned int len, int flank, int W,
                                          long long (&acc)[4], unsigned int (&cov)[4], long long (&part)[3]) {
    bool in[4], any = false;
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
        in[cc] = (unsigned int) (j0 + (kMinus ? 3 - cc : cc) - cl) < len;
        any = any || in[cc];
    }
    Quad q = {{0, 0, 0, 0}};
    if (any) q = *reinterpret_cast<const Quad *>(at + voff);                   // at most 3 values past either end of the region: inside the pads
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
        const long long x = in[cc] ? (long long) q.v[cc] : 0ll;
        if (kProfile) {
            acc[cc] += x;
            cov[cc] += in[cc] ? 1u : 0u;
        }
        if (kPerSite) {
            const int j = j0 + (kMinus ? 3 - cc : cc);
            part[0] += j < flank ? x : 0ll;
            part[1] += (j >= flank && j < flank + W) ? x : 0ll;
            part[2] += j >= flank + W ? x : 0ll;
        }
    }
}

template <bool kProfile, bool kPerSite>
__global__ __launch_bounds__(kSigThreads) void sitesignal_kernel(SigArgs A) {
    __shared__ unsigned long long s_sum[2 * kSigPanel];
    __shared__ unsigned int s_cov[2 * kSigPanel];
    const int row = A.row0 + (int) blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t a0 = A.motif_first[A.m0 + row], a1 = A.motif_first[A.m0 + row + 1];
    const int64_t n_chunks = (a1 - a0 + kSigChunk - 1) / kSigChunk;
    const int flank = A.flank, W = A.width[row], ncol = W + 2 * flank, c0 = (int) blockIdx.z * kSigPanel;
    if ((int64_t) blockIdx.x >= n_chunks || c0 >= ncol) return;                // uniform over the block
    if (kProfile) {
        for (int i = tid; i < 2 * kSigPanel; i += kSigThreads) { s_sum[i] = 0; s_cov[i] = 0; }
        __syncthreads();
    }
    const int j0 = c0 + 4 * lane;                                              // the lane's columns: j0 .. j0 + 3
    const unsigned int voff_p = 4u * (unsigned int) lane, voff_m = 4u * (unsigned int) (63 - lane);
    long long acc_p[4] = {}, acc_m[4] = {};                                    // acc_m, cov_m: in component order (take_site)
    unsigned int cov_p[4] = {}, cov_m[4] = {};
    unsigned int n_str[2] = {0, 0};                                            // wave-uniform: the sites of either strand
    for (int64_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        const int64_t cb = a0 + ch * kSigChunk, ce = std::min<int64_t>(cb + kSigChunk, a1);
        for (int64_t k0 = cb + 64 * wave; k0 < ce; k0 += kSigThreads) {        // 64 sites, one per lane
            const int64_t k = k0 + lane;
            bool ok = k < ce, minus = false;
            int64_t base = 0;                                                  // the track index of the site's column 0
            int cl = 0, len = 0;                                               // its inside columns: [cl, cl + len)
            if (ok) {
                const int64_t r = A.seq_idx[k], p = A.pos[k];
                minus = A.strand[k] == 2;
                if (r < 0 || r >= A.R) ok = false;
                else {
                    const int64_t lo = A.offsets[r], L = A.offsets[r + 1] - lo;
                    if (p < 0 || p > L - W) ok = false;
                    else {
                        // '+': column j reads p - flank + j, inside for flank - p <= j < L - p + flank;
                        // '-': column j reads p + W - 1 + flank - j, inside for p + W + flank - L <= j < p + W + flank
                        base = minus ? lo + p + W - 1 + flank : lo + p - flank;
                        const int64_t first = minus ? p + W + flank - L : flank - p, end = minus ? p + W + flank : L - p + flank;
                        cl = (int) std::max<int64_t>(first, 0);                // <= flank
                        len = (int) std::min<int64_t>(end, ncol) - cl;         // end >= flank + W: the core is always inside
                    }
                }
                if (!ok) *A.bad = 1u;
            }
            const unsigned long long okm = __ballot(ok), mim = __ballot(ok && minus);
            n_str[0] += (unsigned int) __popcll(okm & ~mim);
            n_str[1] += (unsigned int) __popcll(mim);
            const int n = (int) std::min<int64_t>(64, ce - k0);
            for (int i = 0; i < n; ++i) {
                if (!((okm >> i) & 1ull)) continue;                            // uniform over the wave
                const int64_t b = lane_value(base, i);
                const int s_cl = __builtin_amdgcn_readlane(cl, i);
                const unsigned int s_len = (unsigned int) __builtin_amdgcn_readlane(len, i);
                long long part[3] = {0, 0, 0};
                // '+': the lane's columns lie at b + j0 ..; '-': at b - j0 - 3 .. = (b - c0 - 255) + 4 (63 - lane) ..
                if ((mim >> i) & 1ull) take_site<true, kProfile, kPerSite>(A.values + (b - c0 - (kSigPanel - 1)), voff_m, j0, s_cl, s_len, flank, W, acc_m, cov_m, part);
                else take_site<false, kProfile, kPerSite>(A.values + (b + c0), voff_p, j0, s_cl, s_len, flank, W, acc_p, cov_p, part);
                if (kPerSite) {
                    // (up, core, down, 0) over 64 lanes: the first two steps halve the values with the lanes, the last four fold one value
                    const bool up32 = lane & 32, up16 = lane & 16;
                    const long long ka = up32 ? part[2] : part[0], kb = up32 ? 0ll : part[1];
                    const long long sa = up32 ? part[0] : part[2], sb = up32 ? part[1] : 0ll;
                    const long long a = ka + __shfl_xor(sa, 32), bb = kb + __shfl_xor(sb, 32);
                    long long x = (up16 ? bb : a) + __shfl_xor(up16 ? a : bb, 16);
                    x += __shfl_xor(x, 8);
                    x += __shfl_xor(x, 4);
                    x += __shfl_xor(x, 2);
                    x += __shfl_xor(x, 1);
                    if ((lane & 15) == 0 && lane < 48) {                        // lane 0: upstream, 16: core, 32: downstream
                        long long *dst = A.per_site + 3 * (k0 + i - A.k_base) + (lane >> 4);
                        if (A.panels == 1) *dst = x;
                        else if (x) atomicAdd(reinterpret_cast<unsigned long long *>(dst), (unsigned long long) x);
                    }
                }
            }
        }
    }
    if (blockIdx.z == 0 && lane < 2 && n_str[lane])
        atomicAdd(&A.n_sites[2 * (size_t) row + lane], (unsigned long long) n_str[lane]);
    if (!kProfile) return;
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
        const int cell_p = 4 * lane + cc, cell_m = kSigPanel + 4 * lane + 3 - cc;
        if (acc_p[cc]) atomicAdd(&s_sum[cell_p], (unsigned long long) acc_p[cc]);
        if (cov_p[cc]) atomicAdd(&s_cov[cell_p], cov_p[cc]);
        if (acc_m[cc]) atomicAdd(&s_sum[cell_m], (unsigned long long) acc_m[cc]);
        if (cov_m[cc]) atomicAdd(&s_cov[cell_m], cov_m[cc]);
    }
    __syncthreads();
    for (int i = tid; i < 2 * kSigPanel; i += kSigThreads) {
        const int s = i / kSigPanel, j = c0 + i % kSigPanel;
        if (j >= ncol) continue;
        const size_t cell = ((size_t) row * 2 + s) * (size_t) A.C + j;
        if (s_sum[i]) atomicAdd(&A.sum[cell], s_sum[i]);
        if (A.cover && s_cov[i]) atomicAdd(&A.cover[cell], (unsigned long long) s_cov[i]);
    }
}

}  // namespace
}  // namespace ms

using namespace ms;

extern "C" {

int ms_debug_sitesignal_dims(int32_t out[4]) {
    if (!out) { set_error("NULL output"); return MS_ERR_INVALID; }
    out[0] = kSigThreads;
    out[1] = kSigChunk;
    out[2] = kSigPanel;
    out[3] = kSigMaxBlocksX;
    return MS_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the track --

int ms_track_create(const int32_t *values, const int64_t *offsets, int64_t n_seqs, ms_track **out) {
    if (!require_device()) return MS_ERR_RUNTIME;
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    if (n_seqs < 0) { set_error("n_seqs < 0"); return MS_ERR_INVALID; }
    if (!offsets) { set_error("offsets is NULL"); return MS_ERR_INVALID; }
    if (offsets[0] != 0) { set_error("offsets[0] must be 0"); return MS_ERR_INVALID; }
    for (int64_t r = 0; r < n_seqs; ++r)
        if (offsets[r + 1] < offsets[r]) { set_error("offsets must be non-decreasing (at %lld)", (long long) r); return MS_ERR_INVALID; }
    const int64_t n = offsets[n_seqs];
    if (n > 0 && !values) { set_error("values is NULL"); return MS_ERR_INVALID; }
    const int device = current_device();
    int place = 0, other = -1;
    if (n > 0 && (place = pointer_place(values, device, &other)) < 0) {
        set_error("the values live on device %d, the calling thread's device is %d", other, device);
        return MS_ERR_INVALID;
    }
    DeviceCtx *c;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    ms_track *t = new (std::nothrow) ms_track();
    if (!t) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    t->device = device;
    t->R = n_seqs;
    t->n_values = n;
    try { t->offsets.assign(offsets, offsets + n_seqs + 1); }
    catch (const std::bad_alloc &) { delete t; set_error("out of host memory"); return MS_ERR_NOMEM; }

    std::lock_guard<std::mutex> lk_dev(c->mu);
    hipError_t he = hipSetDevice(c->device);
    if (he != hipSuccess) { delete t; set_error("hipSetDevice failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    const size_t b_val = up256(4 * ((size_t) n + 2 * kTrackPad)), b_off = up256(8 * ((size_t) n_seqs + 1));
    size_t got = 0;
    if ((rc = pool_alloc(c, b_val + b_off, &t->block, &got))) { delete t; return rc; }
    t->block_bytes = got;
    char *b = static_cast<char *>(t->block);
    t->d_values = reinterpret_cast<int32_t *>(b) + kTrackPad;
    t->d_offsets = reinterpret_cast<int64_t *>(b + b_val);
    const hipStream_t st = c->stream;
    he = hipMemsetAsync(b, 0, 4 * kTrackPad, st);
    if (he == hipSuccess) he = hipMemsetAsync(t->d_values + n, 0, 4 * kTrackPad, st);
    if (he == hipSuccess && n > 0) he = hipMemcpyAsync(t->d_values, values, 4 * (size_t) n, place > 0 ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(t->d_offsets, t->offsets.data(), 8 * ((size_t) n_seqs + 1), hipMemcpyHostToDevice, st);
    const hipError_t hs = hipStreamSynchronize(st);                            // also on an error: the block goes back to the pool below
    if (he == hipSuccess) he = hs;
    if (he != hipSuccess) {
        pool_free(c, t->block, t->block_bytes);
        delete t;
        set_error("upload of the track failed: %s", hipGetErrorString(he));
        return he == hipErrorOutOfMemory ? MS_ERR_NOMEM : MS_ERR_RUNTIME;
    }
    *out = t;
    return MS_OK;
}

int ms_track_size(const ms_track *t, int64_t *n_seqs, int64_t *n_values) {
    if (!t) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (n_seqs) *n_seqs = t->R;
    if (n_values) *n_values = t->n_values;
    return MS_OK;
}

int ms_track_values_host(const ms_track *t, int64_t first, int64_t n, int32_t *out) {
    if (!t) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (first < 0 || n < 0 || first > t->n_values || n > t->n_values - first) { set_error("values [%lld, %lld + %lld) outside the track's %lld", (long long) first, (long long) first, (long long) n, (long long) t->n_values); return MS_ERR_INVALID; }
    if (n == 0) return MS_OK;
    if (!out) { set_error("NULL output"); return MS_ERR_INVALID; }
    MS_HIP(hipSetDevice(t->device));
    MS_HIP(hipMemcpy(out, t->d_values + first, 4 * (size_t) n, hipMemcpyDeviceToHost));
    return MS_OK;
}

void ms_track_free(ms_track *t) {
    if (!t) return;
    (void) hipSetDevice(t->device);
    DeviceCtx *c = nullptr;
    if (t->block) {
        if (get_ctx(t->device, &c) == MS_OK) pool_free(c, t->block, t->block_bytes);
        else (void) hipFree(t->block);
    }
    delete t;
}

// ------------------------------------------------------------------------------------------------------------ the reduction --

int ms_result_site_signal(const ms_result *r, const ms_pwmset *pwms, const ms_track *track, int32_t flank, int32_t m0, int32_t m1, uint32_t flags,
                          int64_t *sum, int64_t *cover, int64_t *n_sites, int64_t *per_site, double *device_ms) {
    if (!require_device()) return MS_ERR_RUNTIME;
    if (device_ms) *device_ms = 0.0;
    if (!r || !pwms || !track) { set_error("NULL handle"); return MS_ERR_INVALID; }
    if (!sum && !per_site) { set_error("NULL outputs: at least one of sum and per_site is needed"); return MS_ERR_INVALID; }
    if (flags != 0) { set_error("unknown site-signal flags 0x%x", flags); return MS_ERR_INVALID; }
    if (flank < 0 || flank > MS_SITESIGNAL_MAX_FLANK) { set_error("flank must be in [0, %d]", MS_SITESIGNAL_MAX_FLANK); return MS_ERR_INVALID; }
    if (r->counts_only) { set_error("a counts-only result (MS_SCAN_COUNTS_ONLY, a counts-only batch or sweep span of a stream) holds the per-motif region counts and site numbers, no site arrays"); return MS_ERR_INVALID; }
    if (pwms->P != r->P) { set_error("result and PWM set disagree on the number of PWMs"); return MS_ERR_INVALID; }
    if (m0 < 0 || m1 < m0 || m1 > r->P) { set_error("motif range [%d, %d) outside [0, %d)", m0, m1, r->P); return MS_ERR_INVALID; }
    if (track->R != r->R) { set_error("the result was made over %lld regions, the track holds %lld", (long long) r->R, (long long) track->R); return MS_ERR_INVALID; }
    if (track->device != r->device) { set_error("the track lives on device %d, the result on device %d", track->device, r->device); return MS_ERR_INVALID; }
    const int32_t rows = m1 - m0;
    if (rows == 0) return MS_OK;
    const int C = pwms->max_width + 2 * flank;
    const int64_t k_base = r->motif_offsets[(size_t) m0], n_sel = r->motif_offsets[(size_t) m1] - k_base;
    void *outs[4] = {sum, cover, n_sites, per_site};
    const size_t out_bytes[4] = {8 * (size_t) rows * 2 * (size_t) C, 8 * (size_t) rows * 2 * (size_t) C, 8 * (size_t) rows * 2, 8 * 3 * (size_t) n_sel};
    bool on_dev[4] = {false, false, false, false};
    for (int i = 0; i < 4; ++i) {
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
    int64_t most = 0;
    int widest = 0;
    try {
        width.assign(pwms->widths.begin() + m0, pwms->widths.begin() + m1);
        for (int32_t i = 0; i < rows; ++i) {
            const int64_t n = r->motif_offsets[(size_t) (m0 + i) + 1] - r->motif_offsets[(size_t) (m0 + i)];
            most = std::max(most, n);
            if (n > 0) widest = std::max(widest, width[(size_t) i]);
        }
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    const int panels = std::max(1, (widest + 2 * flank + kSigPanel - 1) / kSigPanel);     // of the widest row that has a site

    std::lock_guard<std::mutex> lk_dev(c->mu);
    MS_HIP(hipSetDevice(c->device));
    // what the kernel writes that the caller did not give in device memory: slots of one pooled block
    bool own[4];                                                               // the strand counts are always made on the device
    size_t slot[4], at = 0;
    for (int i = 0; i < 4; ++i) {
        own[i] = i == 2 ? !on_dev[2] : (outs[i] && !on_dev[i]);
        slot[i] = at;
        if (own[i]) at += up256(out_bytes[i]);
    }
    const size_t at_w = at, at_bad = at_w + up256(4 * (size_t) rows);
    void *blk = nullptr;
    size_t got = 0;
    if ((rc = pool_alloc(c, at_bad + 256, &blk, &got))) return rc;
    auto hip_fail = [&](hipError_t e, const char *what) {
        (void) hipStreamSynchronize(c->stream);
        pool_free(c, blk, got);
        set_error("%s failed: %s", what, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? MS_ERR_NOMEM : MS_ERR_RUNTIME;
    };
    char *b = static_cast<char *>(blk);
    unsigned long long *d_out[4];
    for (int i = 0; i < 4; ++i)
        d_out[i] = own[i] ? reinterpret_cast<unsigned long long *>(b + slot[i]) : reinterpret_cast<unsigned long long *>(outs[i]);
    int32_t *d_width = reinterpret_cast<int32_t *>(b + at_w);
    unsigned int *d_bad = reinterpret_cast<unsigned int *>(b + at_bad);
    unsigned int bad = 0;
    const hipStream_t st = c->stream;
    hipError_t he = hipMemsetAsync(d_bad, 0, 256, st);
    for (int i = 0; i < 4 && he == hipSuccess; ++i) {
        if (!d_out[i] || out_bytes[i] == 0) continue;
        if (i == 3 && panels == 1) continue;                                   // every row of per_site is stored whole
        he = hipMemsetAsync(d_out[i], 0, out_bytes[i], st);
    }
    if (he == hipSuccess) he = hipMemcpyAsync(d_width, width.data(), 4 * (size_t) rows, hipMemcpyHostToDevice, st);
    if (he != hipSuccess) return hip_fail(he, "clearing the site signal");
    const bool launched = most > 0;
    if (launched) {
        SigArgs A;
        A.motif_first = r->d_motif_first; A.seq_idx = r->d_seq_idx; A.pos = r->d_pos; A.strand = r->d_strand;
        A.values = track->d_values; A.offsets = track->d_offsets; A.R = track->R; A.k_base = k_base;
        A.width = d_width;
        A.m0 = m0; A.row0 = 0; A.flank = flank; A.C = C; A.panels = panels;
        A.sum = d_out[0]; A.cover = d_out[1]; A.n_sites = d_out[2]; A.per_site = reinterpret_cast<long long *>(d_out[3]); A.bad = d_bad;
        const int64_t n_chunks = (most + kSigChunk - 1) / kSigChunk;
        const int64_t gx = std::max<int64_t>(std::min<int64_t>(kSigMaxBlocksX, n_chunks), (n_chunks + kSigMaxChunksPerBlock - 1) / kSigMaxChunksPerBlock);
        (void) hipEventRecord(c->ev[0], st);
        for (int32_t row0 = 0; row0 < rows; row0 += kSigGridY) {
            A.row0 = row0;
            const dim3 grid((unsigned) gx, (unsigned) std::min<int32_t>(kSigGridY, rows - row0), (unsigned) panels), block(kSigThreads);
            if (sum && per_site) hipLaunchKernelGGL((sitesignal_kernel<true, true>), grid, block, 0, st, A);
            else if (sum) hipLaunchKernelGGL((sitesignal_kernel<true, false>), grid, block, 0, st, A);
            else hipLaunchKernelGGL((sitesignal_kernel<false, true>), grid, block, 0, st, A);
            if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "site-signal kernel");
        }
        (void) hipEventRecord(c->ev[1], st);
    }
    for (int i = 0; i < 4 && he == hipSuccess; ++i)
        if (outs[i] && !on_dev[i] && out_bytes[i]) he = hipMemcpyAsync(outs[i], d_out[i], out_bytes[i], hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) return hip_fail(he, "site signal");
    float ms01 = 0;
    if (launched) (void) hipEventElapsedTime(&ms01, c->ev[0], c->ev[1]);
    if (device_ms) *device_ms = ms01;
    if (bad) {
        for (int i = 0; i < 4 && he == hipSuccess; ++i) {
            if (!outs[i] || out_bytes[i] == 0) continue;
            if (on_dev[i]) he = hipMemsetAsync(outs[i], 0, out_bytes[i], st);
            else std::memset(outs[i], 0, out_bytes[i]);
        }
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        if (he != hipSuccess) return hip_fail(he, "clearing the site signal");
        pool_free(c, blk, got);
        set_error("a site does not lie inside its region (region index outside [0, R), pos < 0 or pos + W > L): the result and the track do not belong together");
        return MS_ERR_INVALID;
    }
    pool_free(c, blk, got);
    return MS_OK;
}

}  // extern "C"
