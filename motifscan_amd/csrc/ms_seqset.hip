// ms_seqset.hip -- the sequence set handle (four ways to build one: device pack, host pack, upload now / pack in front of the scan, from
// device memory) and the resident genome, which is a sequence set whose sequences are the chromosomes.
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

// --------------------------------------------------------------------------- pack --

constexpr int kPackThreads = 256;                // pack_kernel, extract_kernel, blk2reg_kernel: one block
int32_t seqset_block_bases() { return kPackThreads * 32; }

// One thread per 32 bases: two 16-byte loads, one 8-byte + one 4-byte store.
__global__ void __launch_bounds__(kPackThreads) pack_kernel(const uint8_t *__restrict__ ascii, int64_t n_bases,
                                                   uint32_t *__restrict__ codes, uint32_t *__restrict__ nmask,
                                                   int64_t n_units, int aligned16) {
    const int64_t u = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_units) return;
    const int64_t base = u * 32;
    uint32_t raw[8];
    if (aligned16 && base + 32 <= n_bases) {
        const uint4 a = *reinterpret_cast<const uint4 *>(ascii + base);
        const uint4 b = *reinterpret_cast<const uint4 *>(ascii + base + 16);
        raw[0] = a.x; raw[1] = a.y; raw[2] = a.z; raw[3] = a.w;
        raw[4] = b.x; raw[5] = b.y; raw[6] = b.z; raw[7] = b.w;
    } else {
        for (int k = 0; k < 8; k++) {
            uint32_t w = 0;
            for (int j = 0; j < 4; j++) {
                const int64_t i = base + k * 4 + j;
                w |= (uint32_t) (i < n_bases ? ascii[i] : (uint8_t) 'A') << (8 * j);
            }
            raw[k] = w;
        }
    }
    uint64_t cw = 0;
    uint32_t nw = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t ch = ((raw[k] >> (8 * j)) & 0xFFu) | 0x20u;      // fold case (cscore.c:93-108)
            const uint32_t code = ((ch >> 1) ^ (ch >> 2)) & 3u;             // a,c,g,t -> 0,1,2,3
            const bool acgt = ch == 0x61u || ch == 0x63u || ch == 0x67u || ch == 0x74u;
            const int i = k * 4 + j;
            cw |= (uint64_t) (acgt ? code : 0u) << (2 * i);
            nw |= (acgt ? 0u : 1u) << i;
        }
    }
    if (base + 32 > n_bases) {          // bases past the end are neither N nor scanned
        const int valid = (int) (n_bases - base);
        nw &= low_mask(valid);
    }
    codes[2 * u] = (uint32_t) cw;
    codes[2 * u + 1] = (uint32_t) (cw >> 32);
    nmask[u] = nw;
}

// --------------------------------------------------------------- on-device extraction --

// Regions cut out of a resident packed genome (replaces Scanner._extract_seq -> Genome.fetch_sequence
// -> pysam fetch, scanner.py:71-87 / genome/__init__.py:117-135): one thread per 32 output bases,
// which may straddle several regions.  src_start[r] is the region's first base in the genome's
// packed coordinates; dst_off[r] its first base in the output.
__global__ void __launch_bounds__(kPackThreads) extract_kernel(const uint32_t *__restrict__ gcodes, const uint32_t *__restrict__ gnmask,
                                                      const int64_t *__restrict__ src_start, const int64_t *__restrict__ dst_off,
                                                      int64_t R, int64_t n_out, uint32_t *__restrict__ codes,
                                                      uint32_t *__restrict__ nmask) {
    const int64_t u = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t pos = u * 32;
    if (pos >= n_out) return;
    int64_t r = find_region_bsearch(dst_off, R, pos);
    uint64_t cw = 0;
    uint32_t nw = 0;
    int filled = 0;
    while (filled < 32 && pos + filled < n_out) {
        const int64_t d = pos + filled;
        while (dst_off[r + 1] <= d) r++;                              // skip empty regions
        const int64_t left = dst_off[r + 1] - d;
        const int seg = left < (int64_t) (32 - filled) ? (int) left : 32 - filled;
        const int64_t sp = src_start[r] + (d - dst_off[r]);
        const uint64_t scw = code_window(gcodes, sp);
        const uint32_t snw = n_window(gnmask, sp);
        const uint64_t m = seg >= 32 ? ~0ULL : ((1ULL << (2 * seg)) - 1ULL);
        cw |= (scw & m) << (2 * filled);
        nw |= (snw & low_mask(seg)) << filled;
        filled += seg;
    }
    codes[2 * u] = (uint32_t) cw;
    codes[2 * u + 1] = (uint32_t) (cw >> 32);
    nmask[u] = nw;
}

// ------------------------------------------------------------------- region hints --

// blk2reg[b] = region that holds position 64*b (part of the extraction stage, next to pack_kernel); blkinfo[b] = the same region with
// its own and the next two regions' starts RELATIVE to 64*b as 32-bit numbers -- everything rescore_kernel needs to place a position,
// in one 16-byte read (the fp64 stage pays per vector-memory instruction); region -1: a start lies more than 2^31 bases away, look it up
__global__ void __launch_bounds__(kPackThreads) blk2reg_kernel(const int64_t *__restrict__ offsets, int64_t R, int64_t n_blocks,
                                                      int32_t *__restrict__ blk2reg, int4 *__restrict__ blkinfo, int all_far) {
    const int64_t b = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blocks) return;
    const int64_t r = find_region_bsearch(offsets, R, b * 64);
    blk2reg[b] = (int32_t) r;
    const int64_t base = b * 64;
    const int64_t o0 = offsets[r] - base, o1 = offsets[r + 1 <= R ? r + 1 : R] - base, o2 = offsets[r + 2 <= R ? r + 2 : (r + 1 <= R ? r + 1 : R)] - base;
    const bool fits = o0 > -(1LL << 31) && o1 < (1LL << 31) && o2 < (1LL << 31) && o1 > -(1LL << 31) && o2 > -(1LL << 31) && r < (1LL << 31);
    blkinfo[b] = fits && !all_far ? make_int4((int) r, (int) o0, (int) o1, (int) o2) : make_int4(-1, 0, 0, 0);     // (all_far: a test aid, MS_BLKINFO_FAR)
}

static int launch_extract(const uint32_t *gcodes, const uint32_t *gnmask, const int64_t *src_start, const int64_t *dst_off,
                          int64_t R, int64_t n_out, uint32_t *codes, uint32_t *nmask, hipStream_t st) {
    const int64_t n_units = (n_out + 31) / 32;
    if (n_units == 0) return MS_OK;
    hipLaunchKernelGGL(extract_kernel, dim3((unsigned) ((n_units + kPackThreads - 1) / kPackThreads)), dim3(kPackThreads), 0, st, gcodes, gnmask, src_start,
                       dst_off, R, n_out, codes, nmask);
    MS_HIP(hipGetLastError());
    return MS_OK;
}

static int launch_blk2reg(const int64_t *offsets, int64_t R, int64_t n_bases, int32_t *blk2reg, int4 *blkinfo, hipStream_t st) {
    const int64_t n_blocks = (n_bases + 63) / 64 + 1;
    const int all_far = measure_env("MS_BLKINFO_FAR") ? 1 : 0;          // test aid: every block record says "look the region up" (starts beyond 32 bits)
    hipLaunchKernelGGL(blk2reg_kernel, dim3((unsigned) ((n_blocks + kPackThreads - 1) / kPackThreads)), dim3(kPackThreads), 0, st, offsets, R, n_blocks,
                       blk2reg, blkinfo, all_far);
    MS_HIP(hipGetLastError());
    return MS_OK;
}

static int launch_pack(const uint8_t *ascii, int64_t n_bases, uint32_t *codes, uint32_t *nmask, hipStream_t st) {
    const int64_t n_units = (n_bases + 31) / 32;
    if (n_units == 0) return MS_OK;
    const int aligned16 = (reinterpret_cast<uintptr_t>(ascii) & 15u) == 0;
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned) ((n_units + kPackThreads - 1) / kPackThreads)), dim3(kPackThreads), 0, st, ascii, n_bases,
                       codes, nmask, n_units, aligned16);
    MS_HIP(hipGetLastError());
    return MS_OK;
}

// Host loops over tens of millions of regions (whole-genome window sweeps) are split over a few threads.
template <typename F>
static void parallel_chunks(int64_t n, F fn) {                 // fn(chunk index, begin, end)
    int T = 1;
    if (n >= (1 << 20)) T = (int) std::min<int64_t>(16, std::max<int64_t>(1, (int64_t) std::thread::hardware_concurrency()));
    if (T <= 1) { fn(0, (int64_t) 0, n); return; }
    std::vector<std::thread> th;
    const int64_t step = (n + T - 1) / T;
    for (int t = 0; t < T; t++) {
        const int64_t b = std::min<int64_t>(n, t * step), e = std::min<int64_t>(n, (t + 1) * step);
        th.emplace_back([=]() { fn(t, b, e); });
    }
    for (auto &x : th) x.join();
}
static constexpr int kMaxChunks = 16;

DevSeq dev_seq(const ms_seqset *s) {
    DevSeq d;
    d.codes = s->d_codes; d.nmask = s->d_nmask; d.offsets = s->d_offsets; d.blk2reg = s->d_blk2reg; d.blkinfo = s->d_blkinfo; d.R = s->R;
    d.n_bases = s->n_bases;
    return d;
}

// sum_r max(L_r - W + 1, 0) from the sorted lengths
int64_t windows_for_width(const ms_seqset *s, int W) {
    const auto it = std::lower_bound(s->len_sorted.begin(), s->len_sorted.end(), (int64_t) W);
    const size_t idx = (size_t) (it - s->len_sorted.begin());
    return s->len_sum_ge[idx] - (int64_t) (W - 1) * s->len_cnt_ge[idx];
}

static int seqset_common(const int64_t *offsets, int64_t n_seqs, std::unique_ptr<ms_seqset> &s,
                         std::vector<int64_t> *adopt = nullptr) {
    if (n_seqs < 0) { set_error("n_seqs < 0"); return MS_ERR_INVALID; }
    if (!offsets) { set_error("offsets is NULL"); return MS_ERR_INVALID; }
    if (offsets[0] != 0) { set_error("offsets[0] must be 0"); return MS_ERR_INVALID; }
    // one pass: monotonicity, shortest and longest sequence
    int64_t cmin[kMaxChunks], cmax[kMaxChunks], cbad[kMaxChunks];
    for (int t = 0; t < kMaxChunks; t++) { cmin[t] = INT64_MAX; cmax[t] = 0; cbad[t] = -1; }
    parallel_chunks(n_seqs, [&](int t, int64_t b, int64_t e) {
        int64_t mn = INT64_MAX, mx = 0, bad = -1;
        for (int64_t r = b; r < e; r++) {
            const int64_t L = offsets[r + 1] - offsets[r];
            if (L < 0 && bad < 0) bad = r;
            mn = std::min(mn, L);
            mx = std::max(mx, L);
        }
        cmin[t] = mn; cmax[t] = mx; cbad[t] = bad;
    });
    int64_t lmin = INT64_MAX, lmax = 0;
    for (int t = 0; t < kMaxChunks; t++) {
        if (cbad[t] >= 0) { set_error("offsets must be non-decreasing (at %lld)", (long long) cbad[t]); return MS_ERR_INVALID; }
        lmin = std::min(lmin, cmin[t]);
        lmax = std::max(lmax, cmax[t]);
    }
    s.reset(new (std::nothrow) ms_seqset());
    if (!s) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    s->device = current_device();
    s->R = n_seqs;
    s->n_bases = offsets[n_seqs];
    if (s->n_bases > kMaxBases) { set_error("a sequence set holds at most %lld bases; split the regions over several sets", (long long) kMaxBases); return MS_ERR_INVALID; }
    if (n_seqs >= (1LL << 31)) { set_error("too many sequences in one set"); return MS_ERR_INVALID; }
    try {
        if (adopt) s->offsets.swap(*adopt);
        else s->offsets.assign(offsets, offsets + n_seqs + 1);
        offsets = s->offsets.data();
        // distinct lengths with counts: direct histograms when the lengths span a small range
        // (fixed-size windows: one bin), a sort otherwise
        std::vector<std::pair<int64_t, int64_t>> runs;           // (length, count) ascending
        if (n_seqs > 0 && lmax - lmin <= (1 << 16)) {
            const size_t bins = (size_t) (lmax - lmin + 1);
            std::vector<std::vector<int64_t>> hist(kMaxChunks);
            parallel_chunks(n_seqs, [&](int t, int64_t b, int64_t e) {
                hist[(size_t) t].assign(bins, 0);
                for (int64_t r = b; r < e; r++) hist[(size_t) t][(size_t) (offsets[r + 1] - offsets[r] - lmin)]++;
            });
            for (size_t i = 0; i < bins; i++) {
                int64_t cnt = 0;
                for (int t = 0; t < kMaxChunks; t++) if (!hist[(size_t) t].empty()) cnt += hist[(size_t) t][i];
                if (cnt) runs.emplace_back(lmin + (int64_t) i, cnt);
            }
        } else if (n_seqs > 0) {
            std::vector<int64_t> lens((size_t) n_seqs);
            for (int64_t r = 0; r < n_seqs; r++) lens[(size_t) r] = offsets[r + 1] - offsets[r];
            std::sort(lens.begin(), lens.end());
            for (size_t i = 0; i < lens.size();) {
                size_t j = i;
                while (j < lens.size() && lens[j] == lens[i]) j++;
                runs.emplace_back(lens[i], (int64_t) (j - i));
                i = j;
            }
        }
        const size_t nd = runs.size();
        s->len_sorted.resize(nd);
        s->len_cnt_ge.assign(nd + 1, 0);
        s->len_sum_ge.assign(nd + 1, 0);
        for (size_t i = nd; i-- > 0;) {
            s->len_sorted[i] = runs[i].first;
            s->len_cnt_ge[i] = s->len_cnt_ge[i + 1] + runs[i].second;
            s->len_sum_ge[i] = s->len_sum_ge[i + 1] + runs[i].first * runs[i].second;
        }
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    return MS_OK;
}

static int seqset_alloc_packed(ms_seqset *s, bool pads_by_copy = false, bool defer_pads = false) {
    const size_t n_units = (size_t) ((s->n_bases + 31) / 32);
    const size_t b_codes = (2 * n_units + kPadWords) * sizeof(uint32_t);
    const size_t b_nmask = (n_units + kPadWords) * sizeof(uint32_t);
    const size_t b_off = ((size_t) s->R + 1) * sizeof(int64_t);
    const size_t b_blk = ((size_t) (s->n_bases / 64) + 2) * sizeof(int32_t);
    const size_t b_info = ((size_t) (s->n_bases / 64) + 2) * sizeof(int4);
    auto up = [](size_t x) { return (x + 255) & ~(size_t) 255; };
    DeviceCtx *c;
    int rc = get_ctx(s->device, &c);
    if (rc) return rc;
    if ((rc = pool_alloc(c, up(b_codes) + up(b_nmask) + up(b_off) + up(b_blk) + up(b_info), &s->block, &s->block_bytes))) return rc;
    char *b = static_cast<char *>(s->block);
    s->d_codes = reinterpret_cast<uint32_t *>(b);
    s->d_nmask = reinterpret_cast<uint32_t *>(b + up(b_codes));
    s->d_offsets = reinterpret_cast<int64_t *>(b + up(b_codes) + up(b_nmask));
    s->d_blk2reg = reinterpret_cast<int32_t *>(b + up(b_codes) + up(b_nmask) + up(b_off));
    s->d_blkinfo = reinterpret_cast<int4 *>(b + up(b_codes) + up(b_nmask) + up(b_off) + up(b_blk));
    // only the pad words behind the packed data need clearing: the kernels write everything else
    // sequence sets are built on the upload stream: a batch can be packed while the previous one is being scanned
    s->up = c->stream_up;                                 // read once: every step of building this set stays on one stream
    if (!pads_by_copy && !defer_pads) {                   // (a memset is a KERNEL: the host-packed form copies zero pad words along instead, the upload-only form clears them when it packs)
        MS_HIP(hipMemsetAsync(s->d_codes + 2 * n_units, 0, kPadWords * sizeof(uint32_t), s->up));
        MS_HIP(hipMemsetAsync(s->d_nmask + n_units, 0, kPadWords * sizeof(uint32_t), s->up));
    }
    if (!pads_by_copy) {                                  // (host-packed: the offsets travel in the one copy of the whole block)
        // through pinned words, so that the copy runs on the SDMA engines like the sequence's: from the pageable vector the runtime copies with a one-workgroup
        // KERNEL, which in a batch stream waits for a CU while the previous batch's pre-filter holds them all (profiles/r06z_trace_e2e_gaps_sdma.log: 3.5 ms
        // per batch on the upload stream).  Pageable memory only if no pinned words can be had.
        const void *src = s->offsets.data();
        if ((s->h_off_pin = pinned_alloc(b_off, &s->h_off_pin_bytes))) {
            std::memcpy(s->h_off_pin, s->offsets.data(), b_off);
            src = s->h_off_pin;
        }
        MS_HIP(hipMemcpyAsync(s->d_offsets, src, b_off, hipMemcpyHostToDevice, s->up));
    }
    return MS_OK;
}

// stage / stage_bytes: the caller's grow-only pinned staging block (a batch stream's uploader keeps ONE for its life: page-locking ~90 MB
// per batch costs tens of milliseconds); nullptr: a block of the call's own.
int seqset_create_hostpacked(const char *bases, const int64_t *offsets, int64_t n_seqs, int n_threads, void **stage_io, size_t *stage_bytes_io, ms_seqset **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    std::unique_ptr<ms_seqset> s;
    int rc = seqset_common(offsets, n_seqs, s);
    if (rc) return rc;
    if (s->n_bases > 0 && !bases) { set_error("bases is NULL"); return MS_ERR_INVALID; }
    if (n_threads < 1) n_threads = 1;
    if (n_threads > 64) n_threads = 64;
    DeviceCtx *c;
    if ((rc = get_ctx(s->device, &c))) return rc;
    ms_seqset *raw = s.release();
    auto fail = [&](int code) { ms_seqset_free(raw); return code; };
    if ((rc = seqset_alloc_packed(raw, true))) return fail(rc);
    const int64_t n_units = (raw->n_bases + 31) / 32, n_blocks = (raw->n_bases + 63) / 64 + 1;
    // The staging block MIRRORS the set's device block (seqset_alloc_packed: codes + pad | mask + pad | offsets | region of every 64th
    // position | block records, 256-byte aligned), so that ONE copy moves everything -- no kernel (a memset is one) and no second copy is
    // queued on the upload stream.
    const size_t o_nmask = (size_t) (reinterpret_cast<char *>(raw->d_nmask) - static_cast<char *>(raw->block));
    const size_t o_off = (size_t) (reinterpret_cast<char *>(raw->d_offsets) - static_cast<char *>(raw->block));
    const size_t o_blk = (size_t) (reinterpret_cast<char *>(raw->d_blk2reg) - static_cast<char *>(raw->block));
    const size_t o_info = (size_t) (reinterpret_cast<char *>(raw->d_blkinfo) - static_cast<char *>(raw->block));
    const size_t need = up256(o_info + (size_t) n_blocks * 16) + 256;
    size_t got = 0;
    char *stage = nullptr;
    if (stage_io) {
        if (*stage_bytes_io < need) {
            if (*stage_io) (void) hipHostFree(*stage_io);
            *stage_io = nullptr; *stage_bytes_io = 0;
            void *p = nullptr;
            if (hipHostMalloc(&p, need + need / 8) != hipSuccess) { set_error("out of pinned host memory"); return fail(MS_ERR_NOMEM); }
            *stage_io = p; *stage_bytes_io = need + need / 8;
        }
        stage = static_cast<char *>(*stage_io);
    } else {
        stage = static_cast<char *>(pinned_alloc(need, &got));
        if (!stage) { set_error("out of pinned host memory"); return fail(MS_ERR_NOMEM); }
    }
    auto release = [&]() { if (!stage_io) pinned_free(stage, got); };
    uint32_t *h_codes = reinterpret_cast<uint32_t *>(stage), *h_nmask = reinterpret_cast<uint32_t *>(stage + o_nmask);
    int32_t *h_blk = reinterpret_cast<int32_t *>(stage + o_blk);
    int32_t *h_info = reinterpret_cast<int32_t *>(stage + o_info);
    {
        const bool all_far = measure_env("MS_BLKINFO_FAR") != nullptr;
        const int64_t *off = raw->offsets.data();
        const int64_t R = raw->R, nb = raw->n_bases;
        const int T = (int) std::min<int64_t>(n_threads, std::max<int64_t>(1, n_units / 4096));
        auto work = [&](int t) {
            host_pack_units(reinterpret_cast<const uint8_t *>(bases), nb, n_units * t / T, n_units * (t + 1) / T, h_codes, h_nmask);
            host_region_hints(off, R, n_blocks * t / T, n_blocks * (t + 1) / T, h_blk, h_info, all_far);
        };
        std::vector<std::thread> th;
        try { for (int t = 1; t < T; t++) th.emplace_back(work, t); }
        catch (const std::exception &) { for (auto &x : th) x.join(); release(); set_error("could not start packing threads"); return fail(MS_ERR_RUNTIME); }
        work(0);
        for (auto &x : th) x.join();
        std::memset(h_codes + 2 * n_units, 0, kPadWords * sizeof(uint32_t));
        std::memset(h_nmask + n_units, 0, kPadWords * sizeof(uint32_t));
        std::memcpy(stage + o_off, off, ((size_t) R + 1) * sizeof(int64_t));
    }
    hipError_t e = hipMemcpyAsync(raw->block, stage, o_info + (size_t) n_blocks * 16, hipMemcpyHostToDevice, raw->up);
    if (e == hipSuccess) e = hipStreamSynchronize(raw->up);
    release();
    if (e != hipSuccess) { set_error("upload of the packed set failed: %s", hipGetErrorString(e)); return fail(MS_ERR_RUNTIME); }
    raw->built = true;
    *out = raw;
    return MS_OK;
}

// The batch stream's upload stage (round 6): ONLY the copies -- ASCII and offsets cross the link on the DMA engines, nothing here needs a CU.
// convert_seq (pack_kernel) and the region hints are made by the SCAN stage, on the scan stream, in front of the batch's pre-filter
// (seqset_pack_pending, called by scan_locked).  Why: every kernel launched on the upload stream beside a scan waits for the pre-filter's
// persistent blocks to retire -- a full CU stalls the dispatcher's in-order hand-out (ms_handles.h, StreamSel) -- so the upload stage used
// to end when the PREVIOUS batch's pre-filter did (53 ms of "work" per configs[3] pass for 18 ms of copies and 0.6 ms of kernels,
// profiles/r05d_e2e_bounds.log) and the scan stage could not queue the next batch's scan behind the running one.  On the scan stream the
// two kernels cost what they cost in the resident step (0.3 ms per 500 Mbase) and wait for nothing.
int seqset_create_upload_only(const char *bases, const int64_t *offsets, int64_t n_seqs, ms_seqset **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    std::unique_ptr<ms_seqset> s;
    int rc = seqset_common(offsets, n_seqs, s);
    if (rc) return rc;
    if (s->n_bases > 0 && !bases) { set_error("bases is NULL"); return MS_ERR_INVALID; }
    DeviceCtx *c;
    if ((rc = get_ctx(s->device, &c))) return rc;
    ms_seqset *raw = s.release();
    auto fail = [&](int code) { ms_seqset_free(raw); return code; };
    if ((rc = seqset_alloc_packed(raw, false, true))) return fail(rc);
    {
        void *blk = nullptr;
        if ((rc = pool_alloc(c, (size_t) raw->n_bases + 64, &blk, &raw->ascii_bytes))) return fail(rc);
        raw->d_ascii = static_cast<uint8_t *>(blk);
    }
    hipError_t e = hipSuccess;
    if (raw->n_bases > 0) e = hipMemcpyAsync(raw->d_ascii, bases, (size_t) raw->n_bases, hipMemcpyHostToDevice, raw->up);
    if (e == hipSuccess) e = hipStreamSynchronize(raw->up);
    if (e != hipSuccess) { set_error("H2D copy failed: %s", hipGetErrorString(e)); return fail(MS_ERR_RUNTIME); }
    raw->built = true;
    raw->pack_pending = true;
    *out = raw;
    return MS_OK;
}

// ... and the rest of the set's construction, queued on `st` (the scan stream; the caller holds the device's lock)
int seqset_pack_pending(const ms_seqset *s_c, hipStream_t st) {
    ms_seqset *s = const_cast<ms_seqset *>(s_c);
    if (!s->pack_pending) return MS_OK;
    const size_t n_units = (size_t) ((s->n_bases + 31) / 32);
    MS_HIP(hipMemsetAsync(s->d_codes + 2 * n_units, 0, kPadWords * sizeof(uint32_t), st));
    MS_HIP(hipMemsetAsync(s->d_nmask + n_units, 0, kPadWords * sizeof(uint32_t), st));
    int rc;
    if ((rc = launch_pack(s->d_ascii, s->n_bases, s->d_codes, s->d_nmask, st))) return rc;
    if ((rc = launch_blk2reg(s->d_offsets, s->R, s->n_bases, s->d_blk2reg, s->d_blkinfo, st))) return rc;
    s->pack_pending = false;                       // (queued: everything that reads the set follows on the same stream, or waits for it)
    return MS_OK;
}

// A set of the given offsets on `device` whose planes and region hints are still to be written by the caller's kernels (ms_personal.hip:
// the splice writes the planes, seqset_launch_hints the hints): host tables, the device block, the offsets and the zero pad words, waited for.
int seqset_create_unpacked(const int64_t *offsets, int64_t n_seqs, int device, ms_seqset **out) {
    *out = nullptr;
    const int prev_dev = current_device();
    set_current_device(device);
    std::unique_ptr<ms_seqset> s;
    int rc = seqset_common(offsets, n_seqs, s);
    set_current_device(prev_dev);
    if (rc) return rc;
    ms_seqset *raw = s.release();
    auto fail = [&](int code) { ms_seqset_free(raw); return code; };
    if ((rc = seqset_alloc_packed(raw))) return fail(rc);
    const hipError_t e = hipStreamSynchronize(raw->up);
    if (e != hipSuccess) { set_error("upload of the offsets failed: %s", hipGetErrorString(e)); return fail(MS_ERR_RUNTIME); }
    raw->built = true;
    *out = raw;
    return MS_OK;
}

int seqset_launch_hints(const ms_seqset *s, hipStream_t st) { return launch_blk2reg(s->d_offsets, s->R, s->n_bases, s->d_blk2reg, s->d_blkinfo, st); }

}  // namespace ms

using namespace ms;

extern "C" {

// -------------------------------------------------------------------- sequence set --

int ms_seqset_create(const char *bases, const int64_t *offsets, int64_t n_seqs, int keep_ascii, ms_seqset **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    std::unique_ptr<ms_seqset> s;
    int rc = seqset_common(offsets, n_seqs, s);
    if (rc) return rc;
    if (s->n_bases > 0 && !bases) { set_error("bases is NULL"); return MS_ERR_INVALID; }
    DeviceCtx *c;
    if ((rc = get_ctx(s->device, &c))) return rc;
    ms_seqset *raw = s.release();
    auto fail = [&](int code) { ms_seqset_free(raw); return code; };
    if ((rc = seqset_alloc_packed(raw))) return fail(rc);
    {
        void *blk = nullptr;
        if ((rc = pool_alloc(c, (size_t) raw->n_bases + 64, &blk, &raw->ascii_bytes))) return fail(rc);
        raw->d_ascii = static_cast<uint8_t *>(blk);
    }
    if (raw->n_bases > 0) {
        hipError_t e = hipMemcpyAsync(raw->d_ascii, bases, (size_t) raw->n_bases, hipMemcpyHostToDevice, raw->up);
        if (e != hipSuccess) { set_error("H2D copy failed: %s", hipGetErrorString(e)); return fail(MS_ERR_RUNTIME); }
    }
    if ((rc = launch_pack(raw->d_ascii, raw->n_bases, raw->d_codes, raw->d_nmask, raw->up))) return fail(rc);
    if ((rc = launch_blk2reg(raw->d_offsets, raw->R, raw->n_bases, raw->d_blk2reg, raw->d_blkinfo, raw->up))) return fail(rc);
    hipError_t e = hipStreamSynchronize(raw->up);
    if (e != hipSuccess) { set_error("upload / pack failed: %s", hipGetErrorString(e)); return fail(MS_ERR_RUNTIME); }
    if (!keep_ascii) { pool_free(c, raw->d_ascii, raw->ascii_bytes); raw->d_ascii = nullptr; raw->ascii_bytes = 0; }
    raw->built = true;
    *out = raw;
    return MS_OK;
}

// convert_seq on HOST threads (ms_hostpack.cpp): the packed codes, the mask and the region hints are made in pinned staging memory by
// n_threads threads and cross the link on the copy engines -- no kernel is launched, so nothing of the set's construction waits for CUs
// a running scan holds (the batch stream's upload stage, MS_STREAM_HOST_PACK).  The set is identical to ms_seqset_create's.
int ms_seqset_create_hostpacked(const char *bases, const int64_t *offsets, int64_t n_seqs, int n_threads, ms_seqset **out) {
    return seqset_create_hostpacked(bases, offsets, n_seqs, n_threads, nullptr, nullptr, out);
}

// the host packer alone, for CPU tests (no device): codes [2 * ceil(n / 32)], nmask [ceil(n / 32)], blk2reg [(n + 63) / 64 + 1], blkinfo [4 x that]
int ms_debug_host_pack(const char *bases, const int64_t *offsets, int64_t n_seqs, uint32_t *codes, uint32_t *nmask, int32_t *blk2reg, int32_t *blkinfo) {
    if (!offsets || n_seqs < 0 || !codes || !nmask || !blk2reg || !blkinfo) { set_error("NULL argument"); return MS_ERR_INVALID; }
    const int64_t n = offsets[n_seqs];
    if (n > 0 && !bases) { set_error("bases is NULL"); return MS_ERR_INVALID; }
    host_pack_units(reinterpret_cast<const uint8_t *>(bases), n, 0, (n + 31) / 32, codes, nmask);
    host_region_hints(offsets, n_seqs, 0, (n + 63) / 64 + 1, blk2reg, blkinfo, false);
    return MS_OK;
}

// the four device arrays of a built set on the host, in ms_debug_host_pack's layout (any pointer may be NULL)
int ms_debug_seqset_planes(const ms_seqset *s, uint32_t *codes, uint32_t *nmask, int32_t *blk2reg, int32_t *blkinfo) {
    if (!s) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (!s->built || s->pack_pending || !s->block) { set_error("the set's planes are not on the device yet (packed by its first scan)"); return MS_ERR_INVALID; }
    const size_t n_units = (size_t) ((s->n_bases + 31) / 32), n_blocks = (size_t) ((s->n_bases + 63) / 64 + 1);
    MS_HIP(hipSetDevice(s->device));
    if (codes && n_units) MS_HIP(hipMemcpy(codes, s->d_codes, n_units * 8, hipMemcpyDeviceToHost));
    if (nmask && n_units) MS_HIP(hipMemcpy(nmask, s->d_nmask, n_units * 4, hipMemcpyDeviceToHost));
    if (blk2reg) MS_HIP(hipMemcpy(blk2reg, s->d_blk2reg, n_blocks * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (blkinfo) MS_HIP(hipMemcpy(blkinfo, s->d_blkinfo, n_blocks * sizeof(int4), hipMemcpyDeviceToHost));
    return MS_OK;
}

// the kPadWords words behind each of the two planes of a built set: zero, whichever way the set was made
int ms_debug_seqset_pad_words(const ms_seqset *s, uint32_t *codes_pad, uint32_t *nmask_pad) {
    if (!s || !codes_pad || !nmask_pad) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (!s->built || s->pack_pending || !s->block) { set_error("the set's planes are not on the device yet (packed by its first scan)"); return MS_ERR_INVALID; }
    static_assert(kPadWords == 16, "include/motifscan_amd_debug.h promises 16 words per plane");
    const size_t n_units = (size_t) ((s->n_bases + 31) / 32);
    MS_HIP(hipSetDevice(s->device));
    MS_HIP(hipMemcpy(codes_pad, s->d_codes + 2 * n_units, kPadWords * sizeof(uint32_t), hipMemcpyDeviceToHost));
    MS_HIP(hipMemcpy(nmask_pad, s->d_nmask + n_units, kPadWords * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MS_OK;
}

// the two planes of a built set on the host, in ms_genome_create_packed's layout (the public counterpart of ms_genome_packed_host)
int ms_seqset_packed_host(const ms_seqset *s, uint32_t *codes, uint32_t *nmask) {
    if (!s) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (!s->built || s->pack_pending || !s->block) { set_error("the set's planes are not on the device yet (packed by its first scan)"); return MS_ERR_INVALID; }
    const size_t n_units = (size_t) ((s->n_bases + 31) / 32);
    if (n_units == 0) return MS_OK;
    if (!codes || !nmask) { set_error("NULL argument"); return MS_ERR_INVALID; }
    MS_HIP(hipSetDevice(s->device));
    MS_HIP(hipMemcpy(codes, s->d_codes, n_units * 8, hipMemcpyDeviceToHost));
    MS_HIP(hipMemcpy(nmask, s->d_nmask, n_units * 4, hipMemcpyDeviceToHost));
    return MS_OK;
}

int ms_seqset_from_device(const void *d_bases, const int64_t *offsets, int64_t n_seqs, ms_seqset **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    std::unique_ptr<ms_seqset> s;
    int rc = seqset_common(offsets, n_seqs, s);
    if (rc) return rc;
    if (s->n_bases > 0 && !d_bases) { set_error("d_bases is NULL"); return MS_ERR_INVALID; }
    DeviceCtx *c;
    if ((rc = get_ctx(s->device, &c))) return rc;
    ms_seqset *raw = s.release();
    auto fail = [&](int code) { ms_seqset_free(raw); return code; };
    if ((rc = seqset_alloc_packed(raw))) return fail(rc);
    if ((rc = launch_pack(static_cast<const uint8_t *>(d_bases), raw->n_bases, raw->d_codes, raw->d_nmask, raw->up)))
        return fail(rc);
    if ((rc = launch_blk2reg(raw->d_offsets, raw->R, raw->n_bases, raw->d_blk2reg, raw->d_blkinfo, raw->up))) return fail(rc);
    hipError_t e = hipStreamSynchronize(raw->up);
    if (e != hipSuccess) { set_error("pack kernel failed: %s", hipGetErrorString(e)); return fail(MS_ERR_RUNTIME); }
    raw->built = true;
    *out = raw;
    return MS_OK;
}

int ms_seqset_repack(ms_seqset *s) {
    if (!s) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (!s->d_ascii) { set_error("sequence set was created without keep_ascii"); return MS_ERR_INVALID; }
    DeviceCtx *c;
    int rc = get_ctx(s->device, &c);
    if (rc) return rc;
    const hipStream_t up = c->stream_up;
    // (the region hints stay as they are: a handle's offsets are written when it is created and never again, and blk2reg_kernel's output follows
    // from them alone -- a set whose hints are still to be made, pack_pending, gets them from its first scan as before)
    if ((rc = launch_pack(s->d_ascii, s->n_bases, s->d_codes, s->d_nmask, up))) return rc;
    MS_HIP(hipStreamSynchronize(up));
    return MS_OK;
}

int ms_seqset_size(const ms_seqset *s, int64_t *n_seqs, int64_t *n_bases) {
    if (!s) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (n_seqs) *n_seqs = s->R;
    if (n_bases) *n_bases = s->n_bases;
    return MS_OK;
}

void ms_seqset_free(ms_seqset *s) {
    if (!s) return;
    (void) hipSetDevice(s->device);
    // a set freed on an ERROR path of its construction may still have its memsets / upload / pack kernel queued on the upload
    // stream: the blocks must not go back to the pool (another thread can take them at once) before that work is done.
    // A set that was built (built: its stream was synchronised then) needs no wait -- the stream is shared, waiting would stall
    // behind the NEXT batch's upload.
    if (!s->built && s->up) (void) hipStreamSynchronize(s->up);
    DeviceCtx *c = nullptr;
    const bool have = get_ctx(s->device, &c) == MS_OK;
    if (s->d_ascii) { if (have) pool_free(c, s->d_ascii, s->ascii_bytes); else (void) hipFree(s->d_ascii); }
    if (s->block) { if (have) pool_free(c, s->block, s->block_bytes); else (void) hipFree(s->block); }
    if (s->h_off_pin) pinned_free(s->h_off_pin, s->h_off_pin_bytes);
    delete s;
}

// ------------------------------------------------------------------- resident genome --

// A genome is a sequence set whose "sequences" are the chromosomes, kept packed in HBM
// (3 Gbp = 1.1 GB); regions are then cut out on the device with no ASCII traffic at all.
int ms_genome_create(const char *bases, const int64_t *chrom_offsets, int32_t n_chroms, ms_genome **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    ms_seqset *s = nullptr;
    int rc = ms_seqset_create(bases, chrom_offsets, n_chroms, 0, &s);
    if (rc) return rc;
    *out = reinterpret_cast<ms_genome *>(s);
    return MS_OK;
}

// convert_seq (cscore.c:81-114) into the packed layout on HOST threads, no device: what the genome-file builder runs (ms_hostpack.cpp)
int ms_pack_bases_host(const char *bases, int64_t n_bases, int n_threads, uint32_t *codes, uint32_t *nmask) {
    if (n_bases < 0 || (n_bases > 0 && (!bases || !codes || !nmask))) { set_error("NULL argument"); return MS_ERR_INVALID; }
    const int64_t n_units = (n_bases + 31) / 32;
    const int T = (int) std::max<int64_t>(1, std::min<int64_t>(std::min(n_threads < 1 ? 1 : n_threads, 64), n_units / 4096));
    auto work = [&](int t) { host_pack_units(reinterpret_cast<const uint8_t *>(bases), n_bases, n_units * t / T, n_units * (t + 1) / T, codes, nmask); };
    std::vector<std::thread> th;
    try { for (int t = 1; t < T; t++) th.emplace_back(work, t); }
    catch (const std::exception &) { for (auto &x : th) x.join(); set_error("could not start packing threads"); return MS_ERR_RUNTIME; }
    work(0);
    for (auto &x : th) x.join();
    return MS_OK;
}

// A genome from its PACKED form (a genome file made once: motifscan_amd/genome.py): the two planes cross the link as they are -- 0.375 B per
// base, no ASCII, no pack kernel; only the region hints are made on the device.  The planes are validated first (a file is outside input):
// a non-ACGT base must hold code 0 and nothing may be set past the last base -- the invariants pack_kernel guarantees and the scan kernels rely on.
int ms_genome_create_packed(const uint32_t *codes, const uint32_t *nmask, const int64_t *chrom_offsets, int32_t n_chroms, ms_genome **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    std::unique_ptr<ms_seqset> s;
    int rc = seqset_common(chrom_offsets, n_chroms, s);
    if (rc) return rc;
    const int64_t n_bases = s->n_bases, n_units = (n_bases + 31) / 32;
    if (n_bases > 0 && (!codes || !nmask)) { set_error("codes / nmask is NULL"); return MS_ERR_INVALID; }
    {
        int64_t cbad[kMaxChunks];
        for (int t = 0; t < kMaxChunks; t++) cbad[t] = -1;
        parallel_chunks(n_units, [&](int t, int64_t b, int64_t e) {
            for (int64_t u = b; u < e; u++) {
                const uint64_t cw = (uint64_t) codes[2 * u] | ((uint64_t) codes[2 * u + 1] << 32);
                uint64_t nw = nmask[u], spread = 0;                      // bit i of the mask -> bits 2i, 2i + 1
                for (int i = 0; nw; i++, nw >>= 1) if (nw & 1u) spread |= 3ULL << (2 * i);
                uint64_t tail_c = 0;
                uint32_t tail_n = 0;
                if (32 * (u + 1) > n_bases) {
                    const int valid = (int) (n_bases - 32 * u);
                    tail_c = valid >= 32 ? 0 : ~0ULL << (2 * valid);
                    tail_n = valid >= 32 ? 0 : ~0u << valid;
                }
                if ((cw & spread) || (cw & tail_c) || (nmask[u] & tail_n)) { cbad[t] = u; return; }
            }
        });
        for (int t = 0; t < kMaxChunks; t++)
            if (cbad[t] >= 0) { set_error("packed genome is corrupt at bases %lld..%lld: a non-ACGT base with a non-zero code, or bits past the end", (long long) (32 * cbad[t]), (long long) (32 * cbad[t] + 31)); return MS_ERR_INVALID; }
    }
    DeviceCtx *c;
    if ((rc = get_ctx(s->device, &c))) return rc;
    ms_seqset *raw = s.release();
    auto fail = [&](int code) { ms_seqset_free(raw); return code; };
    if ((rc = seqset_alloc_packed(raw))) return fail(rc);
    if (n_units > 0) {
        hipError_t e = hipMemcpyAsync(raw->d_codes, codes, (size_t) n_units * 8, hipMemcpyHostToDevice, raw->up);
        if (e == hipSuccess) e = hipMemcpyAsync(raw->d_nmask, nmask, (size_t) n_units * 4, hipMemcpyHostToDevice, raw->up);
        if (e != hipSuccess) { set_error("H2D copy of the packed genome failed: %s", hipGetErrorString(e)); return fail(MS_ERR_RUNTIME); }
    }
    if ((rc = launch_blk2reg(raw->d_offsets, raw->R, raw->n_bases, raw->d_blk2reg, raw->d_blkinfo, raw->up))) return fail(rc);
    hipError_t e = hipStreamSynchronize(raw->up);
    if (e != hipSuccess) { set_error("upload of the packed genome failed: %s", hipGetErrorString(e)); return fail(MS_ERR_RUNTIME); }
    raw->built = true;
    *out = reinterpret_cast<ms_genome *>(raw);
    return MS_OK;
}

// ... and back: the two planes of a resident genome on the host (to write the genome file after a genome was packed on the device)
int ms_genome_packed_host(const ms_genome *g, uint32_t *codes, uint32_t *nmask) {
    if (!g || !codes || !nmask) { set_error("NULL argument"); return MS_ERR_INVALID; }
    const ms_seqset *s = reinterpret_cast<const ms_seqset *>(g);
    const size_t n_units = (size_t) ((s->n_bases + 31) / 32);
    if (n_units == 0) return MS_OK;
    MS_HIP(hipSetDevice(s->device));
    MS_HIP(hipMemcpy(codes, s->d_codes, n_units * 8, hipMemcpyDeviceToHost));
    MS_HIP(hipMemcpy(nmask, s->d_nmask, n_units * 4, hipMemcpyDeviceToHost));
    return MS_OK;
}

int ms_genome_size(const ms_genome *g, int32_t *n_chroms, int64_t *n_bases) {
    if (!g) { set_error("NULL argument"); return MS_ERR_INVALID; }
    const ms_seqset *s = reinterpret_cast<const ms_seqset *>(g);
    if (n_chroms) *n_chroms = (int32_t) s->R;
    if (n_bases) *n_bases = s->n_bases;
    return MS_OK;
}

void ms_genome_free(ms_genome *g) { ms_seqset_free(reinterpret_cast<ms_seqset *>(g)); }

int ms_seqset_from_genome(const ms_genome *g, const int32_t *chrom, const int64_t *start, const int64_t *end,
                          int64_t n_regions, ms_seqset **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    if (!g) { set_error("NULL genome"); return MS_ERR_INVALID; }
    if (n_regions < 0 || (n_regions > 0 && (!chrom || !start || !end))) { set_error("bad region arrays"); return MS_ERR_INVALID; }
    const ms_seqset *G = reinterpret_cast<const ms_seqset *>(g);
    std::vector<int64_t> dst, src;
    try { dst.resize((size_t) n_regions + 1); src.resize((size_t) n_regions + 1); }
    catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    // pass 1 (threads): validate, source position and length of every region, per-chunk totals
    int64_t csum[kMaxChunks], cbad[kMaxChunks];
    for (int t = 0; t < kMaxChunks; t++) { csum[t] = 0; cbad[t] = -1; }
    const int64_t n_chroms = G->R;
    const int64_t *goff = G->offsets.data();
    parallel_chunks(n_regions, [&](int t, int64_t b, int64_t e) {
        int64_t sum = 0, bad = -1;
        for (int64_t r = b; r < e; r++) {
            const int64_t ch = chrom[r];
            bool ok = ch >= 0 && ch < n_chroms;
            if (ok) {
                const int64_t clen = goff[ch + 1] - goff[ch];
                ok = start[r] >= 0 && end[r] >= start[r] && end[r] <= clen;
            }
            if (!ok) { if (bad < 0) bad = r; continue; }
            src[(size_t) r] = goff[ch] + start[r];
            dst[(size_t) r + 1] = end[r] - start[r];          // length for now
            sum += end[r] - start[r];
        }
        csum[t] = sum; cbad[t] = bad;
    });
    for (int t = 0; t < kMaxChunks; t++)
        if (cbad[t] >= 0) {
            const int64_t r = cbad[t];
            if (chrom[r] < 0 || chrom[r] >= n_chroms) set_error("region %lld: chromosome index %d out of range", (long long) r, chrom[r]);
            else set_error("region %lld: [%lld, %lld) is outside chromosome %d of length %lld", (long long) r, (long long) start[r],
                           (long long) end[r], chrom[r], (long long) (goff[chrom[r] + 1] - goff[chrom[r]]));
            return MS_ERR_INVALID;
        }
    // pass 2 (threads): lengths -> offsets, every chunk starting at the sum of the chunks before it
    int64_t cbase[kMaxChunks + 1];
    cbase[0] = 0;
    for (int t = 0; t < kMaxChunks; t++) cbase[t + 1] = cbase[t] + csum[t];
    dst[0] = 0;
    parallel_chunks(n_regions, [&](int t, int64_t b, int64_t e) {
        int64_t run = cbase[t];
        for (int64_t r = b; r < e; r++) { run += dst[(size_t) r + 1]; dst[(size_t) r + 1] = run; }
    });
    src[(size_t) n_regions] = 0;
    const int prev_dev = current_device();
    set_current_device(G->device);                            // the new set lives next to its genome
    std::unique_ptr<ms_seqset> s;
    int rc = seqset_common(dst.data(), n_regions, s, &dst);
    set_current_device(prev_dev);
    if (rc) return rc;
    DeviceCtx *c;
    if ((rc = get_ctx(G->device, &c))) return rc;
    ms_seqset *raw = s.release();
    auto fail = [&](int code) { ms_seqset_free(raw); return code; };
    if ((rc = seqset_alloc_packed(raw))) return fail(rc);
    int64_t *d_src = nullptr;
    if ((rc = dev_alloc(&d_src, (size_t) n_regions + 1))) return fail(rc);
    hipError_t he = hipMemcpyAsync(d_src, src.data(), ((size_t) n_regions + 1) * sizeof(int64_t), hipMemcpyHostToDevice, raw->up);
    if (he == hipSuccess) {
        rc = launch_extract(G->d_codes, G->d_nmask, d_src, raw->d_offsets, raw->R, raw->n_bases, raw->d_codes, raw->d_nmask, raw->up);
        if (!rc) rc = launch_blk2reg(raw->d_offsets, raw->R, raw->n_bases, raw->d_blk2reg, raw->d_blkinfo, raw->up);
        if (!rc) he = hipStreamSynchronize(raw->up);
    }
    dev_free(d_src);
    if (rc) return fail(rc);
    if (he != hipSuccess) { set_error("extraction failed: %s", hipGetErrorString(he)); return fail(MS_ERR_RUNTIME); }
    raw->built = true;
    *out = raw;
    return MS_OK;
}

}  // extern "C"
