// ms_scorehist.hip -- the score distribution of every window (ms_scan_score_histogram): per motif, the exact count of windows per score
// bin over a whole sequence set.  The exhaustive form of what `motif --build` samples (c_score of 10^6 random windows, cscore.c:174-229,
// sorted and read at a few ranks, motif/__init__.py:378-401): integer counting, so the bytes are the same on every run and the result is
// additive over regions, chromosomes and ranks (one all-reduce(sum)).
//
// Scoring.  For motif m of width W and region r of length L the windows pos = 0 .. L - W are scored exactly as ms_scan scores them
// (cscore.c:336-390; the scorer of ms_fp64.hip and ms_best.hip: columns 0 .. W - 1, forward M[b][c], reverse M[3 - b][W - 1 - c] at the
// same step, +0.0 for a base that adds nothing, raw / max_raw as ONE IEEE divide).  Without MS_HIST_PER_POSITION every (window, strand of
// the mask) is one count; with it a window is one count of (fwd > rev ? fwd : rev) / max_raw -- c_score (cscore.c:207-223) at every
// position -- selected on the RAW sums, then one divide.
//
// The bin rule (the definition; the Python layer restates it with numpy's correctly rounded operations): d = score - lo[m] (one rounded
// subtraction), t = d * inv_width[m] (one rounded multiply); t < 0 -> slot 0 ("below", -inf included), t >= n_bins -> slot n_bins + 1
// ("above"), else slot 1 + (int) floor(t).
//
// Divide only where it matters.  x -> x / max_raw (max_raw > 0), x -> x - lo and x -> x * inv_width (inv_width > 0) are each monotone
// non-decreasing under round-to-nearest, so t is a monotone non-decreasing function of the raw sum.  The host therefore finds, per motif, by
// bisection over the ordered bit patterns of all doubles and with the SAME three operations,
//     raw_lo = the least double whose t >= 0          raw_hi = the least double whose t >= n_bins
// (both exist: t(+inf) = +inf, t(-inf) = -inf).  Then raw < raw_lo is EXACTLY "below" and raw >= raw_hi EXACTLY "above", whatever the
// roundings in between did -- this is ms_scan_best's "divide only when the raw sum improves" argument (ms_best.hip) with two fixed
// thresholds in place of the running best.  Only a window between the two pays the divide, the subtraction and the multiply, and its
// slot is inside [1, n_bins] by the same monotonicity.  For a tail histogram (lo = 0.7, say) almost every window is "below" and costs two
// compares.  A scorable motif (scorable(), ms_best_dev.h) has no NaN or +inf entry and a finite max_raw > 0, so no raw sum is NaN and
// every counted window lands in exactly one slot; an unscorable motif is never scored and keeps its all-zero row.
//
// Mapping (best_kernel's, ms_best.hip, with the reduction replaced).  A region is cut into SEGMENTS of kHistSegWindows window starts; a
// block owns one TILE of motifs -- consecutive scorable motifs whose tab2 entries are consecutive in HBM and fit kHistTileEntries, staged in
// LDS with one contiguous copy behind an all-zero entry 0 -- and kHistBlockSegs consecutive segments, whose (region start, length, first
// window) it looks up ONCE into LDS.  Per motif of the tile the block clears an LDS histogram of n_bins + 2 32-bit counters, every wave
// walks its kHistSegsPerWave segments (a lane takes 64-window strips: one code word, one mask word, W column reads of 16 bytes from LDS
// and 2 W fp64 adds per window), and the block then adds the non-zero counters to the motif's int64 row with no-return 64-bit global
// atomic adds.  "Below" and "above" never touch an LDS atomic in the walk: they are counted per wave with ballot + popcount in scalar
// registers and added to their two slots once per (wave, motif) -- for a tail histogram every lane of a wave would hit the same
// LDS address.  The histogram being per motif, the segment loop sits INSIDE the motif loop, so a lane reads a strip's two words again for
// every motif (20 bytes from L2 -- the block's segments are 24 KB of planes -- against W LDS reads and 2 W adds): keeping the words of
// kHistSegsPerWave segments in registers, as best_kernel keeps one segment's, would take 192 VGPRs.
//
// The flush bound.  Per (block, motif) the clear and the flush touch at most n_bins + 2 <= 4098 counters with 512 threads: <= 9 LDS
// writes, 9 LDS reads and <= 9 atomics a thread, and two barriers.  Between two flushes the block scores up to kHistBlockSegs x
// kHistSegWindows = 65536 window starts = 128 a thread, each W >= 1 LDS reads + 2 W adds: for the shortest motifs of the benchmark set
// (W = 5) 640 column steps against <= 27 counter operations, 4 %; for one-column motifs and 4096 bins of which all are hit, 21 %
// (a histogram of fewer hit bins skips the zero counters).  A counter is at most 2 strands x 65536 = 2^17 < 2^32.
//
// max_n >= 0 drops a window with more than max_n non-ACGT bases among its OWN W bases (bits of the nmask plane, IUPAC letters included;
// not the reference's filter, which counts N / n only and on the widest motif's window): popcount(mask word & low_mask(W)) from the
// register for W <= 32, plus the further words a wider motif loads anyway.
//
// Motifs wider than kHistTileMaxW read their table from HBM (score_window), one motif per "tile" (the <false> form).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "ms_best_dev.h"
#include "ms_device.h"
#include "ms_handles.h"

namespace ms {

namespace {

constexpr int kHistThreads = 512;
constexpr int kHistWaves = kHistThreads / 64;
constexpr int kHistStrips = 8;                           // strips of 64 window starts per segment
constexpr int kHistSegWindows = 64 * kHistStrips;
constexpr int kHistSegsPerWave = 16;                     // segments a wave counts between two flushes
constexpr int kHistBlockSegs = kHistWaves * kHistSegsPerWave;
constexpr int kHistTileMaxW = 928;                       // widest motif whose table is staged in LDS
constexpr int kHistTileEntries = kHistTileMaxW * 4;      // 58 KB of tab2 entries per tile (+ the zero entry) + 16 KB of counters + 3 KB of segments: two blocks share a CU's 160 KB
constexpr int kHistSlots = MS_SCOREHIST_MAX_BINS + 2;
constexpr DenseGeom kHistGeom = {kHistSegWindows, kHistTileMaxW, kHistTileEntries, false};      // what the host plans with: counts are added, no partials

struct HistSeg {                                         // a segment of the block: its region's first base and length, its first window start
    int64_t beg, len, p0;
};
constexpr size_t kHistSegBytes = sizeof(HistSeg) * kHistBlockSegs;

__host__ __device__ constexpr size_t hist_counter_bytes(int n_bins) { return ((size_t) (n_bins + 2) * 4 + 15) & ~(size_t) 15; }

struct HistArgs {
    const uint32_t *codes, *nmask;
    const int64_t *offsets;                              // [R + 1]
    int64_t R;
    const int64_t *seg_first;                            // [R + 1] first segment of the region; nullptr: one segment per region
    int64_t n_seg;
    const int32_t *tile_first;                           // [tiles + 1] into mot
    const int32_t *mot;                                  // the scorable motifs, tile after tile
    DevPwm Pw;
    const double *bins;                                  // [P][4] lo, inv_width, raw_lo, raw_hi
    int strand_mask;
    int per_position;
    int32_t n_bins;
    int32_t max_n;
    unsigned long long *out;                             // [P][n_bins + 2]
};

// grid = (ceil(segments / kHistBlockSegs), tiles).  LDS: [segments][counters][the tile's tables]; !LDS: one motif per tile, its table in HBM.
template <bool LDS>
__global__ void __launch_bounds__(kHistThreads, 4) scorehist_kernel(const HistArgs A, int32_t tile0) {
    extern __shared__ double2 hist_lds[];
    HistSeg *__restrict__ segs = reinterpret_cast<HistSeg *>(hist_lds);
    unsigned int *__restrict__ cnt = reinterpret_cast<unsigned int *>(reinterpret_cast<char *>(hist_lds) + kHistSegBytes);
    const double2 *__restrict__ tab_lds = reinterpret_cast<const double2 *>(reinterpret_cast<char *>(hist_lds) + kHistSegBytes + hist_counter_bytes(A.n_bins));
    const int32_t tile = tile0 + (int32_t) blockIdx.y;
    const int32_t k0 = A.tile_first[tile], k1 = A.tile_first[tile + 1];
    const int64_t tab0 = A.Pw.tab_off[A.mot[k0]];
    const int64_t s0 = (int64_t) blockIdx.x * kHistBlockSegs;
    const int n_here = (int) (A.n_seg - s0 < kHistBlockSegs ? A.n_seg - s0 : kHistBlockSegs);    // >= 1 by the grid
    if (LDS) {
        const int32_t ml = A.mot[k1 - 1];
        const int32_t n = (int32_t) (A.Pw.tab_off[ml] - tab0) + A.Pw.width[ml] * 4;
        const double2 *__restrict__ src = A.Pw.tab2 + tab0;
        double2 *__restrict__ dst = const_cast<double2 *>(tab_lds);
        if (threadIdx.x == 0) dst[0] = make_double2(0.0, 0.0);
        for (int32_t i = threadIdx.x; i < n; i += kHistThreads) dst[1 + i] = src[i];
    }
    if ((int) threadIdx.x < n_here) {
        const int64_t seg = s0 + threadIdx.x;
        const int64_t r = A.seg_first ? find_region_bsearch(A.seg_first, A.R, seg) : seg;
        HistSeg h;
        h.beg = A.offsets[r];
        h.len = A.offsets[r + 1] - h.beg;
        h.p0 = (A.seg_first ? seg - A.seg_first[r] : 0) * kHistSegWindows;
        segs[threadIdx.x] = h;
    }
    const int wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const int lane = (int) (threadIdx.x & 63u);
    const int n_slots = A.n_bins + 2;
    const bool both = A.strand_mask == 3;

    for (int32_t k = k0; k < k1; k++) {
        const int32_t m = A.mot[k];
        const int W = A.Pw.width[m];
        const double max_raw = A.Pw.max_raw[m];
        const int64_t tab_m = A.Pw.tab_off[m];
        const uint32_t tb = 1u + (uint32_t) (tab_m - tab0);
        const double lo = A.bins[4 * (int64_t) m], inv = A.bins[4 * (int64_t) m + 1], raw_lo = A.bins[4 * (int64_t) m + 2], raw_hi = A.bins[4 * (int64_t) m + 3];
        for (int i = threadIdx.x; i < n_slots; i += kHistThreads) cnt[i] = 0u;
        __syncthreads();                                  // (the first trip: the tile and the segments are staged too)
        uint32_t below = 0, above = 0;                    // of the wave: the same value in every lane
        // one count: wave-uniform control flow up to the LDS atomic, so that the ballots see every lane
        auto count = [&](bool counted, double raw) {
            const bool is_below = counted && raw < raw_lo, is_above = counted && raw >= raw_hi;
            below += (uint32_t) __popcll(__ballot(is_below));
            above += (uint32_t) __popcll(__ballot(is_above));
            if (counted && !is_below && !is_above) {
                const double q = raw / max_raw;
                const double d = q - lo;
                const double t = d * inv;
                int bin = (int) t;                        // 0 <= t < n_bins by the thresholds: truncation is floor
                bin = bin < 0 ? 0 : (bin >= A.n_bins ? A.n_bins - 1 : bin);      // (never taken; keeps the LDS write inside the counters whatever happens)
                atomicAdd(&cnt[1 + bin], 1u);
            }
        };
#pragma unroll 1
        for (int sw = wave; sw < n_here; sw += kHistWaves) {
            const HistSeg h = segs[sw];
            const int64_t last = h.len - W;               // the region's last window start
#pragma unroll 1
            for (int s = 0; s < kHistStrips; s++) {
                if (h.p0 + s * 64 > last) break;          // (wave-uniform) no window of this strip, or of a later one, fits the region
                const int64_t pos = h.p0 + s * 64 + lane;
                const bool valid = pos <= last;
                double fwd = 0.0, rev = 0.0;
                int n_non = 0;
                if (LDS) {
                    const uint64_t cws = valid ? code_window(A.codes, h.beg + pos) : 0ULL;
                    const uint32_t nws = valid ? n_window(A.nmask, h.beg + pos) : ~0u;
                    const int n0 = W < 32 ? W : 32;
                    best_cols32(tab_lds, tb, n0, cws, nws | ~low_mask(n0), fwd, rev);
                    n_non = __popc(nws & low_mask(n0));
                    for (int c0 = 32; c0 < W; c0 += 32) { // wider motifs: the further words (a lane without a window reads nothing)
                        const int n = (W - c0) < 32 ? (W - c0) : 32;
                        const uint64_t cwx = valid ? code_window(A.codes, h.beg + pos + c0) : 0ULL;
                        const uint32_t nwx = valid ? n_window(A.nmask, h.beg + pos + c0) : ~0u;
                        best_cols32(tab_lds, tb + (uint32_t) c0 * 4u, n, cwx, nwx | ~low_mask(n), fwd, rev);
                        n_non += __popc(nwx & low_mask(n));
                    }
                } else if (valid) {
                    DevSeq S;
                    S.codes = A.codes; S.nmask = A.nmask;
                    score_window(S, A.Pw.tab2 + tab_m, W, h.beg + pos, fwd, rev);
                    if (A.max_n >= 0)
                        for (int c0 = 0; c0 < W; c0 += 32) n_non += __popc(n_window(A.nmask, h.beg + pos + c0) & low_mask((W - c0) < 32 ? (W - c0) : 32));
                }
                const bool counted = valid && (A.max_n < 0 || n_non <= A.max_n);
                if (A.per_position) {
                    count(counted, both ? (fwd > rev ? fwd : rev) : ((A.strand_mask & 1) ? fwd : rev));
                } else {
                    if (A.strand_mask & 1) count(counted, fwd);
                    if (A.strand_mask & 2) count(counted, rev);
                }
            }
        }
        if (lane == 0) {
            if (below) atomicAdd(&cnt[0], below);
            if (above) atomicAdd(&cnt[n_slots - 1], above);
        }
        __syncthreads();
        // the flush: the thread that reads counter i here is the one that clears it for the next motif
        unsigned long long *__restrict__ row = A.out + (int64_t) m * n_slots;
        for (int i = threadIdx.x; i < n_slots; i += kHistThreads) {
            const unsigned int c = cnt[i];
            if (c) atomicAdd(&row[i], (unsigned long long) c);
        }
    }
}


// the ordered bit pattern of a double: a < b <=> key(a) < key(b) for all non-NaN doubles (-0.0 just below +0.0)
uint64_t ord_key(double x) {
    uint64_t u;
    std::memcpy(&u, &x, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
double ord_val(uint64_t k) {
    const uint64_t u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    double x;
    std::memcpy(&x, &u, 8);
    return x;
}

// the least double raw with ((raw / max_raw) - lo) * inv >= bound (the header comment: the three roundings are monotone)
double raw_threshold(double max_raw, double lo, double inv, double bound) {
    auto at_least = [&](double raw) {
        volatile double q = raw / max_raw;                // (volatile: each operation rounded to double on its own, as on the device)
        volatile double d = q - lo;
        volatile double t = d * inv;
        return t >= bound;
    };
    const double inf = std::numeric_limits<double>::infinity();
    uint64_t a = ord_key(-inf), b = ord_key(inf);         // at_least(-inf) is false, at_least(+inf) is true
    while (b - a > 1) {
        const uint64_t mid = a + (b - a) / 2;
        if (at_least(ord_val(mid))) b = mid; else a = mid;
    }
    return ord_val(b);
}

}  // namespace

}  // namespace ms

using namespace ms;

extern "C" {

int ms_debug_scorehist_dims(int32_t out[4]) {
    if (!out) { set_error("NULL argument"); return MS_ERR_INVALID; }
    out[0] = kHistSegWindows;
    out[1] = kHistTileMaxW;
    out[2] = kHistSlots;
    out[3] = kHistBlockSegs * kHistSegWindows;
    return MS_OK;
}

int ms_scan_score_histogram(const ms_pwmset *pwms_c, const ms_seqset *seqs, int strand_mask, uint32_t flags, const double *lo, const double *inv_width,
                            int32_t n_bins, int32_t max_n, int64_t *out, double *device_ms) {
    if (!require_device()) return MS_ERR_RUNTIME;
    if (device_ms) *device_ms = 0.0;
    if (!pwms_c || !seqs) { set_error("NULL handle"); return MS_ERR_INVALID; }
    if (strand_mask < 1 || strand_mask > 3) { set_error("invalid strand mask %d (1 '+', 2 '-', 3 both)", strand_mask); return MS_ERR_INVALID; }
    if (flags & ~MS_HIST_PER_POSITION) { set_error("unknown score-histogram flags 0x%x", flags); return MS_ERR_INVALID; }
    if (n_bins < 1 || n_bins > MS_SCOREHIST_MAX_BINS) { set_error("n_bins must be in [1, %d]", MS_SCOREHIST_MAX_BINS); return MS_ERR_INVALID; }
    ms_pwmset *pwms = const_cast<ms_pwmset *>(pwms_c);
    const int32_t P = pwms->P;
    const int64_t R = seqs->R;
    if (P == 0) return MS_OK;                          // no row to fill
    if (!lo || !inv_width || !out) { set_error("NULL array"); return MS_ERR_INVALID; }
    for (int32_t m = 0; m < P; m++) {
        if (!std::isfinite(lo[m])) { set_error("lo[%d] is not finite", m); return MS_ERR_INVALID; }
        if (!(std::isfinite(inv_width[m]) && inv_width[m] > 0.0)) { set_error("inv_width[%d] is not a finite number > 0", m); return MS_ERR_INVALID; }
    }
    hipPointerAttribute_t attr;
    std::memset(&attr, 0, sizeof(attr));
    const bool out_on_device = hipPointerGetAttributes(&attr, out) == hipSuccess && attr.type == hipMemoryTypeDevice;
    (void) hipGetLastError();                          // a pageable host pointer is "not found" here, which is no error
    if (out_on_device && attr.device != seqs->device) { set_error("output lives on device %d, the sequence set on device %d", attr.device, seqs->device); return MS_ERR_INVALID; }
    const int n_slots = n_bins + 2;
    const size_t out_bytes = 8 * (size_t) P * (size_t) n_slots;
    DeviceCtx *c;
    int rc = get_ctx(seqs->device, &c);
    if (rc) return rc;

    // ---- the plan, on the host: segments of the regions, tiles of the motifs (ms_dense_plan.h), the raw-space thresholds
    DensePlan plan;
    if ((rc = dense_plan_for(kHistGeom, pwms, seqs, kHistBlockSegs, [&](int32_t m) { return scorable(pwms, m); }, &plan))) return rc;
    plan.skipped.clear();                              // (their rows stay as cleared: nothing of them goes to the device)
    std::vector<double> bins;
    try {
        bins.assign(4 * (size_t) P, 0.0);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    for (const int32_t m : plan.mot) {
        bins[4 * (size_t) m] = lo[m];
        bins[4 * (size_t) m + 1] = inv_width[m];
        bins[4 * (size_t) m + 2] = raw_threshold(pwms->max_raw[(size_t) m], lo[m], inv_width[m], 0.0);
        bins[4 * (size_t) m + 3] = raw_threshold(pwms->max_raw[(size_t) m], lo[m], inv_width[m], (double) n_bins);
    }

    std::lock_guard<std::mutex> lk_dev(c->mu);
    std::lock_guard<std::mutex> lk_pwm(pwms->mu);
    MS_HIP(hipSetDevice(c->device));
    Carve cv;
    const DenseSlots ds = dense_slots(cv, plan);
    const auto s_bins = cv.add<double>(bins.size());
    const auto s_out = cv.add<unsigned long long>(out_on_device ? 0 : (size_t) P * (size_t) n_slots);
    const hipStream_t st = c->stream;
    WorkBlock work;                                    // (behind the locks: it goes back behind a wait for the stream, whichever way this returns)
    if ((rc = work.alloc(c, st, cv.bytes()))) return rc;
    void *const wblk = work.p;
    double *d_bins = Carve::at(wblk, s_bins);
    unsigned long long *d_out = out_on_device ? reinterpret_cast<unsigned long long *>(out) : Carve::at(wblk, s_out);

    hipError_t he = hipMemsetAsync(d_out, 0, out_bytes, st);
    if (he != hipSuccess) return hip_rc(he, "clearing the histogram");
    float ms01 = 0;
    const bool walk = R > 0 && !plan.mot.empty();
    if (walk) {
        if ((rc = pwmset_upload(pwms, c->device, st))) return rc;
        if ((rc = seqset_pack_pending(seqs, st))) return rc;
        const size_t lds_fixed = kHistSegBytes + hist_counter_bytes(n_bins), lds = lds_fixed + (plan.max_tile + 1) * sizeof(double2);
        if ((rc = dense_raise_lds(c, reinterpret_cast<const void *>(scorehist_kernel<true>), lds,
                                  kHistSegBytes + hist_counter_bytes(MS_SCOREHIST_MAX_BINS) + (kHistTileEntries + 1) * sizeof(double2))))
            return rc;
        DenseDev d;
        if ((rc = dense_upload(plan, ds, wblk, st, &d))) return rc;
        he = hipMemcpyAsync(d_bins, bins.data(), 8 * bins.size(), hipMemcpyHostToDevice, st);
        if (he != hipSuccess) return hip_rc(he, "upload of the plan");

        HistArgs A;
        A.codes = seqs->d_codes; A.nmask = seqs->d_nmask; A.offsets = seqs->d_offsets; A.R = R;
        A.seg_first = d.seg_first;
        A.n_seg = plan.n_seg;
        A.tile_first = d.tile_first; A.mot = d.mot;
        A.Pw = dev_pwm(pwms);
        A.bins = d_bins;
        A.strand_mask = strand_mask;
        A.per_position = (flags & MS_HIST_PER_POSITION) ? 1 : 0;
        A.n_bins = n_bins;
        A.max_n = max_n;
        A.out = d_out;
        HistArgs Aw = A;                                 // the wide motifs: one "tile" each
        Aw.tile_first = d.wide_first;

        (void) hipEventRecord(c->ev[0], st);
        const unsigned gx = (unsigned) ((plan.n_seg + kHistBlockSegs - 1) / kHistBlockSegs);
        rc = dense_chunks((int64_t) plan.tile_first.size() - 1, "score-histogram kernel", [&](int64_t t0, unsigned ny) {
            hipLaunchKernelGGL(scorehist_kernel<true>, dim3(gx, ny), dim3(kHistThreads), lds, st, A, (int32_t) t0);
        });
        if (!rc) rc = dense_chunks((int64_t) plan.wide_first.size() - 1, "score-histogram kernel (tables in HBM)", [&](int64_t t0, unsigned ny) {
            hipLaunchKernelGGL(scorehist_kernel<false>, dim3(gx, ny), dim3(kHistThreads), lds_fixed, st, Aw, (int32_t) t0);
        });
        if (rc) return rc;
        (void) hipEventRecord(c->ev[1], st);
    }
    if (!out_on_device) {
        he = hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st);
        if (he != hipSuccess) return hip_rc(he, "copy of the histogram");
    }
    if ((rc = work.wait("score histogram"))) return rc;
    if (walk) (void) hipEventElapsedTime(&ms01, c->ev[0], c->ev[1]);
    if (device_ms) *device_ms = ms01;
    return MS_OK;
}

}  // extern "C"
