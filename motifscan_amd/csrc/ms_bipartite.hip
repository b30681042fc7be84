// ms_bipartite.hip -- the best site of every (bipartite spec, region) cell (ms_scan_best_bipartite): two half-sites of a PWM set, a
// spacer of g_min .. g_max bases between them, a fixed relative orientation; ms_scan_best's dense walk, exact, into the same ms_best
// handle with a fourth plane, the winner's gap.  include/motifscan_amd.h has the definition, operation by operation.
//
// A spec k = (a, b, flip, g_min, g_max).  With F_m(p), R_m(p) the forward and reverse raw sums of motif m at window start p exactly as
// ms_scan_best forms them, the placement (p, strand, g) has
//     '+'  raw = F_a(p) + Y(p + W_a + g),    Y  = F_b (flip 0) or R_b (flip 1)
//     '-'  raw = Y'(p) + R_a(p + W_b + g),   Y' = R_b (flip 0) or F_b (flip 1)
// and score = raw / (max_raw_a + max_raw_b).  The walk is p ascending, '+' before '-', g ascending; a placement replaces the best iff its
// score is GREATER.
//
// Mapping: ms_scan_best's (ms_best.hip).  A wave owns a segment of kBestSegWindows window starts, a block kBestWaves segments and one
// TILE of consecutive scorable specs; a lane keeps the code and mask words of its kBestStrips window starts in registers.  The host lays
// the tables out per call in spec order -- the tab2 entries of a, then those of b (bp_spec_table, ms_bipartite_plan.h) -- so dense_plan
// tiles by the pseudo-width W_a + W_b and a tile is staged with one contiguous copy behind an all-zero entry 0.
//
// Element sums.  Per spec the wave walks kBestStrips + kBpHaloStrips strips of 64 window starts in ascending order (the words of the
// halo strips are fetched per spec).  At strip t every lane forms F and R of both elements at its start p0 + 64 t + lane with the shared
// column loop (best_cols32), writes the two sums that are read SHIFTED -- Y of b and R of a -- to the wave's LDS ring, and keeps the two
// that are read in place -- F_a(p) and Y'(p) -- in registers.  A second half lies at most kBpMaxWidth + kBpMaxGap = 128 starts behind
// its first half, so once strip t is in the ring, behind a wave-level fence, the placements of strip t - 2 have every partner they can
// read: strips t - 2 .. t.  The ring therefore holds FOUR strips (index = start & 255), not the segment and its halo: 2 arrays x 256
// doubles = 4 KB a wave, 32 KB a block; with the 32 KB tile (kBpTileEntries) a block takes 64 KB and TWO blocks share a CU's 160 KB,
// 4 waves a SIMD -- the occupancy of best_kernel.  (Ten strips flat would be 80 KB a block: one block a CU whatever the tile.)  The own
// sums of the two strips in flight rotate through named registers; nothing is indexed dynamically, nothing goes to scratch.
//
// The divide, the tie rule and the reduction are ms_scan_best's (ms_best.hip's header has the argument): a lane's placements come in
// walk order, the IEEE divide is paid only where the raw sum is strictly greater than the lane's best raw sum -- division by a positive
// constant is monotone --, and the wave is reduced with wave_best over the key (pos, strand, g - g_min) (bp_key), which IS the walk's
// order inside a cell: the greater q wins, equal q goes to the smaller key.  A region of one segment writes its four planes; a longer
// one writes a BestPart and a gap per (spec, segment), best_tail folds the partials as for ms_scan_best, and bipartite_gap_kernel takes
// the winner's gap from the partial of segment pos / kBestSegWindows.  best_kernel, best_reduce_kernel and best_fill_kernel are not
// touched; the rows of unscorable specs get gap -1 from bipartite_gap_fill_kernel.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <vector>

#include "ms_best_dev.h"
#include "ms_bipartite_plan.h"
#include "ms_device.h"
#include "ms_handles.h"

namespace ms {

namespace {

static_assert(sizeof(BpEntry) == sizeof(double2), "the host's entry is the device's double2");
constexpr DenseGeom kBpGeom = {kBestSegWindows, kBpTileEntries / 4, kBpTileEntries, true};
constexpr int kBpRing = 256;                             // window starts the ring holds: four strips
constexpr int kBpStrips = kBestStrips + kBpHaloStrips;   // strips a wave sums per spec
constexpr size_t kBpRingBytes = (size_t) kBestWaves * 2 * kBpRing * sizeof(double);
constexpr size_t kBpLdsBytes = ((size_t) kBpTileEntries + 1) * sizeof(double2) + kBpRingBytes;
static_assert(kBpRing >= 64 * (kBpHaloStrips + 1) && (kBpRing & (kBpRing - 1)) == 0, "the ring holds a strip and its halo");
static_assert(2 * kBpLdsBytes <= 160 * 1024, "two blocks share a CU's LDS");

struct BpSpec {                                          // a spec as the kernel reads it
    int32_t Wa, Wb;
    int32_t bits;                                        // flip | g_min << 8 | g_max << 16
    int32_t pad;
};

struct BpArgs {
    const uint32_t *codes, *nmask;
    const int64_t *offsets;                              // [R + 1]
    int64_t R;
    const int64_t *seg_first;                            // [R + 1]; nullptr: one segment per region
    const int64_t *part_first;                           // [R + 1]; nullptr: no partials
    int64_t n_seg, n_part;
    const int32_t *tile_first;                           // [tiles + 1] into mot
    const int32_t *mot;                                  // the scorable specs, tile after tile
    const double2 *tab;                                  // the specs' tables
    const int64_t *tab_off;                              // [n]
    const BpSpec *spec;                                  // [n]
    const double *denom;                                 // [n] max_raw_a + max_raw_b
    int strand_mask;
    double *score;                                       // [n][R]
    int32_t *pos;
    int8_t *strand;
    int16_t *gap;
    BestPart *part;                                      // [n][n_part]
    int16_t *gap_part;                                   // [n][n_part]
};

// F and R of an element of W columns (its table at entry tb of the LDS tile) at the window start g = beg + pos whose first words are
// (cws, nws); inside: the element's window lies in its region (a lane without one reads no further word)
__device__ __forceinline__ void bp_element_sums(const double2 *__restrict__ lds, uint32_t tb, const uint32_t *__restrict__ codes, const uint32_t *__restrict__ nmask,
                                                int W, int64_t g, bool inside, uint64_t cws, uint32_t nws, double &fwd, double &rev) {
    const int n0 = W < 32 ? W : 32;
    best_cols32(lds, tb, n0, cws, nws | ~low_mask(n0), fwd, rev);
    for (int c0 = 32; c0 < W; c0 += 32) {
        const int n = (W - c0) < 32 ? (W - c0) : 32;
        const uint64_t cwx = inside ? code_window(codes, g + c0) : 0ULL;
        const uint32_t nwx = inside ? n_window(nmask, g + c0) : ~0u;
        best_cols32(lds, tb + (uint32_t) c0 * 4u, n, cwx, nwx | ~low_mask(n), fwd, rev);
    }
}

// the placements of one strand at one start: own + ring[at + g] for g = g_min .. g_max, the divide only where the raw sum improves
__device__ __forceinline__ void bp_placements(const double *ring, int at, double own, int g_min, int g_max, int64_t pos, int64_t room, int strand, double denom,
                                              double &best_raw, double &best_q, uint64_t &best_key) {
    for (int g = g_min; g <= g_max; g++) {
        const double raw = own + ring[(at + g) & (kBpRing - 1)];
        if (g <= room && raw > best_raw) {                // room: the greatest gap whose site still ends inside the region
            best_raw = raw;
            const double q = raw / denom;
            if (q > best_q) { best_q = q; best_key = bp_key(pos, strand, g - g_min); }
        }
    }
}

// grid = (ceil(segments / kBestWaves), tiles)
__global__ void __launch_bounds__(kBestThreads, 4) bipartite_best_kernel(const BpArgs A, int32_t tile0) {
    extern __shared__ double2 bp_lds[];                  // [1 + kBpTileEntries] the tile, then the waves' rings
    const int32_t tile = tile0 + (int32_t) blockIdx.y;
    const int32_t k0 = A.tile_first[tile], k1 = A.tile_first[tile + 1];
    const int64_t tab0 = A.tab_off[A.mot[k0]];
    {
        const int32_t ml = A.mot[k1 - 1];
        const int32_t n = (int32_t) (A.tab_off[ml] - tab0) + 4 * (A.spec[ml].Wa + A.spec[ml].Wb);
        dense_stage_tile(bp_lds, A.tab + tab0, n);
    }
    const int wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const int lane = (int) (threadIdx.x & 63u);
    const int64_t seg = (int64_t) blockIdx.x * kBestWaves + wave;
    if (seg >= A.n_seg) return;
    double *ring_y = reinterpret_cast<double *>(bp_lds + 1 + kBpTileEntries) + (size_t) wave * 2 * kBpRing;      // Y of b, by start & 255
    double *ring_r = ring_y + kBpRing;                                                                            // R of a
    const int64_t r = A.seg_first ? find_region_bsearch(A.seg_first, A.R, seg) : seg;
    const int64_t s_in = A.seg_first ? seg - A.seg_first[r] : 0;
    const bool whole = A.seg_first ? A.seg_first[r + 1] - A.seg_first[r] == 1 : true;
    const int64_t beg = A.offsets[r], L = A.offsets[r + 1] - beg;
    const int64_t p0 = s_in * kBestSegWindows;           // the segment's first window start

    uint64_t cw[kBestStrips];
    uint32_t nw[kBestStrips];
    dense_segment_words(A.codes, A.nmask, beg, L, p0, lane, cw, nw);

    const double ninf = -std::numeric_limits<double>::infinity();
    for (int32_t k = k0; k < k1; k++) {
        const int32_t m = A.mot[k];
        const BpSpec sp = A.spec[m];
        const int Wa = sp.Wa, Wb = sp.Wb;
        const bool flip = (sp.bits & 1) != 0;
        const int g_min = (sp.bits >> 8) & 255, g_max = (sp.bits >> 16) & 255;
        const double denom = A.denom[m];
        const uint32_t tba = 1u + (uint32_t) (A.tab_off[m] - tab0), tbb = tba + 4u * (uint32_t) Wa;
        const int64_t last = L - (Wa + Wb + g_min);       // the region's last placement start, at the smallest gap
        double best_raw = ninf, best_q = ninf;
        uint64_t best_key = kNoKey;
        double own_a1 = 0.0, own_y1 = 0.0, own_a2 = 0.0, own_y2 = 0.0;          // F_a(p), Y'(p) of the strips t - 1 and t - 2
        const int t_end = p0 > last ? 0 : kBpStrips;    // (wave-uniform) no placement starts in this segment at all
#pragma unroll 1
        for (int t = 0; t < t_end; t++) {
            if (t >= kBpHaloStrips && p0 + (t - kBpHaloStrips) * 64 > last) break;                // (wave-uniform) no placement starts in strip t - 2 or later
            double own_a = 0.0, own_y = 0.0;
            if (p0 + t * 64 < L) {                        // (wave-uniform) the strip holds a base of the region
                const int64_t pos = p0 + t * 64 + lane;
                uint64_t cws;
                uint32_t nws;
                if (t < kBestStrips) {                    // the strip's words out of the register arrays: a chain of selects on the wave-uniform t
                    cws = cw[0];
                    nws = nw[0];
#pragma unroll
                    for (int j = 1; j < kBestStrips; j++) { cws = t == j ? cw[j] : cws; nws = t == j ? nw[j] : nws; }
                } else {                                  // the halo: read per spec
                    const bool in = pos < L;
                    cws = in ? code_window(A.codes, beg + pos) : 0ULL;
                    nws = in ? n_window(A.nmask, beg + pos) : ~0u;
                }
                double fa = 0.0, ra = 0.0, fb = 0.0, rb = 0.0;
                bp_element_sums(bp_lds, tba, A.codes, A.nmask, Wa, beg + pos, pos + Wa <= L, cws, nws, fa, ra);
                bp_element_sums(bp_lds, tbb, A.codes, A.nmask, Wb, beg + pos, pos + Wb <= L, cws, nws, fb, rb);
                const int at = (t * 64 + lane) & (kBpRing - 1);
                ring_y[at] = flip ? rb : fb;
                ring_r[at] = ra;
                own_a = fa;
                own_y = flip ? fb : rb;
            }
            // the wave's ring writes of strip t in front of its reads below (one wave: LDS operations complete in order)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (t >= kBpHaloStrips) {                     // the placements that start in strip t - 2: their partners are in the ring
                const int s = t - kBpHaloStrips;
                const int64_t pos = p0 + s * 64 + lane;
                const int64_t room = L - pos - (Wa + Wb);  // a gap g fits iff g <= room
                if (A.strand_mask & 1) bp_placements(ring_y, s * 64 + lane + Wa, own_a2, g_min, g_max, pos, room, 1, denom, best_raw, best_q, best_key);
                if (A.strand_mask & 2) bp_placements(ring_r, s * 64 + lane + Wb, own_y2, g_min, g_max, pos, room, 2, denom, best_raw, best_q, best_key);
            }
            own_a2 = own_a1; own_y2 = own_y1;
            own_a1 = own_a; own_y1 = own_y;
            // (the reads above in front of the next strip's writes to the slot of strip t - 3)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        wave_best(best_q, best_key);
        if (lane == 0) {
            const bool won = best_key != kNoKey;
            const int16_t gap = won ? (int16_t) (g_min + bp_key_dg(best_key)) : (int16_t) -1;
            if (whole) {
                const int64_t cell = (int64_t) m * A.R + r;
                A.score[cell] = won ? best_q : __builtin_nan("");
                A.pos[cell] = won ? (int32_t) bp_key_pos(best_key) : -1;
                A.strand[cell] = won ? (int8_t) bp_key_strand(best_key) : (int8_t) 0;
                A.gap[cell] = gap;
            } else {
                BestPart p;
                p.q = best_q;
                p.pos = won ? (int32_t) bp_key_pos(best_key) : -1;
                p.strand = won ? (int32_t) bp_key_strand(best_key) : 0;
                const int64_t at = (int64_t) m * A.n_part + A.part_first[r] + s_in;
                A.part[at] = p;
                A.gap_part[at] = gap;
            }
        }
    }
}

struct BpTail {
    const int64_t *part_first;                           // [R + 1]
    int64_t n_part, R;
    const int32_t *pos;                                  // [n][R], folded by best_reduce_kernel
    int16_t *gap;                                        // [n][R]
    const int16_t *gap_part;                             // [n][n_part]
};

// grid = (ceil(long regions / 256), scorable specs): the gap of a long region's winner is its segment's
__global__ void __launch_bounds__(256) bipartite_gap_kernel(const BpTail A, const int64_t *__restrict__ long_regions, int64_t n_long, const int32_t *__restrict__ specs) {
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= n_long) return;
    const int64_t r = long_regions[i];
    const int32_t m = specs[blockIdx.y];
    const int64_t cell = (int64_t) m * A.R + r;
    const int32_t pos = A.pos[cell];
    A.gap[cell] = pos >= 0 ? A.gap_part[(int64_t) m * A.n_part + A.part_first[r] + pos / kBestSegWindows] : (int16_t) -1;
}

// grid = (ceil(R / 256), unscorable specs): their rows hold no winner
__global__ void __launch_bounds__(256) bipartite_gap_fill_kernel(int16_t *__restrict__ gap, int64_t R, const int32_t *__restrict__ specs) {
    const int64_t r = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    gap[(int64_t) specs[blockIdx.y] * R + r] = (int16_t) -1;
}

}  // namespace

}  // namespace ms

using namespace ms;

extern "C" {

int ms_debug_bipartite_dims(int32_t out[8]) {
    if (!out) { set_error("NULL output"); return MS_ERR_INVALID; }
    out[0] = kBestThreads;
    out[1] = kBestSegWindows;
    out[2] = kBpTileEntries;
    out[3] = kBpMaxWidth;
    out[4] = kBpMaxGap;
    out[5] = kBpHaloStrips;
    out[6] = (int32_t) kBpLdsBytes;
    out[7] = 0;
    return MS_OK;
}

int ms_scan_best_bipartite(const ms_pwmset *pwms, const int32_t *a, const int32_t *b, const uint8_t *flip, const int32_t *gap_min, const int32_t *gap_max, int32_t n_specs,
                           const ms_seqset *seqs, int strand_mask, uint32_t flags, ms_best **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    int rc = dense_check(pwms, seqs, strand_mask);
    if (rc) return rc;
    if (flags != 0u) { set_error("unknown bipartite best-site scan flags 0x%x", flags); return MS_ERR_INVALID; }
    int32_t bad = -1;
    switch (bp_validate(a, b, flip, gap_min, gap_max, n_specs, pwms->widths.data(), pwms->P, &bad)) {
    case kBpOk: break;
    case kBpNull: set_error("a spec array is NULL"); return MS_ERR_INVALID;
    case kBpCount: set_error("n_specs must be >= 0, got %d", n_specs); return MS_ERR_INVALID;
    case kBpIndex: set_error("spec %d names motifs %d and %d outside [0, %d)", bad, a[bad], b[bad], pwms->P); return MS_ERR_INVALID;
    case kBpFlip: set_error("spec %d has flip %d (0 or 1)", bad, (int) flip[bad]); return MS_ERR_INVALID;
    case kBpGap: set_error("spec %d has gaps %d .. %d (need 0 <= gap_min <= gap_max <= %d)", bad, gap_min[bad], gap_max[bad], kBpMaxGap); return MS_ERR_INVALID;
    case kBpTooWide: set_error("spec %d has an element of more than %d columns (widths %d and %d)", bad, kBpMaxWidth, pwms->widths[(size_t) a[bad]], pwms->widths[(size_t) b[bad]]); return MS_ERR_INVALID;
    }
    const int32_t n = n_specs;
    const int64_t R = seqs->R;

    // ---- the specs as the plan and the kernel read them (ms_bipartite_plan.h): pseudo-widths, the scorable rule, the tables in spec order
    std::vector<int32_t> pseudo;
    std::vector<uint8_t> ok;
    std::vector<double> denom;
    std::vector<BpSpec> spec;
    std::vector<int64_t> tab_off;
    std::vector<BpEntry> tab;
    try {
        pseudo.resize((size_t) n); ok.resize((size_t) n); denom.resize((size_t) n); spec.resize((size_t) n); tab_off.resize((size_t) n);
        int64_t entries = 0;
        for (int32_t k = 0; k < n; k++) {
            const int32_t Wa = pwms->widths[(size_t) a[k]], Wb = pwms->widths[(size_t) b[k]];
            tab_off[(size_t) k] = entries;
            entries += bp_entries(Wa, Wb);
        }
        tab.resize((size_t) entries);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    for (int32_t k = 0; k < n; k++) {
        const int32_t ia = a[k], ib = b[k];
        const int32_t Wa = pwms->widths[(size_t) ia], Wb = pwms->widths[(size_t) ib];
        const double *ma = pwms->values.data() + pwms->val_off[(size_t) ia], *mb = pwms->values.data() + pwms->val_off[(size_t) ib];
        pseudo[(size_t) k] = bp_pseudo_width(Wa, Wb);
        denom[(size_t) k] = bp_denominator(pwms->max_raw[(size_t) ia], pwms->max_raw[(size_t) ib]);
        ok[(size_t) k] = bp_scorable(ma, Wa, pwms->max_raw[(size_t) ia], mb, Wb, pwms->max_raw[(size_t) ib]) ? 1 : 0;
        spec[(size_t) k] = {Wa, Wb, (int32_t) flip[k] | gap_min[k] << 8 | gap_max[k] << 16, 0};
        bp_spec_table(ma, Wa, mb, Wb, tab.data() + tab_off[(size_t) k]);
    }

    BestPtr res(nullptr, ms_best_free);                  // (in front of the run: freed behind the run's wait for the stream)
    DenseRun run;
    if ((rc = dense_open(&run, kBpGeom, pseudo.data(), n, nullptr, seqs, "positions are", [&](int32_t k) { return ok[(size_t) k] != 0; }))) return rc;
    run.lds = run.lds_most = kBpLdsBytes;                // the full tile and the waves' rings, whatever the plan's largest tile
    if ((rc = best_alloc(run, n, R, &res, true))) return rc;
    if (n == 0 || R == 0) { *out = res.release(); return MS_OK; }
    const DensePlan &plan = run.plan;

    // ---- the work block: the plan, the specs' tables and arrays (a few KB per spec, uploaded per call in front of the timed launches),
    // the partials and their gaps
    Carve &cv = run.cv;
    const auto s_tab = cv.add<BpEntry>(tab.size());
    const auto s_tab_off = cv.add<int64_t>((size_t) n);
    const auto s_spec = cv.add<BpSpec>((size_t) n);
    const auto s_denom = cv.add<double>((size_t) n);
    const auto s_part = cv.add<BestPart>((size_t) n * (size_t) plan.n_part);
    const auto s_gap_part = cv.add<int16_t>((size_t) n * (size_t) plan.n_part);
    if ((rc = dense_start(&run, nullptr, seqs, reinterpret_cast<const void *>(bipartite_best_kernel)))) return rc;
    const hipStream_t st = run.st;
    hipError_t he = hipSuccess;
    auto up = [&](const auto &v, auto slot) {
        auto *p = Carve::at(run.work.p, slot);
        if (he == hipSuccess && !v.empty()) he = hipMemcpyAsync(p, v.data(), sizeof(v[0]) * v.size(), hipMemcpyHostToDevice, st);
        return p;
    };
    const DenseDev &d = run.d;
    BpArgs A;
    A.tab = reinterpret_cast<const double2 *>(up(tab, s_tab));
    A.tab_off = up(tab_off, s_tab_off);
    A.spec = up(spec, s_spec);
    A.denom = up(denom, s_denom);
    if (he != hipSuccess) return hip_rc(he, "upload of the specs");
    A.codes = seqs->d_codes; A.nmask = seqs->d_nmask; A.offsets = seqs->d_offsets; A.R = R;
    A.seg_first = d.seg_first; A.part_first = d.part_first;
    A.n_seg = plan.n_seg; A.n_part = plan.n_part;
    A.tile_first = d.tile_first; A.mot = d.mot;
    A.strand_mask = strand_mask;
    A.score = res->d_score; A.pos = res->d_pos; A.strand = res->d_strand; A.gap = res->d_gap;
    A.part = Carve::at(run.work.p, s_part);
    A.gap_part = Carve::at(run.work.p, s_gap_part);

    (void) hipEventRecord(run.c->ev[0], st);
    rc = dense_chunks((int64_t) plan.tile_first.size() - 1, "bipartite best-site kernel", [&](int64_t t0, unsigned ny) {
        hipLaunchKernelGGL(bipartite_best_kernel, dim3(run.gx, ny), dim3(kBestThreads), run.lds, st, A, (int32_t) t0);
    });
    if (!rc) rc = best_tail(run, "bipartite best-site", A.part, res.get());
    const BpTail T = {d.part_first, plan.n_part, R, res->d_pos, res->d_gap, A.gap_part};
    const int64_t n_long = (int64_t) plan.long_regions.size();
    if (!rc && n_long > 0) rc = dense_chunks((int64_t) plan.mot.size(), "bipartite gap gather", [&](int64_t k0, unsigned ny) {
        hipLaunchKernelGGL(bipartite_gap_kernel, dim3((unsigned) ((n_long + 255) / 256), ny), dim3(256), 0, st, T, d.long_regions, n_long, d.mot + k0);
    });
    if (!rc) rc = dense_chunks((int64_t) plan.skipped.size(), "bipartite gap fill", [&](int64_t u0, unsigned ny) {
        hipLaunchKernelGGL(bipartite_gap_fill_kernel, dim3((unsigned) ((R + 255) / 256), ny), dim3(256), 0, st, res->d_gap, R, d.skipped + u0);
    });
    if (!rc) rc = dense_end(&run, "bipartite best-site scan", res.get());
    if (rc) return rc;
    *out = res.release();
    return MS_OK;
}

int ms_best_gaps(const ms_best *b, int32_t m0, int32_t m1, int16_t *gap) {
    if (!b) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (!b->d_gap) { set_error("the result holds no gap plane: it is not ms_scan_best_bipartite's"); return MS_ERR_INVALID; }
    size_t at = 0, n = 0;
    if (int rc = dense_rows(b, m0, m1, &at, &n)) return rc;
    if (gap && n) MS_HIP(hipMemcpy(gap, b->d_gap + at, 2 * n, hipMemcpyDeviceToHost));
    return MS_OK;
}

int ms_best_gaps_device(const ms_best *b, void **d_gap) {
    if (!b) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (!b->d_gap) { set_error("the result holds no gap plane: it is not ms_scan_best_bipartite's"); return MS_ERR_INVALID; }
    if (d_gap) *d_gap = b->d_gap;
    return MS_OK;
}

}  // extern "C"
