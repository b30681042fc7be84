// ms_alleles.hip -- motif sites on the two haplotypes of sequence-resolved alleles of any length (ms_scan_alleles): substitutions,
// multi-base replacements, insertions and deletions on a genome that is resident in HBM.
//
// Variant v = (chromosome, x, r, alt[0..a)) replaces the r reference bases [x, x + r) by a alt bases.  The ref haplotype is the
// chromosome, the alt haplotype chrom[0:x] + alt + chrom[x + r:].  For a motif of width W the windows that matter on a haplotype
// whose allele has `len` bases (r or a) start at max(0, x - W + 1) .. min(x + len - 1, L_h - W) in that haplotype's coordinates: with
// lo = x bases in front of the allele and hi = L - x - r behind it that is  len + min(0, hi - W + 1) + min(lo, W - 1)  windows (none when
// that is <= 0; len = 0 leaves the windows that straddle the junction).  Every one is scored with the scan's arithmetic (cscore.c:336-390;
// ms_fp64.hip: columns 0 .. W - 1, forward M[b][c], reverse M[3 - b][W - 1 - c] at the same step, a non-ACGT base adds +0.0,
// raw / max_raw, score - cutoff >= -1e-10) and gives 0, 1 or 2 records ('+' before '-').
//
// Mapping.  A work item is (variant, allele, window): one haplotype, so two fp64 adds a column and no select (ms_variants.hip scores
// both alleles of a window in one item, which only works while they have the same length).  The items of a motif are numbered
// variant-major, ref before alt, start ascending: item order IS the output order.  A block owns one motif and a TILE of kAlTile
// variants.  A variant's item count depends on r, a and its distance to the chromosome's ends, so the tile keeps the exclusive prefix
// of its variants' item counts in LDS, and a thread finds the variant of its item of the round by a 7-step binary search in it.
// Placement is ms_scan_variants's, the same code (place_round, ms_allele_dev.h): ballot prefix inside the wave, the waves' totals through
// LDS, no sort and no atomic on the records.
//
// Splice.  The alt bytes of all variants are packed by a prep kernel into a 2-bit code plane and a non-ACGT mask plane in the genome's
// own layout (ms_device.h), so code_window / n_window read them too.  A 32-column step of an alt-haplotype window is put together of
// at most three such reads -- genome left of x, the alt plane, genome from x + r on -- by shifts and masks; a step that lies wholly on
// one side of the allele, and every step of a ref-haplotype window, is one read.
//
// Order without a sort: pass 1 counts the records of every (motif, tile), an exclusive prefix sum and the per-motif totals place every
// block, pass 2 recomputes and writes; variants go in chunks that bound the count arrays.  That driver is place_records (ms_variants.hip,
// declared in ms_handles.h; the chunk plan is place_chunks of ms_place.h under the same ms_debug_varscan_chunk): this file gives it the
// two launches and the allocation of the record arrays.  The upload of the variants is al_upload (ms_allele_dev.h), shared with
// ms_allelebest.hip and ms_personal.hip.  One long allele makes its tile's block long: no balancing is done for it.
#include <algorithm>
#include <memory>
#include <type_traits>

#include "ms_allele_dev.h"
#include "ms_device.h"
#include "ms_handles.h"

struct ms_allelescan : ms::RecHead {
    int64_t *d_variant = nullptr;
    int64_t *d_start = nullptr;
    double *d_score = nullptr;
    int8_t *d_strand = nullptr;
    uint8_t *d_allele = nullptr;
    std::vector<uint8_t> mismatch;                    // [V]
};

namespace ms {

namespace {

constexpr int kAlTile = 128;                    // variants per block
constexpr int kAlThreads = 256;
constexpr int kAlTabMaxW = 896;                 // widest motif whose table (W x 4 entries, 56 KB) fits 64 KB of LDS beside the tile's 6 KB; wider ones read it from HBM
constexpr int64_t kAlMaxTiles = 1LL << 24;      // (motif, tile) counts of one chunk

struct AlOut {
    int64_t *variant, *start;
    double *score;
    int8_t *strand;
    uint8_t *allele;
    uint64_t cap;
};

// the reference's normalisation and hit test for one strand (cscore.c:356-358 / 373-375; test_and_emit of ms_fp64.hip: a raw sum below
// the motif's floor cannot pass, so the divide is paid only by windows that can).  Both passes call THIS.
__device__ __forceinline__ bool judge_one(double raw, double max_raw, double cutoff, double floor_, double &score) {
    score = 0.0;
    if (raw < floor_) return false;
    score = raw / max_raw;
    return score - cutoff >= -1e-10;
}

// grid = (tiles of the chunk, motifs).  FILL = false: tile_cnt[motif][tile] = records of the tile, and (gained != nullptr) the motif's
// variants with only alt / only ref records; FILL = true: the records, from row_base[motif] + (tile_excl[motif][tile] -
// tile_excl[motif][0]) on.  LDS_TAB: the motif's table in LDS (W <= kAlTabMaxW) or read from HBM; a block of the other kind leaves at once.
template <bool FILL, bool LDS_TAB>
__global__ void __launch_bounds__(kAlThreads) al_scan_kernel(const uint32_t *__restrict__ codes, const uint32_t *__restrict__ nmask,
                                                             const uint32_t *__restrict__ acodes, const uint32_t *__restrict__ amask, const DevPwm Pw,
                                                             const AlRec *__restrict__ rec, const int64_t *__restrict__ pos, int64_t v0, int64_t nv,
                                                             int strand_mask, uint32_t *__restrict__ tile_cnt, const uint64_t *__restrict__ tile_excl,
                                                             const uint64_t *__restrict__ row_base, unsigned long long *__restrict__ gained,
                                                             unsigned long long *__restrict__ lost, const AlOut O) {
    extern __shared__ double2 atab_lds[];                      // [W * 4 + 1]: the motif's entries, and an all-zero one for the columns that add nothing
    __shared__ uint32_t s_wtot[2][kAlThreads / 64];
    __shared__ uint32_t s_flag[kAlTile];
    __shared__ uint32_t s_pre[kAlTile + 1];                    // exclusive prefix of the variants' item counts
    __shared__ uint32_t s_half[2];
    __shared__ AlRec s_rec[kAlTile];
    const int32_t m = (int32_t) blockIdx.y;
    const int W = Pw.width[m];
    if ((W <= kAlTabMaxW) != LDS_TAB) return;
    const double2 *__restrict__ tab_g = Pw.tab2 + Pw.tab_off[m];
    const uint32_t zero = (uint32_t) W * 4u;
    if (LDS_TAB) tab_stage<kAlThreads>(atab_lds, tab_g, W);
    const int64_t tile = (int64_t) blockIdx.x, row = (int64_t) m * gridDim.x;
    const int64_t vl0 = tile * kAlTile;                        // first variant of the tile, in the chunk
    const int n_local = (int) (nv - vl0 < kAlTile ? nv - vl0 : kAlTile);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // ---- the tile's variants and the prefix of their item counts (waves 0 and 1 hold the kAlTile counts)
    uint32_t cnt = 0u;
    if ((int) threadIdx.x < n_local) {
        const AlRec q = rec[v0 + vl0 + threadIdx.x];
        s_rec[threadIdx.x] = q;
        cnt = allele_windows(q.lo, q.hi, q.r, W) + allele_windows(q.lo, q.hi, q.a, W);
    }
    uint32_t inc = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(inc, d);
        if ((int) lane >= d) inc += y;
    }
    if (wave < 2u && lane == 63u) s_half[wave] = inc;
    if (threadIdx.x < kAlTile) s_flag[threadIdx.x] = 0u;
    __syncthreads();
    if (threadIdx.x < kAlTile) s_pre[threadIdx.x] = inc - cnt + (wave == 1u ? s_half[0] : 0u);
    if (threadIdx.x == 0) s_pre[kAlTile] = s_half[0] + s_half[1];
    __syncthreads();
    const uint32_t n_items = s_pre[kAlTile];
    const double max_raw = Pw.max_raw[m], cutoff = Pw.cutoff[m], floor_ = Pw.raw_floor[m];
    uint64_t run = 0;                                          // records of the tile's earlier rounds (+ the tile's place when filling)
    if (FILL) run = row_base[m] + (tile_excl[row + tile] - tile_excl[row]);
    int round = 0;
    for (uint32_t i0 = 0; i0 < n_items; i0 += kAlThreads, round++) {
        bool hit_f = false, hit_r = false;
        double sc_f = 0.0, sc_r = 0.0;
        int vl = 0, rel = 0;
        uint32_t allele = 0u;
        const uint32_t i = i0 + threadIdx.x;
        if (i < n_items) {
#pragma unroll
            for (int step = kAlTile / 2; step > 0; step >>= 1)  // the last variant whose prefix is <= i: its count is not 0
                if (s_pre[vl + step] <= i) vl += step;
            const AlRec q = s_rec[vl];
            const uint32_t k = i - s_pre[vl], n_ref = allele_windows(q.lo, q.hi, q.r, W);
            allele = k >= n_ref ? 1u : 0u;
            rel = (int) (allele ? k - n_ref : k) - (q.lo < W - 1 ? q.lo : W - 1);      // the window's start, from x on
            double fw = 0.0, rv = 0.0;
            for (int c0 = 0; c0 < W; c0 += 32) {
                const int n = (W - c0) < 32 ? (W - c0) : 32;
                uint64_t cw;
                uint32_t nw;
                if (allele) {
                    alt_step(codes, nmask, acodes, amask, q, rel + c0, n, cw, nw);
                } else {
                    cw = code_window(codes, q.g + rel + c0);
                    nw = n_window(nmask, q.g + rel + c0);
                }
                // tab_step<LDS_TAB, false> (ms_allele_dev.h) written out: called through the function, hipcc schedules this kernel's walk
                // differently (its disassembly changes) and the scan measures 0.9 % slower; the code is to stay as measured.  A change
                // to the step is made in both places.
                const uint32_t skip = nw | ~low_mask(n);                               // bit c: column c0 + c adds nothing
                // eight columns a step while more than four are left, then four: the reads of a step are issued together
                auto columns = [&](auto width, int c1) {
                    constexpr int N = decltype(width)::value;
                    double2 t[N];
#pragma unroll
                    for (int u = 0; u < N; u++) {
                        const int c = c1 + u;
                        const bool nothing = (skip >> c) & 1u;                          // adds +0.0: a sum that started at +0.0 is never -0.0
                        if constexpr (LDS_TAB) {
                            t[u] = atab_lds[nothing ? zero : (uint32_t) (c0 + c) * 4u + ((uint32_t) (cw >> (2 * c)) & 3u)];
                        } else {
                            const int cc = c < n ? c : n - 1;                           // clamped: always an entry of the motif
                            t[u] = tab_g[(uint32_t) (c0 + cc) * 4u + ((uint32_t) (cw >> (2 * cc)) & 3u)];
                            if (nothing) t[u] = make_double2(0.0, 0.0);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < N; u++) {
                        fw += t[u].x;
                        rv += t[u].y;
                    }
                };
                int c1 = 0;
                for (; n - c1 > 4; c1 += 8) columns(std::integral_constant<int, 8>{}, c1);
                if (n - c1 > 0) columns(std::integral_constant<int, 4>{}, c1);
            }
            if (strand_mask & 1) hit_f = judge_one(fw, max_raw, cutoff, floor_, sc_f);
            if (strand_mask & 2) hit_r = judge_one(rv, max_raw, cutoff, floor_, sc_r);
        }
        uint32_t before, all;
        place_round<kAlThreads>(s_wtot, round, hit_f, hit_r, before, all);
        if (FILL) {
            uint64_t d = run + before;
            const int64_t v = v0 + vl0 + vl;
            if (hit_f && d < O.cap) {
                O.variant[d] = v; O.start[d] = pos[v] + rel; O.strand[d] = (int8_t) 1; O.allele[d] = (uint8_t) allele; O.score[d] = sc_f;
            }
            d += hit_f ? 1u : 0u;
            if (hit_r && d < O.cap) {
                O.variant[d] = v; O.start[d] = pos[v] + rel; O.strand[d] = (int8_t) 2; O.allele[d] = (uint8_t) allele; O.score[d] = sc_r;
            }
        } else if (gained) {
            if (hit_f || hit_r) atomicOr(&s_flag[vl], 1u << allele);                   // (an OR: the order of the writers cannot show)
        }
        run += all;
    }
    if (!FILL) {
        if (threadIdx.x == 0) tile_cnt[row + tile] = (uint32_t) run;
        if (gained) {
            __syncthreads();
            const uint32_t f = (int) threadIdx.x < n_local ? s_flag[threadIdx.x] : 0u;
            tally_motif(f == 1u, f == 2u, &lost[m], &gained[m]);                        // records of the ref haplotype only / the alt only
        }
    }
}

struct AlLaunch {
    const ms_seqset *G;
    const uint32_t *acodes, *amask;
    DevPwm Pw;
    const AlRec *rec;
    const int64_t *pos;
    int strand_mask;
    int max_width, min_width;
    size_t lds;
};

template <bool FILL>
int launch_al_scan(const AlLaunch &L, int64_t v0, int64_t nv, uint32_t *tile_cnt, const uint64_t *tile_excl, const uint64_t *row_base,
                   unsigned long long *gained, unsigned long long *lost, const AlOut &O, hipStream_t st) {
    const dim3 grid((unsigned) ((nv + kAlTile - 1) / kAlTile), (unsigned) L.Pw.P);
    if (L.min_width <= kAlTabMaxW) {
        hipLaunchKernelGGL((al_scan_kernel<FILL, true>), grid, dim3(kAlThreads), L.lds, st, L.G->d_codes, L.G->d_nmask, L.acodes, L.amask, L.Pw, L.rec,
                           L.pos, v0, nv, L.strand_mask, tile_cnt, tile_excl, row_base, gained, lost, O);
        MS_HIP(hipGetLastError());
    }
    if (L.max_width > kAlTabMaxW) {
        hipLaunchKernelGGL((al_scan_kernel<FILL, false>), grid, dim3(kAlThreads), 0, st, L.G->d_codes, L.G->d_nmask, L.acodes, L.amask, L.Pw, L.rec,
                           L.pos, v0, nv, L.strand_mask, tile_cnt, tile_excl, row_base, gained, lost, O);
        MS_HIP(hipGetLastError());
    }
    return MS_OK;
}

}  // namespace

void allelescan_dims(int32_t out[3]) {
    out[0] = kAlTile;
    out[1] = kAlThreads;
    out[2] = kAlTabMaxW;
}

}  // namespace ms

using namespace ms;

extern "C" {

void ms_allelescan_free(ms_allelescan *r) {
    rec_release(r);
    delete r;
}

int ms_scan_alleles(const ms_pwmset *pwms_c, const ms_genome *genome, const int32_t *chrom, const int64_t *pos, const int32_t *ref_len,
                    const char *alt_bases, const int64_t *alt_offsets, const char *ref_bases, int64_t n_variants, int strand_mask,
                    uint32_t flags, ms_allelescan **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    if (strand_mask < 1 || strand_mask > 3) { set_error("invalid strand mask %d (1 '+', 2 '-', 3 both)", strand_mask); return MS_ERR_INVALID; }
    if (flags != 0u) { set_error("unknown allele scan flags 0x%x", flags); return MS_ERR_INVALID; }
    if (!require_device()) return MS_ERR_RUNTIME;
    if (!pwms_c || !genome) { set_error("NULL handle"); return MS_ERR_INVALID; }
    ms_pwmset *pwms = const_cast<ms_pwmset *>(pwms_c);
    const ms_seqset *G = reinterpret_cast<const ms_seqset *>(genome);
    const int64_t V = n_variants;
    const int32_t P = pwms->P;
    std::vector<int64_t> ref_off;
    int64_t A = 0, Rn = 0;
    int rc = validate_alleles(G, chrom, pos, ref_len, alt_bases, alt_offsets, ref_bases, V, ref_off, &A, &Rn);
    if (rc) return rc;
    DeviceCtx *c;
    if ((rc = get_ctx(G->device, &c))) return rc;
    std::unique_ptr<ms_allelescan> res(new (std::nothrow) ms_allelescan());
    if (!res) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    try {
        res->motif_offsets.assign((size_t) P + 1, 0);
        res->gained.assign((size_t) P, 0);
        res->lost.assign((size_t) P, 0);
        res->mismatch.assign((size_t) V, 0);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    res->device = c->device;
    res->P = P;
    res->V = V;
    std::lock_guard<std::mutex> lk_dev(c->mu);
    std::lock_guard<std::mutex> lk_pwm(pwms->mu);
    if ((rc = pwmset_upload(pwms, c->device, c->stream))) return rc;
    const hipStream_t st = c->stream;

    // ---- chunks of variants: at most kAlMaxTiles (motif, tile) counts at a time
    const PlaceChunks ch = place_chunks(V, P, kAlTile, kAlMaxTiles, varscan_chunk_setting());
    Carve cv;
    const AlSlots us = al_upload_slots(cv, V, A, Rn);
    PlaceSlots ps;
    if ((rc = place_slots(cv, ch, P, st, &ps))) return rc;
    void *wblk = nullptr;
    size_t wgot = 0;
    if ((rc = pool_alloc(c, cv.bytes(), &wblk, &wgot))) return rc;
    const AlDev U = al_upload_at(wblk, us);
    ms_allelescan *raw = res.release();
    auto fail = [&](int code) { (void) hipStreamSynchronize(st); pool_free(c, wblk, wgot); ms_allelescan_free(raw); return code; };   // (nothing queued may still read the blocks)
    auto hip_fail = [&](hipError_t e, const char *what) { set_error("%s failed: %s", what, hipGetErrorString(e)); return fail(e == hipErrorOutOfMemory ? MS_ERR_NOMEM : MS_ERR_RUNTIME); };

    AlLaunch L;
    L.G = G; L.acodes = U.acode; L.amask = U.amask; L.Pw = dev_pwm(pwms); L.rec = U.rec; L.pos = U.pos; L.strand_mask = strand_mask;
    L.max_width = pwms->max_width;
    L.min_width = P > 0 ? *std::min_element(pwms->widths.begin(), pwms->widths.end()) : 0;
    int lds_width = 0;
    for (int32_t p = 0; p < P; p++) if (pwms->widths[p] <= kAlTabMaxW) lds_width = std::max(lds_width, (int) pwms->widths[p]);
    L.lds = ((size_t) lds_width * 4 + 1) * sizeof(double2);
    hipError_t he = hipSuccess;
    if (L.lds > 40 * 1024) {                                   // (the static arrays of the kernel take 6 KB of the 48 KB a launch gets unasked)
        he = hipFuncSetAttribute(reinterpret_cast<const void *>(al_scan_kernel<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int) L.lds);
        if (he == hipSuccess) he = hipFuncSetAttribute(reinterpret_cast<const void *>(al_scan_kernel<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int) L.lds);
        if (he != hipSuccess) return hip_fail(he, "raising the LDS limit");
    }

    (void) hipEventRecord(c->ev[0], st);
    if (V > 0) {
        he = al_upload(G, U, chrom, pos, ref_len, alt_bases, alt_offsets, ref_bases, ref_off, V, A, Rn, raw->mismatch.data(), st);
        if (he != hipSuccess) return hip_fail(he, "variant upload");
    }

    AlOut O{};                                                 // (no arrays while counting)
    PlaceCalls calls;
    calls.count = [&](int64_t v0, int64_t nv, uint32_t *tile_cnt, unsigned long long *gained, unsigned long long *lost) {
        return launch_al_scan<false>(L, v0, nv, tile_cnt, nullptr, nullptr, gained, lost, O, st);
    };
    calls.fill = [&](int64_t v0, int64_t nv, const uint64_t *tile_excl, const uint64_t *row_base) {
        return launch_al_scan<true>(L, v0, nv, nullptr, tile_excl, row_base, nullptr, nullptr, O, st);
    };
    calls.alloc = [&](size_t n) {
        const size_t nz = std::max<size_t>(n, 1);
        Carve rv;
        const auto s_variant = rv.add<int64_t>(nz), s_start = rv.add<int64_t>(nz);
        const auto s_score = rv.add<double>(nz);
        const auto s_strand = rv.add<int8_t>(nz);
        const auto s_allele = rv.add<uint8_t>(nz);
        void *blk = nullptr;
        size_t got = 0;
        if (int r = pool_alloc(c, rv.bytes(), &blk, &got)) return r;
        raw->block = blk;
        raw->block_bytes = got;
        O.variant = raw->d_variant = Carve::at(blk, s_variant);
        O.start = raw->d_start = Carve::at(blk, s_start);
        O.score = raw->d_score = Carve::at(blk, s_score);
        O.strand = raw->d_strand = Carve::at(blk, s_strand);
        O.allele = raw->d_allele = Carve::at(blk, s_allele);
        O.cap = (uint64_t) n;
        return MS_OK;
    };
    if ((rc = place_records(c, ch, kAlTile, wblk, ps, "allele", calls, raw))) return fail(rc);
    pool_free(c, wblk, wgot);
    *out = raw;
    return MS_OK;
}

int ms_allelescan_num_sites(const ms_allelescan *r, int64_t *n) { return rec_num_sites(r, n); }
int ms_allelescan_motif_offsets(const ms_allelescan *r, int64_t *out) { return rec_motif_offsets(r, out); }
int ms_allelescan_motif_counts(const ms_allelescan *r, int64_t *gained, int64_t *lost) { return rec_motif_counts(r, gained, lost); }
int ms_allelescan_device_ms(const ms_allelescan *r, double *ms) { return rec_device_ms(r, ms); }

int ms_allelescan_sites(const ms_allelescan *r, int64_t *variant, uint8_t *allele, int64_t *start, int8_t *strand, double *score) {
    if (!r) { set_error("NULL argument"); return MS_ERR_INVALID; }
    const size_t n = (size_t) r->n;
    if (n == 0) return MS_OK;
    MS_HIP(hipSetDevice(r->device));
    if (variant) MS_HIP(hipMemcpy(variant, r->d_variant, 8 * n, hipMemcpyDeviceToHost));
    if (allele) MS_HIP(hipMemcpy(allele, r->d_allele, n, hipMemcpyDeviceToHost));
    if (start) MS_HIP(hipMemcpy(start, r->d_start, 8 * n, hipMemcpyDeviceToHost));
    if (strand) MS_HIP(hipMemcpy(strand, r->d_strand, n, hipMemcpyDeviceToHost));
    if (score) MS_HIP(hipMemcpy(score, r->d_score, 8 * n, hipMemcpyDeviceToHost));
    return MS_OK;
}

int ms_allelescan_ref_mismatch(const ms_allelescan *r, uint8_t *out) {
    if (!r || (!out && r->V > 0)) { set_error("NULL argument"); return MS_ERR_INVALID; }
    std::copy(r->mismatch.begin(), r->mismatch.end(), out);
    return MS_OK;
}

}  // extern "C"
