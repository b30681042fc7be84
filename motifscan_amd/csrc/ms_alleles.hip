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
// Placement is ms_variants.hip's: ballot prefix inside the wave, the waves' totals through LDS, no sort and no atomic on the records.
//
// Splice.  The alt bytes of all variants are packed by a prep kernel into a 2-bit code plane and a non-ACGT mask plane in the genome's
// own layout (ms_device.h), so code_window / n_window read them too.  A 32-column step of an alt-haplotype window is put together of
// at most three such reads -- genome left of x, the alt plane, genome from x + r on -- by shifts and masks; a step that lies wholly on
// one side of the allele, and every step of a ref-haplotype window, is one read.
//
// Order without a sort: pass 1 counts the records of every (motif, tile), an exclusive prefix sum and the per-motif totals place every
// block, pass 2 recomputes and writes; variants go in chunks that bound the count arrays (ms_variants.hip: the same scheme and the same
// ms_debug_varscan_chunk).  One long allele makes its tile's block long: no balancing is done for it.
#include <algorithm>
#include <memory>
#include <type_traits>

#include "ms_allele_dev.h"
#include "ms_device.h"
#include "ms_handles.h"

struct ms_allelescan {
    int device = 0;
    int32_t P = 0;
    int64_t V = 0;
    int64_t n = 0;                                    // records
    void *block = nullptr;                            // one pooled device block holding the record arrays
    size_t block_bytes = 0;
    int64_t *d_variant = nullptr;
    int64_t *d_start = nullptr;
    double *d_score = nullptr;
    int8_t *d_strand = nullptr;
    uint8_t *d_allele = nullptr;
    std::vector<int64_t> motif_offsets;               // [P+1]
    std::vector<int64_t> gained, lost;                // [P], counted on the device
    std::vector<uint8_t> mismatch;                    // [V]
    double device_ms = 0.0;                           // first launch -> last kernel done
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
    if (LDS_TAB) {
        for (int i = threadIdx.x; i < W * 4; i += kAlThreads) atab_lds[i] = tab_g[i];
        if (threadIdx.x == 0) atab_lds[zero] = make_double2(0.0, 0.0);
    }
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
    const uint64_t lt = (1ULL << lane) - 1ULL;
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
        const unsigned long long bf = __ballot(hit_f), br = __ballot(hit_r);
        const int buf = round & 1;                             // (two buffers: a wave may write round r + 1's total while another still reads round r's)
        if (lane == 0u) s_wtot[buf][wave] = (uint32_t) (__popcll(bf) + __popcll(br));
        __syncthreads();
        uint32_t before = 0u, all = 0u;
#pragma unroll
        for (uint32_t w = 0; w < (uint32_t) (kAlThreads / 64); w++) {
            const uint32_t x = s_wtot[buf][w];
            all += x;
            if (w < wave) before += x;
        }
        if (FILL) {
            uint64_t d = run + before + (uint64_t) (__popcll(bf & lt) + __popcll(br & lt));
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
            const unsigned long long bl = __ballot(f == 1u), bg = __ballot(f == 2u);    // records of the ref haplotype only / the alt only
            if (lane == 0u) {
                if (bl) atomicAdd(&lost[m], (unsigned long long) __popcll(bl));            // (integer sums: the same in any order)
                if (bg) atomicAdd(&gained[m], (unsigned long long) __popcll(bg));
            }
        }
    }
}

// tot[m] = records of motif m in the chunk, out of the prefix sums of its tiles (tile_excl has one entry more than there are tiles)
__global__ void __launch_bounds__(256) al_row_total_kernel(const uint64_t *__restrict__ tile_excl, int64_t ntx, int32_t P, uint64_t *__restrict__ tot) {
    const int32_t m = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    if (m < P) tot[m] = tile_excl[(int64_t) (m + 1) * ntx] - tile_excl[(int64_t) m * ntx];
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

size_t al_up256(size_t x) { return (x + 255) & ~(size_t) 255; }

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
    if (!r) return;
    if (r->block) {
        (void) hipSetDevice(r->device);
        DeviceCtx *c = nullptr;
        if (get_ctx(r->device, &c) == MS_OK) pool_free(c, r->block, r->block_bytes); else (void) hipFree(r->block);
    }
    delete r;
}

int ms_scan_alleles(const ms_pwmset *pwms_c, const ms_genome *genome, const int32_t *chrom, const int64_t *pos, const int32_t *ref_len,
                    const char *alt_bases, const int64_t *alt_offsets, const char *ref_bases, int64_t n_variants, int strand_mask,
                    uint32_t flags, ms_allelescan **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    if (strand_mask < 1 || strand_mask > 3) { set_error("invalid strand mask %d (1 '+', 2 '-', 3 both)", strand_mask); return MS_ERR_INVALID; }
    if (flags != 0u) { set_error("unknown allele scan flags 0x%x", flags); return MS_ERR_INVALID; }
    {
        int n_dev = 0;                                         // (a genome handle cannot exist without a device: say so before asking for one)
        if (ms_device_count(&n_dev) != MS_OK || n_dev <= 0) { set_error("no usable HIP device; libmotifscan_amd has no CPU fallback"); return MS_ERR_RUNTIME; }
    }
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
    int64_t chunk = varscan_chunk_setting();
    if (chunk <= 0) chunk = std::max<int64_t>(1, kAlMaxTiles / std::max<int32_t>(P, 1)) * kAlTile;
    chunk = std::min<int64_t>(chunk, std::max<int64_t>(V, 1));
    const int64_t n_chunks = V > 0 ? (V + chunk - 1) / chunk : 0;
    const int64_t ntx_max = (chunk + kAlTile - 1) / kAlTile;
    const size_t n_cells = (size_t) ntx_max * (size_t) std::max<int32_t>(P, 1) + 1;

    size_t scan_tmp = 0;
    if ((rc = exclusive_sum_u32(nullptr, &scan_tmp, nullptr, nullptr, n_cells, st))) return rc;
    const size_t Vz = (size_t) std::max<int64_t>(V, 1), Pz = (size_t) std::max<int32_t>(P, 1), Kz = (size_t) std::max<int64_t>(n_chunks, 1);
    const size_t a_words = (size_t) ((A + 31) / 32);            // mask words of the alt plane; twice as many code words
    const size_t b_chrom = al_up256(4 * Vz), b_pos = al_up256(8 * Vz), b_rlen = al_up256(4 * Vz), b_aoff = al_up256(8 * (Vz + 1)),
                 b_roff = al_up256(8 * (Vz + 1)), b_alt = al_up256((size_t) std::max<int64_t>(A, 1)), b_ref = al_up256((size_t) std::max<int64_t>(Rn, 1)),
                 b_acode = al_up256(4 * (2 * a_words + kAlPlanePad)), b_amask = al_up256(4 * (a_words + kAlPlanePad)), b_rec = al_up256(sizeof(AlRec) * Vz),
                 b_mis = al_up256(Vz), b_cnt = al_up256(4 * n_cells), b_excl = al_up256(8 * n_cells), b_tot = al_up256(8 * Kz * Pz), b_gl = al_up256(16 * Pz),
                 b_tmp = al_up256(std::max<size_t>(scan_tmp, 1));
    void *wblk = nullptr;
    size_t wgot = 0;
    if ((rc = pool_alloc(c, b_chrom + b_pos + b_rlen + b_aoff + b_roff + b_alt + b_ref + b_acode + b_amask + b_rec + b_mis + b_cnt + b_excl + 2 * b_tot + b_gl + b_tmp,
                         &wblk, &wgot))) return rc;
    char *b = static_cast<char *>(wblk);
    int32_t *d_chrom = reinterpret_cast<int32_t *>(b); b += b_chrom;
    int64_t *d_pos = reinterpret_cast<int64_t *>(b); b += b_pos;
    int32_t *d_rlen = reinterpret_cast<int32_t *>(b); b += b_rlen;
    int64_t *d_aoff = reinterpret_cast<int64_t *>(b); b += b_aoff;
    int64_t *d_roff = reinterpret_cast<int64_t *>(b); b += b_roff;
    uint8_t *d_alt = reinterpret_cast<uint8_t *>(b); b += b_alt;
    uint8_t *d_ref = reinterpret_cast<uint8_t *>(b); b += b_ref;
    uint32_t *d_acode = reinterpret_cast<uint32_t *>(b); b += b_acode;
    uint32_t *d_amask = reinterpret_cast<uint32_t *>(b); b += b_amask;
    AlRec *d_rec = reinterpret_cast<AlRec *>(b); b += b_rec;
    uint8_t *d_mis = reinterpret_cast<uint8_t *>(b); b += b_mis;
    uint32_t *d_cnt = reinterpret_cast<uint32_t *>(b); b += b_cnt;
    uint64_t *d_excl = reinterpret_cast<uint64_t *>(b); b += b_excl;
    uint64_t *d_tot = reinterpret_cast<uint64_t *>(b); b += b_tot;          // [chunks][P] records of the motif in the chunk
    uint64_t *d_base = reinterpret_cast<uint64_t *>(b); b += b_tot;         // [chunks][P] where they go
    unsigned long long *d_gained = reinterpret_cast<unsigned long long *>(b);
    unsigned long long *d_lost = d_gained + Pz; b += b_gl;
    void *d_tmp = b;
    ms_allelescan *raw = res.release();
    auto fail = [&](int code) { pool_free(c, wblk, wgot); ms_allelescan_free(raw); return code; };
    auto hip_fail = [&](hipError_t e, const char *what) { set_error("%s failed: %s", what, hipGetErrorString(e)); return fail(e == hipErrorOutOfMemory ? MS_ERR_NOMEM : MS_ERR_RUNTIME); };

    AlLaunch L;
    L.G = G; L.acodes = d_acode; L.amask = d_amask; L.Pw = dev_pwm(pwms); L.rec = d_rec; L.pos = d_pos; L.strand_mask = strand_mask;
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
        he = hipMemcpyAsync(d_chrom, chrom, 4 * (size_t) V, hipMemcpyHostToDevice, st);
        if (he == hipSuccess) he = hipMemcpyAsync(d_pos, pos, 8 * (size_t) V, hipMemcpyHostToDevice, st);
        if (he == hipSuccess) he = hipMemcpyAsync(d_rlen, ref_len, 4 * (size_t) V, hipMemcpyHostToDevice, st);
        if (he == hipSuccess) he = hipMemcpyAsync(d_aoff, alt_offsets, 8 * ((size_t) V + 1), hipMemcpyHostToDevice, st);
        if (he == hipSuccess && ref_bases) he = hipMemcpyAsync(d_roff, ref_off.data(), 8 * ((size_t) V + 1), hipMemcpyHostToDevice, st);
        if (he == hipSuccess && A > 0) he = hipMemcpyAsync(d_alt, alt_bases, (size_t) A, hipMemcpyHostToDevice, st);
        if (he == hipSuccess && Rn > 0) he = hipMemcpyAsync(d_ref, ref_bases, (size_t) Rn, hipMemcpyHostToDevice, st);
        if (he == hipSuccess) he = hipMemsetAsync(d_acode, 0, b_acode + b_amask, st);       // (the two planes lie side by side: their padding too)
        if (he == hipSuccess && A > 0) {
            hipLaunchKernelGGL(al_pack_kernel, dim3((unsigned) ((a_words + 255) / 256)), dim3(256), 0, st, d_alt, A, d_acode, d_amask);
            he = hipGetLastError();
        }
        if (he == hipSuccess) {
            hipLaunchKernelGGL(al_prep_kernel, dim3((unsigned) ((V + 255) / 256)), dim3(256), 0, st, G->d_codes, G->d_nmask, G->d_offsets, d_chrom, d_pos,
                               d_rlen, d_aoff, ref_bases ? d_ref : (const uint8_t *) nullptr, d_roff, V, d_rec, d_mis);
            he = hipGetLastError();
        }
        if (he == hipSuccess) he = hipMemcpyAsync(raw->mismatch.data(), d_mis, (size_t) V, hipMemcpyDeviceToHost, st);
        if (he != hipSuccess) return hip_fail(he, "variant upload");
    }
    he = hipMemsetAsync(d_gained, 0, 16 * Pz, st);
    if (he != hipSuccess) return hip_fail(he, "memset");
    const AlOut none{};

    // one chunk's counts and their prefix sums (tally: with the gained / lost numbers -- the first time only)
    auto count_chunk = [&](int64_t k, bool tally) -> int {
        const int64_t v0 = k * chunk, nv = std::min(chunk, V - v0), ntx = (nv + kAlTile - 1) / kAlTile;
        const size_t cells = (size_t) ntx * (size_t) P;
        hipError_t e = hipMemsetAsync(d_cnt, 0, 4 * (cells + 1), st);
        if (e != hipSuccess) { set_error("memset failed: %s", hipGetErrorString(e)); return MS_ERR_RUNTIME; }
        int r = launch_al_scan<false>(L, v0, nv, d_cnt, nullptr, nullptr, tally ? d_gained : nullptr, tally ? d_lost : nullptr, none, st);
        if (r) return r;
        size_t tmp = scan_tmp;
        return exclusive_sum_u32(d_tmp, &tmp, d_cnt, d_excl, cells + 1, st);
    };

    std::vector<uint64_t> h_tot, h_base;
    if (V > 0 && P > 0) {
        // ---- pass 1: every chunk counted
        for (int64_t k = 0; k < n_chunks; k++) {
            if ((rc = count_chunk(k, true))) return fail(rc);
            const int64_t nv = std::min(chunk, V - k * chunk), ntx = (nv + kAlTile - 1) / kAlTile;
            hipLaunchKernelGGL(al_row_total_kernel, dim3((unsigned) ((P + 255) / 256)), dim3(256), 0, st, d_excl, ntx, P, d_tot + (size_t) k * P);
            if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "row totals");
        }
        try { h_tot.resize((size_t) n_chunks * P); h_base.resize((size_t) n_chunks * P); }
        catch (const std::bad_alloc &) { set_error("out of host memory"); return fail(MS_ERR_NOMEM); }
        he = hipMemcpyAsync(h_tot.data(), d_tot, 8 * h_tot.size(), hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        if (he != hipSuccess) return hip_fail(he, "allele count pass");
        // ---- the motif offsets, and where every (chunk, motif) run of records starts
        uint64_t at = 0;
        for (int32_t m = 0; m < P; m++) {
            raw->motif_offsets[(size_t) m] = (int64_t) at;
            for (int64_t k = 0; k < n_chunks; k++) { h_base[(size_t) k * P + m] = at; at += h_tot[(size_t) k * P + m]; }
        }
        raw->motif_offsets[(size_t) P] = (int64_t) at;
        raw->n = (int64_t) at;
    }
    {
        const size_t n = (size_t) raw->n, nz = std::max<size_t>(n, 1);
        void *blk = nullptr;
        size_t got = 0;
        if ((rc = pool_alloc(c, 3 * al_up256(8 * nz) + 2 * al_up256(nz), &blk, &got))) return fail(rc);
        raw->block = blk;
        raw->block_bytes = got;
        char *p = static_cast<char *>(blk);
        raw->d_variant = reinterpret_cast<int64_t *>(p); p += al_up256(8 * nz);
        raw->d_start = reinterpret_cast<int64_t *>(p); p += al_up256(8 * nz);
        raw->d_score = reinterpret_cast<double *>(p); p += al_up256(8 * nz);
        raw->d_strand = reinterpret_cast<int8_t *>(p); p += al_up256(nz);
        raw->d_allele = reinterpret_cast<uint8_t *>(p);
    }
    if (raw->n > 0) {
        // ---- pass 2: every chunk filled (its counts made again unless they are still there)
        AlOut O;
        O.variant = raw->d_variant; O.start = raw->d_start; O.score = raw->d_score; O.strand = raw->d_strand; O.allele = raw->d_allele;
        O.cap = (uint64_t) raw->n;
        he = hipMemcpyAsync(d_base, h_base.data(), 8 * h_base.size(), hipMemcpyHostToDevice, st);
        if (he != hipSuccess) return hip_fail(he, "upload of the record offsets");
        for (int64_t k = 0; k < n_chunks; k++) {
            if (n_chunks > 1 && (rc = count_chunk(k, false))) return fail(rc);
            const int64_t v0 = k * chunk, nv = std::min(chunk, V - v0);
            if ((rc = launch_al_scan<true>(L, v0, nv, nullptr, d_excl, d_base + (size_t) k * P, nullptr, nullptr, O, st))) return fail(rc);
        }
    }
    (void) hipEventRecord(c->ev[1], st);
    he = hipSuccess;
    if (P > 0) he = hipMemcpyAsync(raw->gained.data(), d_gained, 8 * (size_t) P, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess && P > 0) he = hipMemcpyAsync(raw->lost.data(), d_lost, 8 * (size_t) P, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) return hip_fail(he, "allele scan");
    float ms01 = 0;
    (void) hipEventElapsedTime(&ms01, c->ev[0], c->ev[1]);
    raw->device_ms = ms01;
    pool_free(c, wblk, wgot);
    *out = raw;
    return MS_OK;
}

int ms_allelescan_num_sites(const ms_allelescan *r, int64_t *n) {
    if (!r || !n) { set_error("NULL argument"); return MS_ERR_INVALID; }
    *n = r->n;
    return MS_OK;
}

int ms_allelescan_motif_offsets(const ms_allelescan *r, int64_t *out) {
    if (!r || !out) { set_error("NULL argument"); return MS_ERR_INVALID; }
    std::copy(r->motif_offsets.begin(), r->motif_offsets.end(), out);
    return MS_OK;
}

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

int ms_allelescan_motif_counts(const ms_allelescan *r, int64_t *gained, int64_t *lost) {
    if (!r) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (gained) std::copy(r->gained.begin(), r->gained.end(), gained);
    if (lost) std::copy(r->lost.begin(), r->lost.end(), lost);
    return MS_OK;
}

int ms_allelescan_ref_mismatch(const ms_allelescan *r, uint8_t *out) {
    if (!r || (!out && r->V > 0)) { set_error("NULL argument"); return MS_ERR_INVALID; }
    std::copy(r->mismatch.begin(), r->mismatch.end(), out);
    return MS_OK;
}

int ms_allelescan_device_ms(const ms_allelescan *r, double *ms) {
    if (!r || !ms) { set_error("NULL argument"); return MS_ERR_INVALID; }
    *ms = r->device_ms;
    return MS_OK;
}

}  // extern "C"
