// ms_variants.hip -- motif sites gained and lost by single-base substitutions (ms_scan_variants), on a genome that is resident in HBM.
//
// For variant v = (chromosome, position x, alt byte a) and motif m of width W only the W windows that cover x matter: starts
// s = x - W + 1 + j, j = 0 .. W - 1, clipped to the chromosome.  Every such window is scored twice -- on the genome as it is and with base
// x replaced by a -- in the reference's order of operations (cscore.c:336-390; the scorer of ms_fp64.hip: columns 0 .. W - 1, forward
// M[b][c], reverse M[3 - b][W - 1 - c] at the same step, a non-ACGT base adds nothing, raw / max_raw, score - cutoff >= -1e-10).
// There is no pre-filter: the integer bound of ms_kernels.hip pays where a handful of 3 x 10^9 windows pass; here a motif has W windows
// per variant and both alleles' fp64 scores are part of the output of every window one of them passes.
//
// Mapping.  A work item is (variant, j); the items of a motif are numbered variant-major, so item order IS the output order (variant
// ascending, start ascending), and an item gives 0, 1 or 2 records ('+' before '-').  A block owns one motif and one TILE of kVarTile
// variants: it stages the motif's tab2 entries in LDS (a column is then one 16-byte broadcast read: <= 4 distinct addresses per wave),
// walks its kVarTile x W items in rounds of 256, and places the records of a round with a ballot prefix inside the wave and the waves'
// totals through LDS.  The alt allele differs from the ref allele in ONE column, k = x - s: its table entry is read once in front of
// the walk and selected at column k, so the four sums (two alleles x two strands) cost one table read and four fp64 adds per column.
//
// Order without a sort or an atomic: pass 1 (count) writes the number of records of every (motif, tile); an exclusive prefix sum over
// them and the per-motif totals give every block its place; pass 2 (fill) recomputes the scores and writes the records there.
// Variants are taken in CHUNKS so that the (motif, tile) counts stay bounded (kVarMaxTiles): all chunks are counted first, the
// per-(chunk, motif) totals are summed on the host into the motif offsets, then every chunk is filled (counted again when there is
// more than one chunk, the counts of the first pass being gone by then).
// The per-motif numbers of variants that gain / lose a site are counted in pass 1: a flag word per variant of the tile in LDS.
//
// The two passes over the chunks are place_records below, which ms_scan_alleles (ms_alleles.hip) drives with its own kernel; its host
// arithmetic -- the chunk plan, the offsets out of the totals, the layout of the work block -- is ms_place.h, and the accessors the two
// record handles have in common (RecHead, ms_handles.h) are implemented here once.  The kernel's column step, table staging, per-round
// placement and gained / lost tally are ms_allele_dev.h's (tab_step, tab_stage, place_round, tally_motif).
#include <algorithm>
#include <atomic>
#include <memory>

#include "ms_allele_dev.h"
#include "ms_device.h"
#include "ms_handles.h"

struct ms_varscan : ms::RecHead {
    int64_t *d_variant = nullptr;
    int64_t *d_start = nullptr;
    double *d_score_ref = nullptr;
    double *d_score_alt = nullptr;
    int8_t *d_strand = nullptr;
    uint8_t *d_state = nullptr;
    std::vector<int8_t> ref_codes;                    // [V]
};

namespace ms {

namespace {

constexpr int kVarTile = 128;                   // variants per block
constexpr int kVarThreads = 256;
constexpr int kVarTabMaxW = 1023;               // widest motif whose table (W x 4 entries + the zero one: 65 488 B) fits 64 KB; wider ones read it from HBM
                                                // (with the 544 B of static arrays a block then takes 66 032 B: above 64 KB, far below gfx950's 160 KB -- DESIGN.md)
constexpr int64_t kVarMaxTiles = 1LL << 24;     // (motif, tile) counts of one chunk: 64 MB of counts + 128 MB of their prefix sums
constexpr int32_t kVarFar = 1 << 30;

std::atomic<int64_t> g_var_chunk{0};            // ms_debug_varscan_chunk: variants per chunk, 0 = sized by kVarMaxTiles

struct VarRec {                                  // what an item needs of its variant, in one 16-byte read
    int64_t g;                                   // position of the variant in the packed genome
    int32_t lo;                                  // bases of the chromosome in front of it (clamped to kVarFar)
    int32_t hi;                                  // ... and behind it
};

struct VarOut {
    int64_t *variant, *start;
    double *score_ref, *score_alt;
    int8_t *strand;
    uint8_t *state;
    uint64_t cap;
};

// convert_seq (cscore.c:81-114) for the alt bytes; the ref base out of the planes; the variant's place
__global__ void __launch_bounds__(256) var_prep_kernel(const uint32_t *__restrict__ codes, const uint32_t *__restrict__ nmask,
                                                       const int64_t *__restrict__ offsets, const int32_t *__restrict__ chrom,
                                                       const int64_t *__restrict__ pos, const uint8_t *__restrict__ alt, int64_t V,
                                                       VarRec *__restrict__ rec, int8_t *__restrict__ alt_code, int8_t *__restrict__ ref_code) {
    const int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int64_t beg = offsets[chrom[v]], end = offsets[chrom[v] + 1], x = pos[v], g = beg + x;
    VarRec r;
    r.g = g;
    r.lo = (int32_t) (x < kVarFar ? x : kVarFar);
    r.hi = (int32_t) (end - 1 - g < kVarFar ? end - 1 - g : kVarFar);
    rec[v] = r;
    const uint32_t ch = (uint32_t) alt[v] | 0x20u;                                  // fold case (cscore.c:93-108)
    const bool acgt = ch == 0x61u || ch == 0x63u || ch == 0x67u || ch == 0x74u;
    alt_code[v] = acgt ? (int8_t) (((ch >> 1) ^ (ch >> 2)) & 3u) : (int8_t) -1;
    const uint32_t code = (codes[g >> 4] >> (2u * ((uint32_t) g & 15u))) & 3u;
    const uint32_t isn = (nmask[g >> 5] >> ((uint32_t) g & 31u)) & 1u;
    ref_code[v] = isn ? (int8_t) -1 : (int8_t) code;
}

// the reference's normalisation and hit test for the two alleles of one strand (cscore.c:356-358 / 373-375; test_and_emit of ms_fp64.hip:
// a raw sum below the motif's floor cannot pass, so the divides are paid only by windows of which an allele can).  Bit 0: ref passes,
// bit 1: alt passes.  Both passes of the scan call THIS, so the fill pass finds exactly the records the count pass counted.
__device__ __forceinline__ uint32_t judge(double raw_ref, double raw_alt, double max_raw, double cutoff, double floor_, double &s_ref, double &s_alt) {
    const bool try_r = !(raw_ref < floor_), try_a = !(raw_alt < floor_);
    s_ref = 0.0;
    s_alt = 0.0;
    if (!try_r && !try_a) return 0u;
    s_ref = raw_ref / max_raw;
    s_alt = raw_alt / max_raw;
    return ((try_r && s_ref - cutoff >= -1e-10) ? 1u : 0u) | ((try_a && s_alt - cutoff >= -1e-10) ? 2u : 0u);
}

// grid = (tiles of the chunk, motifs).  FILL = false: tile_cnt[motif][tile] = records of the tile, and (gained != nullptr) the motif's
// variants with a gained / a lost site; FILL = true: the records, from row_base[motif] + (tile_excl[motif][tile] - tile_excl[motif][0]) on.
// LDS_TAB: the motif's table in LDS (W <= kVarTabMaxW) or read from HBM (wider motifs); a block of the other kind leaves at once.
template <bool FILL, bool LDS_TAB>
__global__ void __launch_bounds__(kVarThreads) var_scan_kernel(const uint32_t *__restrict__ codes, const uint32_t *__restrict__ nmask, const DevPwm Pw,
                                                               const VarRec *__restrict__ rec, const int8_t *__restrict__ alt_code,
                                                               const int64_t *__restrict__ pos, int64_t v0, int64_t nv, int strand_mask,
                                                               uint32_t *__restrict__ tile_cnt, const uint64_t *__restrict__ tile_excl,
                                                               const uint64_t *__restrict__ row_base, unsigned long long *__restrict__ gained,
                                                               unsigned long long *__restrict__ lost, const VarOut O) {
    extern __shared__ double2 vtab_lds[];                      // [W * 4 + 1]: the motif's entries, and an all-zero one for the columns that add nothing
    __shared__ uint32_t s_wtot[2][kVarThreads / 64];
    __shared__ uint32_t s_flag[kVarTile];
    const int32_t m = (int32_t) blockIdx.y;
    const int W = Pw.width[m];
    if ((W <= kVarTabMaxW) != LDS_TAB) return;
    const double2 *__restrict__ tab_g = Pw.tab2 + Pw.tab_off[m];
    const uint32_t zero = (uint32_t) W * 4u;
    if (LDS_TAB) tab_stage<kVarThreads>(vtab_lds, tab_g, W);
    if (!FILL && threadIdx.x < kVarTile) s_flag[threadIdx.x] = 0u;
    __syncthreads();
    auto entry = [&](uint32_t idx) -> double2 {
        if constexpr (LDS_TAB) return vtab_lds[idx];
        else return tab_g[idx];
    };
    const int64_t tile = (int64_t) blockIdx.x, row = (int64_t) m * gridDim.x;
    const int64_t vl0 = tile * kVarTile;                       // first variant of the tile, in the chunk
    const int n_local = (int) (nv - vl0 < kVarTile ? nv - vl0 : kVarTile);
    const int64_t n_items = (int64_t) n_local * W;
    const double max_raw = Pw.max_raw[m], cutoff = Pw.cutoff[m], floor_ = Pw.raw_floor[m];
    uint64_t run = 0;                                          // records of the tile's earlier rounds (+ the tile's place when filling)
    if (FILL) run = row_base[m] + (tile_excl[row + tile] - tile_excl[row]);
    // item i = vl * W + j of thread t in round r: i = 256 r + t, kept as (vl, j) without a division per round
    int64_t vl = (int64_t) (threadIdx.x / (uint32_t) W);
    int j = (int) (threadIdx.x % (uint32_t) W);
    const int step_v = kVarThreads / W, step_j = kVarThreads % W;
    int round = 0;
    for (int64_t i0 = 0; i0 < n_items; i0 += kVarThreads, round++) {
        uint32_t st_f = 0u, st_r = 0u;
        double sf_ref = 0.0, sf_alt = 0.0, sr_ref = 0.0, sr_alt = 0.0;
        const int k = W - 1 - j;                               // the variant's column in this window
        if (i0 + threadIdx.x < n_items) {
            const VarRec vr = rec[v0 + vl0 + vl];
            if (k <= vr.lo && j <= vr.hi) {                    // the window lies inside the chromosome
                const int a = alt_code[v0 + vl0 + vl];
                const int64_t g = vr.g - k;
                double2 tk = make_double2(0.0, 0.0);           // what the alt allele adds at column k
                if (a >= 0) tk = entry((uint32_t) k * 4u + (uint32_t) a);
                double rf = 0.0, rr = 0.0, af = 0.0, ar = 0.0;
                for (int c0 = 0; c0 < W; c0 += 32) {
                    const uint64_t cw = code_window(codes, g + c0);
                    const int n = (W - c0) < 32 ? (W - c0) : 32;
                    tab_step<LDS_TAB, true>(vtab_lds, tab_g, zero, c0, n, cw, n_window(nmask, g + c0), k - c0, tk, rf, rr, af, ar);
                }
                if (strand_mask & 1) st_f = judge(rf, af, max_raw, cutoff, floor_, sf_ref, sf_alt);
                if (strand_mask & 2) st_r = judge(rr, ar, max_raw, cutoff, floor_, sr_ref, sr_alt);
            }
        }
        uint32_t before, all;
        place_round<kVarThreads>(s_wtot, round, st_f != 0u, st_r != 0u, before, all);
        if (FILL) {
            uint64_t d = run + before;
            const int64_t v = v0 + vl0 + vl;
            if (st_f && d < O.cap) {
                O.variant[d] = v; O.start[d] = pos[v] - k; O.strand[d] = (int8_t) 1;
                O.score_ref[d] = sf_ref; O.score_alt[d] = sf_alt; O.state[d] = (uint8_t) st_f;
            }
            d += st_f ? 1u : 0u;
            if (st_r && d < O.cap) {
                O.variant[d] = v; O.start[d] = pos[v] - k; O.strand[d] = (int8_t) 2;
                O.score_ref[d] = sr_ref; O.score_alt[d] = sr_alt; O.state[d] = (uint8_t) st_r;
            }
        } else if (gained) {
            const uint32_t bits = ((st_f == 1u || st_r == 1u) ? 1u : 0u) | ((st_f == 2u || st_r == 2u) ? 2u : 0u);
            if (bits) atomicOr(&s_flag[vl], bits);             // (an OR: the order of the writers cannot show)
        }
        run += all;
        vl += step_v;
        j += step_j;
        if (j >= W) { j -= W; vl++; }
    }
    if (!FILL) {
        if (threadIdx.x == 0) tile_cnt[row + tile] = (uint32_t) run;
        if (gained) {
            __syncthreads();
            const uint32_t f = (int) threadIdx.x < n_local ? s_flag[threadIdx.x] : 0u;
            tally_motif((f & 1u) != 0u, (f & 2u) != 0u, &lost[m], &gained[m]);
        }
    }
}

// tot[m] = records of motif m in the chunk, out of the prefix sums of its tiles (tile_excl has one entry more than there are tiles)
__global__ void __launch_bounds__(256) row_total_kernel(const uint64_t *__restrict__ tile_excl, int64_t ntx, int32_t P, uint64_t *__restrict__ tot) {
    const int32_t m = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    if (m < P) tot[m] = tile_excl[(int64_t) (m + 1) * ntx] - tile_excl[(int64_t) m * ntx];
}

struct VarLaunch {
    const ms_seqset *G;
    DevPwm Pw;
    const VarRec *rec;
    const int8_t *alt_code;
    const int64_t *pos;
    int strand_mask;
    int max_width, min_width;
    size_t lds;
};

template <bool FILL>
int launch_var_scan(const VarLaunch &L, int64_t v0, int64_t nv, uint32_t *tile_cnt, const uint64_t *tile_excl, const uint64_t *row_base,
                    unsigned long long *gained, unsigned long long *lost, const VarOut &O, hipStream_t st) {
    const dim3 grid((unsigned) ((nv + kVarTile - 1) / kVarTile), (unsigned) L.Pw.P);
    if (L.min_width <= kVarTabMaxW) {
        hipLaunchKernelGGL((var_scan_kernel<FILL, true>), grid, dim3(kVarThreads), L.lds, st, L.G->d_codes, L.G->d_nmask, L.Pw, L.rec, L.alt_code, L.pos,
                           v0, nv, L.strand_mask, tile_cnt, tile_excl, row_base, gained, lost, O);
        MS_HIP(hipGetLastError());
    }
    if (L.max_width > kVarTabMaxW) {
        hipLaunchKernelGGL((var_scan_kernel<FILL, false>), grid, dim3(kVarThreads), 0, st, L.G->d_codes, L.G->d_nmask, L.Pw, L.rec, L.alt_code, L.pos,
                           v0, nv, L.strand_mask, tile_cnt, tile_excl, row_base, gained, lost, O);
        MS_HIP(hipGetLastError());
    }
    return MS_OK;
}

}  // namespace

int64_t varscan_chunk_setting() { return g_var_chunk.load(); }

int place_slots(Carve &cv, const PlaceChunks &ch, int32_t P, hipStream_t st, PlaceSlots *out) {
    size_t tmp = 0;
    if (int rc = exclusive_sum_u32(nullptr, &tmp, nullptr, nullptr, ch.n_cells, st)) return rc;
    const size_t Pz = (size_t) std::max<int32_t>(P, 1), Kz = (size_t) std::max<int64_t>(ch.n_chunks, 1);
    out->cnt = cv.add<uint32_t>(ch.n_cells);
    out->excl = cv.add<uint64_t>(ch.n_cells);
    out->tot = cv.add<uint64_t>(Kz * Pz);
    out->base = cv.add<uint64_t>(Kz * Pz);
    out->gl = cv.add<unsigned long long>(2 * Pz);
    out->tmp = cv.add<char>(std::max<size_t>(tmp, 1));
    out->tmp_bytes = tmp;
    return MS_OK;
}

int place_records(DeviceCtx *c, const PlaceChunks &ch, int tile, void *work, const PlaceSlots &s, const char *what, const PlaceCalls &calls, RecHead *h) {
    const hipStream_t st = c->stream;
    const int32_t P = h->P;
    const int64_t V = h->V, chunk = ch.chunk, n_chunks = ch.n_chunks;
    uint32_t *d_cnt = Carve::at(work, s.cnt);
    uint64_t *d_excl = Carve::at(work, s.excl), *d_tot = Carve::at(work, s.tot), *d_base = Carve::at(work, s.base);
    unsigned long long *d_gained = Carve::at(work, s.gl), *d_lost = d_gained + std::max<int32_t>(P, 1);
    void *d_tmp = Carve::at(work, s.tmp);
    auto hip_err = [&](hipError_t e, const char *op) { set_error("%s failed: %s", op, hipGetErrorString(e)); return e == hipErrorOutOfMemory ? MS_ERR_NOMEM : MS_ERR_RUNTIME; };
    hipError_t he = hipMemsetAsync(d_gained, 0, 16 * (size_t) std::max<int32_t>(P, 1), st);
    if (he != hipSuccess) return hip_err(he, "memset");

    // one chunk's counts and their prefix sums (tally: with the gained / lost numbers -- the first time only)
    auto count_chunk = [&](int64_t k, bool tally) -> int {
        const int64_t v0 = k * chunk, nv = std::min(chunk, V - v0), ntx = (nv + tile - 1) / tile;
        const size_t cells = (size_t) ntx * (size_t) P;
        const hipError_t e = hipMemsetAsync(d_cnt, 0, 4 * (cells + 1), st);
        if (e != hipSuccess) return hip_err(e, "memset");
        if (int r = calls.count(v0, nv, d_cnt, tally ? d_gained : nullptr, tally ? d_lost : nullptr)) return r;
        size_t tmp = s.tmp_bytes;
        return exclusive_sum_u32(d_tmp, &tmp, d_cnt, d_excl, cells + 1, st);
    };

    int rc;
    std::vector<uint64_t> h_tot, h_base;
    if (V > 0 && P > 0) {
        // ---- pass 1: every chunk counted
        for (int64_t k = 0; k < n_chunks; k++) {
            if ((rc = count_chunk(k, true))) return rc;
            const int64_t nv = std::min(chunk, V - k * chunk), ntx = (nv + tile - 1) / tile;
            hipLaunchKernelGGL(row_total_kernel, dim3((unsigned) ((P + 255) / 256)), dim3(256), 0, st, d_excl, ntx, P, d_tot + (size_t) k * P);
            if ((he = hipGetLastError()) != hipSuccess) return hip_err(he, "row totals");
        }
        try { h_tot.resize((size_t) n_chunks * P); h_base.resize((size_t) n_chunks * P); }
        catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }
        he = hipMemcpyAsync(h_tot.data(), d_tot, 8 * h_tot.size(), hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        if (he != hipSuccess) { set_error("%s count pass failed: %s", what, hipGetErrorString(he)); return he == hipErrorOutOfMemory ? MS_ERR_NOMEM : MS_ERR_RUNTIME; }
        // ---- the motif offsets, and where every (chunk, motif) run of records starts
        h->n = (int64_t) place_offsets(h_tot.data(), n_chunks, P, h->motif_offsets.data(), h_base.data());
    }
    if ((rc = calls.alloc((size_t) h->n))) return rc;
    if (h->n > 0) {
        // ---- pass 2: every chunk filled (its counts made again unless they are still there)
        he = hipMemcpyAsync(d_base, h_base.data(), 8 * h_base.size(), hipMemcpyHostToDevice, st);
        if (he != hipSuccess) return hip_err(he, "upload of the record offsets");
        for (int64_t k = 0; k < n_chunks; k++) {
            if (n_chunks > 1 && (rc = count_chunk(k, false))) return rc;
            const int64_t v0 = k * chunk, nv = std::min(chunk, V - v0);
            if ((rc = calls.fill(v0, nv, d_excl, d_base + (size_t) k * P))) return rc;
        }
    }
    (void) hipEventRecord(c->ev[1], st);
    he = hipSuccess;
    if (P > 0) he = hipMemcpyAsync(h->gained.data(), d_gained, 8 * (size_t) P, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess && P > 0) he = hipMemcpyAsync(h->lost.data(), d_lost, 8 * (size_t) P, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) { set_error("%s scan failed: %s", what, hipGetErrorString(he)); return he == hipErrorOutOfMemory ? MS_ERR_NOMEM : MS_ERR_RUNTIME; }
    float ms01 = 0;
    (void) hipEventElapsedTime(&ms01, c->ev[0], c->ev[1]);
    h->device_ms = ms01;
    return MS_OK;
}

void rec_release(RecHead *h) {
    if (!h || !h->block) return;
    (void) hipSetDevice(h->device);
    DeviceCtx *c = nullptr;
    if (get_ctx(h->device, &c) == MS_OK) pool_free(c, h->block, h->block_bytes); else (void) hipFree(h->block);
    h->block = nullptr;
}

int rec_num_sites(const RecHead *h, int64_t *n) {
    if (!h || !n) { set_error("NULL argument"); return MS_ERR_INVALID; }
    *n = h->n;
    return MS_OK;
}

int rec_motif_offsets(const RecHead *h, int64_t *out) {
    if (!h || !out) { set_error("NULL argument"); return MS_ERR_INVALID; }
    std::copy(h->motif_offsets.begin(), h->motif_offsets.end(), out);
    return MS_OK;
}

int rec_motif_counts(const RecHead *h, int64_t *gained, int64_t *lost) {
    if (!h) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (gained) std::copy(h->gained.begin(), h->gained.end(), gained);
    if (lost) std::copy(h->lost.begin(), h->lost.end(), lost);
    return MS_OK;
}

int rec_device_ms(const RecHead *h, double *ms) {
    if (!h || !ms) { set_error("NULL argument"); return MS_ERR_INVALID; }
    *ms = h->device_ms;
    return MS_OK;
}

}  // namespace ms

using namespace ms;

extern "C" {

int ms_debug_varscan_chunk(int64_t n_variants, int64_t *previous) {
    if (n_variants < 0) { set_error("chunk size must be >= 0 (0 = the library's own)"); return MS_ERR_INVALID; }
    const int64_t old = g_var_chunk.exchange(n_variants);
    if (previous) *previous = old;
    return MS_OK;
}

int ms_debug_varscan_dims(int32_t out[6]) {
    if (!out) { set_error("NULL argument"); return MS_ERR_INVALID; }
    out[0] = kVarTile;
    out[1] = kVarThreads;
    out[2] = kVarTabMaxW;
    allelescan_dims(out + 3);
    return MS_OK;
}

void ms_varscan_free(ms_varscan *r) {
    rec_release(r);
    delete r;
}

int ms_scan_variants(const ms_pwmset *pwms_c, const ms_genome *genome, const int32_t *chrom, const int64_t *pos, const char *alt,
                     int64_t n_variants, int strand_mask, uint32_t flags, ms_varscan **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    if (strand_mask < 1 || strand_mask > 3) { set_error("invalid strand mask %d (1 '+', 2 '-', 3 both)", strand_mask); return MS_ERR_INVALID; }
    if (flags != 0u) { set_error("unknown variant scan flags 0x%x", flags); return MS_ERR_INVALID; }
    if (!require_device()) return MS_ERR_RUNTIME;
    if (!pwms_c || !genome) { set_error("NULL handle"); return MS_ERR_INVALID; }
    if (n_variants < 0 || (n_variants > 0 && (!chrom || !pos || !alt))) { set_error("bad variant arrays"); return MS_ERR_INVALID; }
    ms_pwmset *pwms = const_cast<ms_pwmset *>(pwms_c);
    const ms_seqset *G = reinterpret_cast<const ms_seqset *>(genome);
    const int64_t V = n_variants, n_chroms = G->R;
    const int32_t P = pwms->P;
    const int64_t *goff = G->offsets.data();
    for (int64_t v = 0; v < V; v++) {
        if (chrom[v] < 0 || chrom[v] >= n_chroms) { set_error("variant %lld: chromosome index %d out of range", (long long) v, chrom[v]); return MS_ERR_INVALID; }
        const int64_t len = goff[chrom[v] + 1] - goff[chrom[v]];
        if (pos[v] < 0 || pos[v] >= len) {
            set_error("variant %lld: position %lld is outside chromosome %d of length %lld", (long long) v, (long long) pos[v], chrom[v], (long long) len);
            return MS_ERR_INVALID;
        }
    }
    DeviceCtx *c;
    int rc = get_ctx(G->device, &c);
    if (rc) return rc;
    std::unique_ptr<ms_varscan> res(new (std::nothrow) ms_varscan());
    if (!res) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    try {
        res->motif_offsets.assign((size_t) P + 1, 0);
        res->gained.assign((size_t) P, 0);
        res->lost.assign((size_t) P, 0);
        res->ref_codes.assign((size_t) V, 0);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    res->device = c->device;
    res->P = P;
    res->V = V;
    std::lock_guard<std::mutex> lk_dev(c->mu);
    std::lock_guard<std::mutex> lk_pwm(pwms->mu);
    if ((rc = pwmset_upload(pwms, c->device, c->stream))) return rc;
    const hipStream_t st = c->stream;

    // ---- chunks of variants: at most kVarMaxTiles (motif, tile) counts at a time
    const PlaceChunks ch = place_chunks(V, P, kVarTile, kVarMaxTiles, g_var_chunk.load());
    const size_t Vz = (size_t) std::max<int64_t>(V, 1);
    Carve cv;
    const auto s_chrom = cv.add<int32_t>(Vz);
    const auto s_pos = cv.add<int64_t>(Vz);
    const auto s_alt = cv.add<uint8_t>(Vz);
    const auto s_rec = cv.add<VarRec>(Vz);
    const auto s_altc = cv.add<int8_t>(Vz), s_refc = cv.add<int8_t>(Vz);
    PlaceSlots ps;
    if ((rc = place_slots(cv, ch, P, st, &ps))) return rc;
    void *wblk = nullptr;
    size_t wgot = 0;
    if ((rc = pool_alloc(c, cv.bytes(), &wblk, &wgot))) return rc;
    int32_t *d_chrom = Carve::at(wblk, s_chrom);
    int64_t *d_pos = Carve::at(wblk, s_pos);
    uint8_t *d_alt = Carve::at(wblk, s_alt);
    VarRec *d_rec = Carve::at(wblk, s_rec);
    int8_t *d_altc = Carve::at(wblk, s_altc), *d_refc = Carve::at(wblk, s_refc);
    ms_varscan *raw = res.release();
    auto fail = [&](int code) { (void) hipStreamSynchronize(st); pool_free(c, wblk, wgot); ms_varscan_free(raw); return code; };   // (nothing queued may still read the blocks)
    auto hip_fail = [&](hipError_t e, const char *what) { set_error("%s failed: %s", what, hipGetErrorString(e)); return fail(e == hipErrorOutOfMemory ? MS_ERR_NOMEM : MS_ERR_RUNTIME); };

    VarLaunch L;
    L.G = G; L.Pw = dev_pwm(pwms); L.rec = d_rec; L.alt_code = d_altc; L.pos = d_pos; L.strand_mask = strand_mask;
    L.max_width = pwms->max_width;
    L.min_width = P > 0 ? *std::min_element(pwms->widths.begin(), pwms->widths.end()) : 0;
    int lds_width = 0;
    for (int32_t p = 0; p < P; p++) if (pwms->widths[p] <= kVarTabMaxW) lds_width = std::max(lds_width, (int) pwms->widths[p]);
    L.lds = ((size_t) lds_width * 4 + 1) * sizeof(double2);
    hipError_t he = hipSuccess;
    if (L.lds > 48 * 1024) {                                   // (motifs of more than 767 columns: rare enough to ask the driver every time)
        he = hipFuncSetAttribute(reinterpret_cast<const void *>(var_scan_kernel<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int) L.lds);
        if (he == hipSuccess) he = hipFuncSetAttribute(reinterpret_cast<const void *>(var_scan_kernel<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int) L.lds);
        if (he != hipSuccess) return hip_fail(he, "raising the LDS limit");
    }

    (void) hipEventRecord(c->ev[0], st);
    if (V > 0) {
        he = hipMemcpyAsync(d_chrom, chrom, 4 * (size_t) V, hipMemcpyHostToDevice, st);
        if (he == hipSuccess) he = hipMemcpyAsync(d_pos, pos, 8 * (size_t) V, hipMemcpyHostToDevice, st);
        if (he == hipSuccess) he = hipMemcpyAsync(d_alt, alt, (size_t) V, hipMemcpyHostToDevice, st);
        if (he == hipSuccess) {
            hipLaunchKernelGGL(var_prep_kernel, dim3((unsigned) ((V + 255) / 256)), dim3(256), 0, st, G->d_codes, G->d_nmask, G->d_offsets, d_chrom, d_pos,
                               d_alt, V, d_rec, d_altc, d_refc);
            he = hipGetLastError();
        }
        if (he == hipSuccess) he = hipMemcpyAsync(raw->ref_codes.data(), d_refc, (size_t) V, hipMemcpyDeviceToHost, st);
        if (he != hipSuccess) return hip_fail(he, "variant upload");
    }

    VarOut O{};                                                // (no arrays while counting)
    PlaceCalls calls;
    calls.count = [&](int64_t v0, int64_t nv, uint32_t *tile_cnt, unsigned long long *gained, unsigned long long *lost) {
        return launch_var_scan<false>(L, v0, nv, tile_cnt, nullptr, nullptr, gained, lost, O, st);
    };
    calls.fill = [&](int64_t v0, int64_t nv, const uint64_t *tile_excl, const uint64_t *row_base) {
        return launch_var_scan<true>(L, v0, nv, nullptr, tile_excl, row_base, nullptr, nullptr, O, st);
    };
    calls.alloc = [&](size_t n) {
        const size_t nz = std::max<size_t>(n, 1);
        Carve rv;
        const auto s_variant = rv.add<int64_t>(nz), s_start = rv.add<int64_t>(nz);
        const auto s_sref = rv.add<double>(nz), s_salt = rv.add<double>(nz);
        const auto s_strand = rv.add<int8_t>(nz);
        const auto s_state = rv.add<uint8_t>(nz);
        void *blk = nullptr;
        size_t got = 0;
        if (int r = pool_alloc(c, rv.bytes(), &blk, &got)) return r;
        raw->block = blk;
        raw->block_bytes = got;
        O.variant = raw->d_variant = Carve::at(blk, s_variant);
        O.start = raw->d_start = Carve::at(blk, s_start);
        O.score_ref = raw->d_score_ref = Carve::at(blk, s_sref);
        O.score_alt = raw->d_score_alt = Carve::at(blk, s_salt);
        O.strand = raw->d_strand = Carve::at(blk, s_strand);
        O.state = raw->d_state = Carve::at(blk, s_state);
        O.cap = (uint64_t) n;
        return MS_OK;
    };
    if ((rc = place_records(c, ch, kVarTile, wblk, ps, "variant", calls, raw))) return fail(rc);
    pool_free(c, wblk, wgot);
    *out = raw;
    return MS_OK;
}

int ms_varscan_num_sites(const ms_varscan *r, int64_t *n) { return rec_num_sites(r, n); }
int ms_varscan_motif_offsets(const ms_varscan *r, int64_t *out) { return rec_motif_offsets(r, out); }
int ms_varscan_motif_counts(const ms_varscan *r, int64_t *gained, int64_t *lost) { return rec_motif_counts(r, gained, lost); }
int ms_varscan_device_ms(const ms_varscan *r, double *ms) { return rec_device_ms(r, ms); }

int ms_varscan_sites(const ms_varscan *r, int64_t *variant, int64_t *start, int8_t *strand, double *score_ref, double *score_alt, uint8_t *state) {
    if (!r) { set_error("NULL argument"); return MS_ERR_INVALID; }
    const size_t n = (size_t) r->n;
    if (n == 0) return MS_OK;
    MS_HIP(hipSetDevice(r->device));
    if (variant) MS_HIP(hipMemcpy(variant, r->d_variant, 8 * n, hipMemcpyDeviceToHost));
    if (start) MS_HIP(hipMemcpy(start, r->d_start, 8 * n, hipMemcpyDeviceToHost));
    if (strand) MS_HIP(hipMemcpy(strand, r->d_strand, n, hipMemcpyDeviceToHost));
    if (score_ref) MS_HIP(hipMemcpy(score_ref, r->d_score_ref, 8 * n, hipMemcpyDeviceToHost));
    if (score_alt) MS_HIP(hipMemcpy(score_alt, r->d_score_alt, 8 * n, hipMemcpyDeviceToHost));
    if (state) MS_HIP(hipMemcpy(state, r->d_state, n, hipMemcpyDeviceToHost));
    return MS_OK;
}

int ms_varscan_ref_codes(const ms_varscan *r, int8_t *out) {
    if (!r || (!out && r->V > 0)) { set_error("NULL argument"); return MS_ERR_INVALID; }
    std::copy(r->ref_codes.begin(), r->ref_codes.end(), out);
    return MS_OK;
}

}  // extern "C"
