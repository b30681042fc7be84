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
#include <algorithm>
#include <atomic>
#include <memory>
#include <type_traits>

#include "ms_device.h"
#include "ms_handles.h"

struct ms_varscan {
    int device = 0;
    int32_t P = 0;
    int64_t V = 0;
    int64_t n = 0;                                    // records
    void *block = nullptr;                            // one pooled device block holding the record arrays
    size_t block_bytes = 0;
    int64_t *d_variant = nullptr;
    int64_t *d_start = nullptr;
    double *d_score_ref = nullptr;
    double *d_score_alt = nullptr;
    int8_t *d_strand = nullptr;
    uint8_t *d_state = nullptr;
    std::vector<int64_t> motif_offsets;               // [P+1]
    std::vector<int64_t> gained, lost;                // [P], counted on the device
    std::vector<int8_t> ref_codes;                    // [V]
    double device_ms = 0.0;                           // first launch -> last kernel done
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
    if (LDS_TAB) {
        for (int i = threadIdx.x; i < W * 4; i += kVarThreads) vtab_lds[i] = tab_g[i];
        if (threadIdx.x == 0) vtab_lds[zero] = make_double2(0.0, 0.0);
    }
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
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t lt = (1ULL << lane) - 1ULL;
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
                    const uint32_t skip = n_window(nmask, g + c0) | ~low_mask(n);       // bit c: column c0 + c adds nothing
                    const int kk = k - c0;
                    // eight columns a step while more than four are left, then four: the reads of a step are issued together
                    auto columns = [&](auto width, int c1) {
                        constexpr int N = decltype(width)::value;
                        double2 t[N];
#pragma unroll
                        for (int u = 0; u < N; u++) {
                            const int c = c1 + u;
                            const bool nothing = (skip >> c) & 1u;                          // adds +0.0: a sum that started at +0.0 is never -0.0
                            if constexpr (LDS_TAB) {
                                t[u] = vtab_lds[nothing ? zero : (uint32_t) (c0 + c) * 4u + ((uint32_t) (cw >> (2 * c)) & 3u)];
                            } else {
                                const int cc = c < n ? c : n - 1;                           // clamped: always an entry of the motif
                                t[u] = tab_g[(uint32_t) (c0 + cc) * 4u + ((uint32_t) (cw >> (2 * cc)) & 3u)];
                                if (nothing) t[u] = make_double2(0.0, 0.0);
                            }
                        }
#pragma unroll
                        for (int u = 0; u < N; u++) {
                            const double2 ta = (c1 + u == kk) ? tk : t[u];
                            rf += t[u].x; rr += t[u].y;
                            af += ta.x; ar += ta.y;
                        }
                    };
                    int c1 = 0;
                    for (; n - c1 > 4; c1 += 8) columns(std::integral_constant<int, 8>{}, c1);
                    if (n - c1 > 0) columns(std::integral_constant<int, 4>{}, c1);
                }
                if (strand_mask & 1) st_f = judge(rf, af, max_raw, cutoff, floor_, sf_ref, sf_alt);
                if (strand_mask & 2) st_r = judge(rr, ar, max_raw, cutoff, floor_, sr_ref, sr_alt);
            }
        }
        const unsigned long long bf = __ballot(st_f != 0u), br = __ballot(st_r != 0u);
        const int buf = round & 1;                             // (two buffers: a wave may write round r + 1's total while another still reads round r's)
        if (lane == 0u) s_wtot[buf][wave] = (uint32_t) (__popcll(bf) + __popcll(br));
        __syncthreads();
        uint32_t before = 0u, all = 0u;
#pragma unroll
        for (uint32_t w = 0; w < (uint32_t) (kVarThreads / 64); w++) {
            const uint32_t x = s_wtot[buf][w];
            all += x;
            if (w < wave) before += x;
        }
        if (FILL) {
            uint64_t d = run + before + (uint64_t) (__popcll(bf & lt) + __popcll(br & lt));
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
            const unsigned long long bl = __ballot((f & 1u) != 0u), bg = __ballot((f & 2u) != 0u);
            if (lane == 0u) {
                if (bl) atomicAdd(&lost[m], (unsigned long long) __popcll(bl));            // (integer sums: the same in any order)
                if (bg) atomicAdd(&gained[m], (unsigned long long) __popcll(bg));
            }
        }
    }
}

// tot[m] = records of motif m in the chunk, out of the prefix sums of its tiles (tile_excl has one entry more than there are tiles)
__global__ void __launch_bounds__(256) var_row_total_kernel(const uint64_t *__restrict__ tile_excl, int64_t ntx, int32_t P, uint64_t *__restrict__ tot) {
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

size_t up256(size_t x) { return (x + 255) & ~(size_t) 255; }

}  // namespace

int64_t varscan_chunk_setting() { return g_var_chunk.load(); }

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
    if (!r) return;
    if (r->block) {
        (void) hipSetDevice(r->device);
        DeviceCtx *c = nullptr;
        if (get_ctx(r->device, &c) == MS_OK) pool_free(c, r->block, r->block_bytes); else (void) hipFree(r->block);
    }
    delete r;
}

int ms_scan_variants(const ms_pwmset *pwms_c, const ms_genome *genome, const int32_t *chrom, const int64_t *pos, const char *alt,
                     int64_t n_variants, int strand_mask, uint32_t flags, ms_varscan **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    if (strand_mask < 1 || strand_mask > 3) { set_error("invalid strand mask %d (1 '+', 2 '-', 3 both)", strand_mask); return MS_ERR_INVALID; }
    if (flags != 0u) { set_error("unknown variant scan flags 0x%x", flags); return MS_ERR_INVALID; }
    {
        int n_dev = 0;                                         // (a genome handle cannot exist without a device: say so before asking for one)
        if (ms_device_count(&n_dev) != MS_OK || n_dev <= 0) { set_error("no usable HIP device; libmotifscan_amd has no CPU fallback"); return MS_ERR_RUNTIME; }
    }
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
    int64_t chunk = g_var_chunk.load();
    if (chunk <= 0) chunk = std::max<int64_t>(1, kVarMaxTiles / std::max<int32_t>(P, 1)) * kVarTile;
    chunk = std::min<int64_t>(chunk, std::max<int64_t>(V, 1));
    const int64_t n_chunks = V > 0 ? (V + chunk - 1) / chunk : 0;
    const int64_t ntx_max = (chunk + kVarTile - 1) / kVarTile;
    const size_t n_cells = (size_t) ntx_max * (size_t) std::max<int32_t>(P, 1) + 1;

    size_t scan_tmp = 0;
    if ((rc = exclusive_sum_u32(nullptr, &scan_tmp, nullptr, nullptr, n_cells, st))) return rc;
    const size_t Vz = (size_t) std::max<int64_t>(V, 1), Pz = (size_t) std::max<int32_t>(P, 1), Kz = (size_t) std::max<int64_t>(n_chunks, 1);
    const size_t b_chrom = up256(4 * Vz), b_pos = up256(8 * Vz), b_alt = up256(Vz), b_rec = up256(sizeof(VarRec) * Vz), b_altc = up256(Vz),
                 b_refc = up256(Vz), b_cnt = up256(4 * n_cells), b_excl = up256(8 * n_cells), b_tot = up256(8 * Kz * Pz), b_gl = up256(16 * Pz),
                 b_tmp = up256(std::max<size_t>(scan_tmp, 1));
    void *wblk = nullptr;
    size_t wgot = 0;
    if ((rc = pool_alloc(c, b_chrom + b_pos + b_alt + b_rec + b_altc + b_refc + b_cnt + b_excl + 2 * b_tot + b_gl + b_tmp, &wblk, &wgot))) return rc;
    char *b = static_cast<char *>(wblk);
    int32_t *d_chrom = reinterpret_cast<int32_t *>(b); b += b_chrom;
    int64_t *d_pos = reinterpret_cast<int64_t *>(b); b += b_pos;
    uint8_t *d_alt = reinterpret_cast<uint8_t *>(b); b += b_alt;
    VarRec *d_rec = reinterpret_cast<VarRec *>(b); b += b_rec;
    int8_t *d_altc = reinterpret_cast<int8_t *>(b); b += b_altc;
    int8_t *d_refc = reinterpret_cast<int8_t *>(b); b += b_refc;
    uint32_t *d_cnt = reinterpret_cast<uint32_t *>(b); b += b_cnt;
    uint64_t *d_excl = reinterpret_cast<uint64_t *>(b); b += b_excl;
    uint64_t *d_tot = reinterpret_cast<uint64_t *>(b); b += b_tot;          // [chunks][P] records of the motif in the chunk
    uint64_t *d_base = reinterpret_cast<uint64_t *>(b); b += b_tot;         // [chunks][P] where they go
    unsigned long long *d_gained = reinterpret_cast<unsigned long long *>(b);
    unsigned long long *d_lost = d_gained + Pz; b += b_gl;
    void *d_tmp = b;
    ms_varscan *raw = res.release();
    auto fail = [&](int code) { pool_free(c, wblk, wgot); ms_varscan_free(raw); return code; };
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
    he = hipMemsetAsync(d_gained, 0, 16 * Pz, st);
    if (he != hipSuccess) return hip_fail(he, "memset");
    const VarOut none{};

    // one chunk's counts and their prefix sums (tally: with the gained / lost numbers -- the first time only)
    auto count_chunk = [&](int64_t k, bool tally) -> int {
        const int64_t v0 = k * chunk, nv = std::min(chunk, V - v0), ntx = (nv + kVarTile - 1) / kVarTile;
        const size_t cells = (size_t) ntx * (size_t) P;
        hipError_t e = hipMemsetAsync(d_cnt, 0, 4 * (cells + 1), st);
        if (e != hipSuccess) { set_error("memset failed: %s", hipGetErrorString(e)); return MS_ERR_RUNTIME; }
        int r = launch_var_scan<false>(L, v0, nv, d_cnt, nullptr, nullptr, tally ? d_gained : nullptr, tally ? d_lost : nullptr, none, st);
        if (r) return r;
        size_t tmp = scan_tmp;
        return exclusive_sum_u32(d_tmp, &tmp, d_cnt, d_excl, cells + 1, st);
    };

    std::vector<uint64_t> h_tot, h_base;
    if (V > 0 && P > 0) {
        // ---- pass 1: every chunk counted
        for (int64_t k = 0; k < n_chunks; k++) {
            if ((rc = count_chunk(k, true))) return fail(rc);
            const int64_t nv = std::min(chunk, V - k * chunk), ntx = (nv + kVarTile - 1) / kVarTile;
            hipLaunchKernelGGL(var_row_total_kernel, dim3((unsigned) ((P + 255) / 256)), dim3(256), 0, st, d_excl, ntx, P, d_tot + (size_t) k * P);
            if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "row totals");
        }
        try { h_tot.resize((size_t) n_chunks * P); h_base.resize((size_t) n_chunks * P); }
        catch (const std::bad_alloc &) { set_error("out of host memory"); return fail(MS_ERR_NOMEM); }
        he = hipMemcpyAsync(h_tot.data(), d_tot, 8 * h_tot.size(), hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        if (he != hipSuccess) return hip_fail(he, "variant count pass");
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
        if ((rc = pool_alloc(c, 4 * up256(8 * nz) + 2 * up256(nz), &blk, &got))) return fail(rc);
        raw->block = blk;
        raw->block_bytes = got;
        char *p = static_cast<char *>(blk);
        raw->d_variant = reinterpret_cast<int64_t *>(p); p += up256(8 * nz);
        raw->d_start = reinterpret_cast<int64_t *>(p); p += up256(8 * nz);
        raw->d_score_ref = reinterpret_cast<double *>(p); p += up256(8 * nz);
        raw->d_score_alt = reinterpret_cast<double *>(p); p += up256(8 * nz);
        raw->d_strand = reinterpret_cast<int8_t *>(p); p += up256(nz);
        raw->d_state = reinterpret_cast<uint8_t *>(p);
    }
    if (raw->n > 0) {
        // ---- pass 2: every chunk filled (its counts made again unless they are still there)
        VarOut O;
        O.variant = raw->d_variant; O.start = raw->d_start; O.score_ref = raw->d_score_ref; O.score_alt = raw->d_score_alt;
        O.strand = raw->d_strand; O.state = raw->d_state; O.cap = (uint64_t) raw->n;
        he = hipMemcpyAsync(d_base, h_base.data(), 8 * h_base.size(), hipMemcpyHostToDevice, st);
        if (he != hipSuccess) return hip_fail(he, "upload of the record offsets");
        for (int64_t k = 0; k < n_chunks; k++) {
            if (n_chunks > 1 && (rc = count_chunk(k, false))) return fail(rc);
            const int64_t v0 = k * chunk, nv = std::min(chunk, V - v0);
            if ((rc = launch_var_scan<true>(L, v0, nv, nullptr, d_excl, d_base + (size_t) k * P, nullptr, nullptr, O, st))) return fail(rc);
        }
    }
    (void) hipEventRecord(c->ev[1], st);
    he = hipSuccess;
    if (P > 0) he = hipMemcpyAsync(raw->gained.data(), d_gained, 8 * (size_t) P, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess && P > 0) he = hipMemcpyAsync(raw->lost.data(), d_lost, 8 * (size_t) P, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) return hip_fail(he, "variant scan");
    float ms01 = 0;
    (void) hipEventElapsedTime(&ms01, c->ev[0], c->ev[1]);
    raw->device_ms = ms01;
    pool_free(c, wblk, wgot);
    *out = raw;
    return MS_OK;
}

int ms_varscan_num_sites(const ms_varscan *r, int64_t *n) {
    if (!r || !n) { set_error("NULL argument"); return MS_ERR_INVALID; }
    *n = r->n;
    return MS_OK;
}

int ms_varscan_motif_offsets(const ms_varscan *r, int64_t *out) {
    if (!r || !out) { set_error("NULL argument"); return MS_ERR_INVALID; }
    std::copy(r->motif_offsets.begin(), r->motif_offsets.end(), out);
    return MS_OK;
}

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

int ms_varscan_motif_counts(const ms_varscan *r, int64_t *gained, int64_t *lost) {
    if (!r) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (gained) std::copy(r->gained.begin(), r->gained.end(), gained);
    if (lost) std::copy(r->lost.begin(), r->lost.end(), lost);
    return MS_OK;
}

int ms_varscan_device_ms(const ms_varscan *r, double *ms) {
    if (!r || !ms) { set_error("NULL argument"); return MS_ERR_INVALID; }
    *ms = r->device_ms;
    return MS_OK;
}

}  // extern "C"
