// ms_personal.hip -- a personal haplotype as a resident genome (ms_genome_apply_alleles): a whole variant set spliced into a NEW packed
// genome on the device, and the map between the two coordinate systems (ms_liftmap).  The output is an ordinary ms_genome, so every
// region-based entry point runs on it unchanged.
//
// Everything below works in PACKED coordinates: the chromosomes lie back to back in the planes (ms_device.h), variant v = (chromosome c, x, r,
// alt[0..a)) sits at g = offsets[c] + x, and the output genome is again the concatenation of its chromosomes.  So the splice is ONE
// sequence edited at sorted, disjoint places, and the chromosome table is carried along by the prefix sums.
//
// Order and the overlap rule.  Key K_v = g_v + c_v orders by (chromosome, x): g alone does not -- an insertion at x = L_c has the g of
// x = 0 of chromosome c + 1 -- and it needs 36 bits, not 64.  A stable radix sort of (K, index) gives the order (chromosome, x, index).
// With E_v = g_v + r_v + c_v, variant v overlaps an earlier one iff the maximum of E over the variants in front of it exceeds K_v (an end
// in an earlier chromosome is at most offsets[c] + c - 1 < K_v: it never counts): an inclusive max-scan, read one place to the left.  Under
// MS_APPLY_SKIP_MISMATCH a variant whose REF differs gets the key past every other and E = 0: it sorts behind and blocks nothing.
//
// Layout.  The applied variants are compacted in order (flags, exclusive sum), D_j = the exclusive sum of a - r over them, and
//     os_j = g_j + D_j   is where alt_j starts in the output;   os_j + a_j <= os_(j+1)   because   g_j + r_j <= g_(j+1).
// That IS the segment table, of 2 n + 1 pieces -- genome [.., g_0), alt_0, genome [g_0 + r_0, g_1), alt_1, ... : output base p with
// j = the last variant with os_j <= p lies in alt_j at aoff_j + (p - os_j) if p < os_j + a_j, else in the genome at g_j + r_j + (p - os_j -
// a_j); in front of os_0 it is genome base p.  A genome piece may run across chromosome ends: the planes have no gap there.  New chromosome
// offsets: offsets[c] + D at the first applied variant of a chromosome >= c -- the one small copy back to the host, which sizes the output.
//
// Splice kernel (the hot path): extract_kernel's shape (ms_seqset.hip) -- a thread per 32 output bases ORs masked, shifted code_window /
// n_window reads of the genome planes or the alt planes (ms_allele_dev.h: the same layout) until its unit is full; zero-length pieces
// (deletions, empty genome pieces between adjacent substitutions) are stepped over, so a unit may take more than 32 pieces.  A block covers
// kPgBlockBases output bases: the variants that touch them are read from a table of block starts (pg_blockstart_kernel: one binary search
// over os per block, all of them independent), up to kPgStage of them are staged in LDS (a personal genome has ~12 per block) and the
// block's threads search there; a denser block searches the same range in global memory.
//
// Lift kernel: a thread per query, a binary search over the chromosome's applied variants (g for ref -> alt, os for alt -> ref).
#include <algorithm>
#include <memory>

#include "ms_allele_dev.h"
#include "ms_device.h"
#include "ms_handles.h"

struct ms_liftmap {
    int device = 0;
    int32_t C = 0;
    int64_t V = 0, n_applied = 0;
    std::vector<uint8_t> status, mismatch;            // [V]
    std::vector<int64_t> ref_off, alt_off;            // [C + 1] chromosome offsets of the two genomes
    void *block = nullptr;                            // one pooled device block holding the arrays below
    size_t block_bytes = 0;
    int64_t *d_g = nullptr, *d_os = nullptr;          // [n_applied] packed position in the reference / in the output
    int32_t *d_r = nullptr, *d_a = nullptr;
    int64_t *d_goff = nullptr, *d_noff = nullptr, *d_cstart = nullptr;   // [C + 1]: offsets of either genome, first applied variant of the chromosome
    double device_ms = 0.0;                           // first launch -> last kernel done
    double stage_ms[4] = {};                          // upload + pack + prep | order + status + layout | (host: the output's block) | splice + hints
};

namespace ms {

namespace {

constexpr int kPgThreads = 256;
constexpr int kPgBlockBases = kPgThreads * 32;  // output bases of one splice block
constexpr int kPgStage = 512;                   // applied variants a splice block stages in LDS (14 KB); more: it searches global memory
constexpr int kLiftThreads = 256;               // queries per block

unsigned pg_grid(int64_t n) { return (unsigned) ((std::max<int64_t>(n, 1) + kPgThreads - 1) / kPgThreads); }

__global__ void __launch_bounds__(kPgThreads) pg_key_kernel(const AlRec *__restrict__ rec, const int32_t *__restrict__ chrom, const uint8_t *__restrict__ mis,
                                                            int skip, uint64_t skip_key, int64_t V, uint64_t *__restrict__ keys, int64_t *__restrict__ vals) {
    const int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    keys[v] = (skip && mis[v]) ? skip_key : (uint64_t) (rec[v].g + chrom[v]);
    vals[v] = v;
}

// the ends in sorted order; 0 for a variant that takes no part
__global__ void __launch_bounds__(kPgThreads) pg_end_kernel(const AlRec *__restrict__ rec, const int32_t *__restrict__ chrom, const uint8_t *__restrict__ mis,
                                                            int skip, const int64_t *__restrict__ svals, int64_t V, uint64_t *__restrict__ ends) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    const int64_t v = svals[i];
    ends[i] = (skip && mis[v]) ? 0ull : (uint64_t) (rec[v].g + rec[v].r + chrom[v]);
}

// status of the variant at sorted place i (1 applied, 0 overlap, 2 REF mismatch) and its compaction flag; flag[V] = 0 closes the sum
__global__ void __launch_bounds__(kPgThreads) pg_status_kernel(const uint64_t *__restrict__ skeys, const int64_t *__restrict__ svals, const uint64_t *__restrict__ run_max,
                                                               const uint8_t *__restrict__ mis, int skip, int64_t V, uint8_t *__restrict__ status,
                                                               uint32_t *__restrict__ flag) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) flag[V] = 0u;
    if (i >= V) return;
    const int64_t v = svals[i];
    uint32_t st = 1u;
    if (skip && mis[v]) st = 2u;
    else if (i > 0 && run_max[i - 1] > skeys[i]) st = 0u;
    status[v] = (uint8_t) st;
    flag[i] = st == 1u ? 1u : 0u;
}

__global__ void __launch_bounds__(kPgThreads) pg_compact_kernel(const AlRec *__restrict__ rec, const int32_t *__restrict__ chrom, const int64_t *__restrict__ svals,
                                                                const uint32_t *__restrict__ flag, const uint64_t *__restrict__ dest, int64_t V,
                                                                int64_t *__restrict__ ap_g, int32_t *__restrict__ ap_r, int32_t *__restrict__ ap_a,
                                                                int64_t *__restrict__ ap_aoff, int32_t *__restrict__ ap_chrom, int64_t *__restrict__ delta) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V || !flag[i]) return;
    const int64_t v = svals[i], j = (int64_t) dest[i];
    const AlRec q = rec[v];
    ap_g[j] = q.g; ap_r[j] = q.r; ap_a[j] = q.a; ap_aoff[j] = q.aoff; ap_chrom[j] = chrom[v];
    delta[j] = (int64_t) q.a - q.r;
}

// os_j = g_j + D_j for the applied variants (their number is dest[V], still on the device)
__global__ void __launch_bounds__(kPgThreads) pg_outstart_kernel(const int64_t *__restrict__ ap_g, const int64_t *__restrict__ D, const uint64_t *__restrict__ n_dev,
                                                                 int64_t *__restrict__ os) {
    const int64_t j = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (j < (int64_t) *n_dev) os[j] = ap_g[j] + D[j];
}

// per chromosome c in [0, C]: cstart[c] = the first applied variant of a chromosome >= c, noff[c] = goff[c] + D[cstart[c]]; hdr = noff, then n
__global__ void __launch_bounds__(kPgThreads) pg_chrom_kernel(const int32_t *__restrict__ ap_chrom, const int64_t *__restrict__ D, const uint64_t *__restrict__ n_dev,
                                                              const int64_t *__restrict__ goff, int32_t C, int64_t *__restrict__ cstart,
                                                              int64_t *__restrict__ noff, int64_t *__restrict__ hdr) {
    const int32_t c = (int32_t) (blockIdx.x * blockDim.x + threadIdx.x);
    if (c > C) return;
    const int64_t n = (int64_t) *n_dev;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ap_chrom[mid] < c) lo = mid + 1; else hi = mid;
    }
    cstart[c] = lo;
    const int64_t o = goff[c] + D[lo];
    noff[c] = o;
    hdr[c] = o;
    if (c == 0) hdr[C + 1] = n;
}

// the first j in [0, n) with a[j] > key (upper = true) or a[j] >= key (upper = false)
template <bool UPPER, typename F>
__device__ __forceinline__ int64_t pg_bound(F at, int64_t n, int64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int64_t x = at(mid);
        if (UPPER ? x <= key : x < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ub[b] = the number of applied variants that start at or in front of output base b * kPgBlockBases (b < nb), and n for b = nb: the
// variants of every splice block, found once by nb + 1 independent searches instead of two dependent ones at the start of every block
__global__ void __launch_bounds__(kPgThreads) pg_blockstart_kernel(const int64_t *__restrict__ os, int64_t n, int64_t nb, int64_t *__restrict__ ub) {
    const int64_t b = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (b > nb) return;
    ub[b] = b == nb ? n : pg_bound<true>([&](int64_t j) { return os[j]; }, n, b * kPgBlockBases);
}

// One thread per 32 output bases (the file's header has the geometry).  os / g / r / a / aoff [n]: the applied variants in order.
__global__ void __launch_bounds__(kPgThreads) splice_kernel(const uint32_t *__restrict__ gcodes, const uint32_t *__restrict__ gnmask,
                                                            const uint32_t *__restrict__ acodes, const uint32_t *__restrict__ amask,
                                                            const int64_t *__restrict__ os, const int64_t *__restrict__ g, const int32_t *__restrict__ r,
                                                            const int32_t *__restrict__ a, const int64_t *__restrict__ aoff, const int64_t *__restrict__ ub, int64_t n_out,
                                                            uint32_t *__restrict__ codes, uint32_t *__restrict__ nmask) {
    __shared__ int64_t s_os[kPgStage], s_gsrc[kPgStage], s_asrc[kPgStage];
    __shared__ int32_t s_a[kPgStage];
    const int64_t p0 = (int64_t) blockIdx.x * kPgBlockBases;
    const int64_t p1 = p0 + kPgBlockBases < n_out ? p0 + kPgBlockBases : n_out;
    // the block's variants: from the last one that starts at or in front of p0 (its alt or the genome behind it holds p0) to the last that starts
    // in front of p1 (one that starts AT p1 comes along: it is never reached)
    const int64_t first = ub[blockIdx.x] - 1;
    const int64_t j0 = first < 0 ? 0 : first;
    const int64_t cnt = ub[blockIdx.x + 1] - j0;
    const bool staged = cnt <= kPgStage;
    if (staged)
        for (int64_t i = threadIdx.x; i < cnt; i += kPgThreads) {
            s_os[i] = os[j0 + i];
            s_gsrc[i] = g[j0 + i] + r[j0 + i];
            s_asrc[i] = aoff[j0 + i];
            s_a[i] = a[j0 + i];
        }
    __syncthreads();
    const int64_t u = (int64_t) blockIdx.x * kPgThreads + threadIdx.x, p = u * 32;
    if (p >= n_out) return;
    auto OS = [&](int64_t k) { return staged ? s_os[k] : os[j0 + k]; };
    auto GSRC = [&](int64_t k) { return staged ? s_gsrc[k] : g[j0 + k] + r[j0 + k]; };
    auto ASRC = [&](int64_t k) { return staged ? s_asrc[k] : aoff[j0 + k]; };
    auto AL = [&](int64_t k) { return (int64_t) (staged ? s_a[k] : a[j0 + k]); };
    int64_t k = pg_bound<true>(OS, cnt, p) - 1;                  // the last variant of the block's range with os <= p; -1: p lies in front of the first variant of all
    const int total = (int) (n_out - p < 32 ? n_out - p : 32);
    uint64_t cw = 0;
    uint32_t nw = 0;
    int filled = 0;
    while (filled < total) {
        const int64_t d = p + filled;
        while (k + 1 < cnt && OS(k + 1) <= d) k++;               // pieces of no bases are stepped over
        int64_t sp, end;
        const uint32_t *cp = gcodes, *np = gnmask;
        if (k < 0) {
            sp = d;
            end = cnt > 0 ? OS(0) : p1;
        } else {
            const int64_t o = OS(k), al = AL(k);
            if (d < o + al) {
                sp = ASRC(k) + (d - o);
                end = o + al;
                cp = acodes;
                np = amask;
            } else {
                sp = GSRC(k) + (d - o - al);
                end = k + 1 < cnt ? OS(k + 1) : p1;
            }
        }
        const int seg = end - d < (int64_t) (total - filled) ? (int) (end - d) : total - filled;
        const uint64_t scw = code_window(cp, sp);
        const uint32_t snw = n_window(np, sp);
        cw |= (scw & low_mask2(seg)) << (2 * filled);
        nw |= (snw & low_mask(seg)) << filled;
        filled += seg;
    }
    codes[2 * u] = (uint32_t) cw;
    codes[2 * u + 1] = (uint32_t) (cw >> 32);
    nmask[u] = nw;
}

// One thread per query (c, position): the header's two maps, in packed coordinates.
__global__ void __launch_bounds__(kLiftThreads) lift_kernel(int to_ref, const int64_t *__restrict__ g, const int64_t *__restrict__ os, const int32_t *__restrict__ r,
                                                            const int32_t *__restrict__ a, const int64_t *__restrict__ goff, const int64_t *__restrict__ noff,
                                                            const int64_t *__restrict__ cstart, const int32_t *__restrict__ qchrom, const int64_t *__restrict__ qpos,
                                                            int64_t nq, int64_t *__restrict__ out, uint8_t *__restrict__ inside) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const int32_t c = qchrom[i];
    const int64_t j0 = cstart[c], j1 = cstart[c + 1];
    const int64_t *__restrict__ from = to_ref ? os : g;
    const int64_t src0 = to_ref ? noff[c] : goff[c], dst0 = to_ref ? goff[c] : noff[c];
    const int64_t key = src0 + qpos[i];
    const int64_t j = j0 + pg_bound<true>([&](int64_t k) { return from[j0 + k]; }, j1 - j0, key) - 1;
    int64_t res = qpos[i];
    uint32_t in = 0u;
    if (j >= j0) {
        const int64_t gj = g[j], oj = os[j], rj = r[j], aj = a[j];
        const int64_t s = to_ref ? oj : gj, slen = to_ref ? aj : rj, t = to_ref ? gj : oj, tlen = to_ref ? rj : aj;
        if (key < s + slen) {
            const int64_t off = key - s;
            res = t + (off < tlen ? off : tlen) - dst0;
            in = 1u;
        } else {
            const int64_t shift = (oj + aj) - (gj + rj);          // what the variants up to j add to a position behind them
            res = (to_ref ? key - shift : key + shift) - dst0;
        }
    }
    out[i] = res;
    if (inside) inside[i] = (uint8_t) in;
}

}  // namespace

}  // namespace ms

using namespace ms;

extern "C" {

void ms_liftmap_free(ms_liftmap *m) {
    if (!m) return;
    if (m->block) {
        (void) hipSetDevice(m->device);
        DeviceCtx *c = nullptr;
        if (get_ctx(m->device, &c) == MS_OK) pool_free(c, m->block, m->block_bytes); else (void) hipFree(m->block);
    }
    delete m;
}

int ms_genome_apply_alleles(const ms_genome *genome, const int32_t *chrom, const int64_t *pos, const int32_t *ref_len, const char *alt_bases,
                            const int64_t *alt_offsets, const char *ref_bases, int64_t n_variants, uint32_t flags, ms_genome **out, ms_liftmap **map) {
    if (map) *map = nullptr;
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    if (!require_device()) return MS_ERR_RUNTIME;
    if (flags & ~MS_APPLY_SKIP_MISMATCH) { set_error("unknown apply flags 0x%x", flags); return MS_ERR_INVALID; }
    if (!genome) { set_error("NULL handle"); return MS_ERR_INVALID; }
    const ms_seqset *G = reinterpret_cast<const ms_seqset *>(genome);
    const int64_t V = n_variants;
    const int32_t C = (int32_t) G->R;
    std::vector<int64_t> ref_off;
    int64_t A = 0, Rn = 0;
    int rc = validate_alleles(G, chrom, pos, ref_len, alt_bases, alt_offsets, ref_bases, V, ref_off, &A, &Rn);
    if (rc) return rc;
    const int skip = ((flags & MS_APPLY_SKIP_MISMATCH) && ref_bases) ? 1 : 0;
    DeviceCtx *c;
    if ((rc = get_ctx(G->device, &c))) return rc;
    std::unique_ptr<ms_liftmap> res(new (std::nothrow) ms_liftmap());
    if (!res) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    std::vector<int64_t> h_hdr;
    try {
        res->status.assign((size_t) V, 1);
        res->mismatch.assign((size_t) V, 0);
        res->ref_off = G->offsets;
        res->alt_off = G->offsets;
        h_hdr.assign((size_t) C + 2, 0);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    res->device = c->device;
    res->C = C;
    res->V = V;
    std::lock_guard<std::mutex> lk_dev(c->mu);
    const hipStream_t st = c->stream;

    const uint64_t skip_key = (uint64_t) G->n_bases + (uint64_t) C + 1u;     // past every key g + c
    int end_bit = 1;
    while (end_bit < 64 && (skip_key >> end_bit)) end_bit++;
    const size_t Vz = (size_t) std::max<int64_t>(V, 1), Cz = (size_t) C + 2;
    size_t t_sort = 0, t_max = 0, t_sum32 = 0, t_sum64 = 0;
    if (V > 0) {
        if ((rc = sort_hit_pairs(nullptr, &t_sort, nullptr, nullptr, nullptr, nullptr, (size_t) V, 0, end_bit, st))) return rc;
        if ((rc = inclusive_max_u64(nullptr, &t_max, nullptr, nullptr, (size_t) V, st))) return rc;
        if ((rc = exclusive_sum_u32(nullptr, &t_sum32, nullptr, nullptr, (size_t) V + 1, st))) return rc;
        if ((rc = exclusive_sum_i64(nullptr, &t_sum64, nullptr, nullptr, (size_t) V + 1, st))) return rc;
    }
    const size_t tmp_bytes = std::max(std::max(t_sort, t_max), std::max(t_sum32, t_sum64));

    // ---- the map's block: the applied variants (at most V) and the chromosome tables
    {
        Carve mv;
        const auto s_g = mv.add<int64_t>(Vz), s_os = mv.add<int64_t>(Vz);
        const auto s_r = mv.add<int32_t>(Vz), s_a = mv.add<int32_t>(Vz);
        const auto s_goff = mv.add<int64_t>(Cz), s_noff = mv.add<int64_t>(Cz), s_cstart = mv.add<int64_t>(Cz);
        if ((rc = pool_alloc(c, mv.bytes(), &res->block, &res->block_bytes))) return rc;
        res->d_g = Carve::at(res->block, s_g);
        res->d_os = Carve::at(res->block, s_os);
        res->d_r = Carve::at(res->block, s_r);
        res->d_a = Carve::at(res->block, s_a);
        res->d_goff = Carve::at(res->block, s_goff);
        res->d_noff = Carve::at(res->block, s_noff);
        res->d_cstart = Carve::at(res->block, s_cstart);
    }
    ms_liftmap *raw = res.release();

    // ---- the call's work block
    Carve cv;
    const AlSlots us = al_upload_slots(cv, V, A, Rn);
    const auto s_status = cv.add<uint8_t>(Vz);
    const auto s_keys = cv.add<uint64_t>(Vz + 1), s_skeys = cv.add<uint64_t>(Vz + 1), s_ends = cv.add<uint64_t>(Vz + 1), s_max = cv.add<uint64_t>(Vz + 1);
    const auto s_vals = cv.add<int64_t>(Vz + 1), s_svals = cv.add<int64_t>(Vz + 1);
    const auto s_dest = cv.add<uint64_t>(Vz + 1);              // [V + 1]: the last entry is the number applied
    const auto s_delta = cv.add<int64_t>(Vz + 1);              // [V + 1], zero behind the applied ones
    const auto s_D = cv.add<int64_t>(Vz + 1);                  // [V + 1]
    const auto s_flag = cv.add<uint32_t>(Vz + 1);              // [V + 1]
    const auto s_apchrom = cv.add<int32_t>(Vz + 1);
    const auto s_hdr = cv.add<int64_t>(Cz);                    // the new offsets [C + 1], then the number applied
    const auto s_ub = cv.add<int64_t>((size_t) ((G->n_bases + A) / kPgBlockBases) + 3);   // [splice blocks + 1]: pg_blockstart_kernel (the output has at most n_bases + A bases)
    const auto s_tmp = cv.add<char>(std::max<size_t>(tmp_bytes, 1));
    void *wblk = nullptr;
    size_t wgot = 0;
    auto fail = [&](int code) { (void) hipStreamSynchronize(st); if (wblk) pool_free(c, wblk, wgot); ms_liftmap_free(raw); return code; };   // (nothing queued may still read the blocks)
    auto hip_fail = [&](hipError_t e, const char *what) { set_error("%s failed: %s", what, hipGetErrorString(e)); return fail(e == hipErrorOutOfMemory ? MS_ERR_NOMEM : MS_ERR_RUNTIME); };
    if ((rc = pool_alloc(c, cv.bytes(), &wblk, &wgot))) return fail(rc);
    const AlDev U = al_upload_at(wblk, us);
    uint8_t *d_status = Carve::at(wblk, s_status);
    uint64_t *d_keys = Carve::at(wblk, s_keys), *d_skeys = Carve::at(wblk, s_skeys), *d_ends = Carve::at(wblk, s_ends), *d_max = Carve::at(wblk, s_max);
    int64_t *d_vals = Carve::at(wblk, s_vals), *d_svals = Carve::at(wblk, s_svals);
    uint64_t *d_dest = Carve::at(wblk, s_dest);
    int64_t *d_delta = Carve::at(wblk, s_delta), *d_D = Carve::at(wblk, s_D);
    uint32_t *d_flag = Carve::at(wblk, s_flag);
    int32_t *d_apchrom = Carve::at(wblk, s_apchrom);
    int64_t *d_hdr = Carve::at(wblk, s_hdr), *d_ub = Carve::at(wblk, s_ub);
    void *d_tmp = Carve::at(wblk, s_tmp);
    int64_t *d_apaoff = U.pos;                                          // (the positions are not read after the prep kernel: AlRec::g has them)

    hipError_t he = hipEventRecord(c->ev[0], st);
    if (he == hipSuccess) he = hipMemcpyAsync(raw->d_goff, G->offsets.data(), 8 * ((size_t) C + 1), hipMemcpyHostToDevice, st);
    if (he != hipSuccess) return hip_fail(he, "offset upload");
    if (V > 0) {
        he = al_upload(G, U, chrom, pos, ref_len, alt_bases, alt_offsets, ref_bases, ref_off, V, A, Rn, raw->mismatch.data(), st);
        if (he == hipSuccess) he = hipMemsetAsync(d_delta, 0, 8 * ((size_t) V + 1), st);
        if (he == hipSuccess) he = hipEventRecord(c->ev[1], st);
        if (he != hipSuccess) return hip_fail(he, "variant upload");
        // ---- order
        const dim3 gv(pg_grid(V)), bt(kPgThreads);
        hipLaunchKernelGGL(pg_key_kernel, gv, bt, 0, st, U.rec, U.chrom, U.mis, skip, skip_key, V, d_keys, d_vals);
        if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "key kernel");
        size_t tb = tmp_bytes;
        if ((rc = sort_hit_pairs(d_tmp, &tb, d_keys, d_skeys, reinterpret_cast<const double *>(d_vals), reinterpret_cast<double *>(d_svals), (size_t) V, 0, end_bit, st)))
            return fail(rc);                                   // (the values are the indices' bit patterns: the sort only moves them)
        // ---- status and layout
        hipLaunchKernelGGL(pg_end_kernel, gv, bt, 0, st, U.rec, U.chrom, U.mis, skip, d_svals, V, d_ends);
        if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "end kernel");
        tb = tmp_bytes;
        if ((rc = inclusive_max_u64(d_tmp, &tb, d_ends, d_max, (size_t) V, st))) return fail(rc);
        hipLaunchKernelGGL(pg_status_kernel, gv, bt, 0, st, d_skeys, d_svals, d_max, U.mis, skip, V, d_status, d_flag);
        if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "status kernel");
        tb = tmp_bytes;
        if ((rc = exclusive_sum_u32(d_tmp, &tb, d_flag, d_dest, (size_t) V + 1, st))) return fail(rc);
        hipLaunchKernelGGL(pg_compact_kernel, gv, bt, 0, st, U.rec, U.chrom, d_svals, d_flag, d_dest, V, raw->d_g, raw->d_r, raw->d_a, d_apaoff, d_apchrom, d_delta);
        if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "compaction");
        tb = tmp_bytes;
        if ((rc = exclusive_sum_i64(d_tmp, &tb, d_delta, d_D, (size_t) V + 1, st))) return fail(rc);
        hipLaunchKernelGGL(pg_outstart_kernel, gv, bt, 0, st, raw->d_g, d_D, d_dest + V, raw->d_os);
        if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "layout");
        hipLaunchKernelGGL(pg_chrom_kernel, dim3(pg_grid((int64_t) C + 1)), bt, 0, st, d_apchrom, d_D, d_dest + V, raw->d_goff, C, raw->d_cstart, raw->d_noff, d_hdr);
        if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "chromosome table");
        he = hipMemcpyAsync(h_hdr.data(), d_hdr, 8 * ((size_t) C + 2), hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipMemcpyAsync(raw->status.data(), d_status, (size_t) V, hipMemcpyDeviceToHost, st);
    } else {
        he = hipEventRecord(c->ev[1], st);
        if (he == hipSuccess) he = hipMemcpyAsync(raw->d_noff, G->offsets.data(), 8 * ((size_t) C + 1), hipMemcpyHostToDevice, st);
        if (he == hipSuccess) he = hipMemsetAsync(raw->d_cstart, 0, 8 * ((size_t) C + 1), st);
        std::copy(G->offsets.begin(), G->offsets.end(), h_hdr.begin());
    }
    if (he == hipSuccess) he = hipEventRecord(c->ev[2], st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) return hip_fail(he, "variant layout");
    const int64_t n = h_hdr[(size_t) C + 1];
    raw->n_applied = n;
    std::copy(h_hdr.begin(), h_hdr.begin() + C + 1, raw->alt_off.begin());

    // ---- the output genome: host tables and the device block from the new offsets, then the splice and the region hints
    ms_seqset *S = nullptr;
    if ((rc = seqset_create_unpacked(raw->alt_off.data(), C, c->device, &S))) return fail(rc);
    auto fail_out = [&](int code) { (void) hipStreamSynchronize(st); ms_seqset_free(S); return fail(code); };
    const int64_t n_units = (S->n_bases + 31) / 32;
    he = hipEventRecord(c->ev[3], st);
    if (he == hipSuccess && n_units > 0) {
        const int64_t nb = (n_units + kPgThreads - 1) / kPgThreads;
        hipLaunchKernelGGL(pg_blockstart_kernel, dim3(pg_grid(nb + 1)), dim3(kPgThreads), 0, st, (const int64_t *) raw->d_os, n, nb, d_ub);
        he = hipGetLastError();
        if (he == hipSuccess) {
            hipLaunchKernelGGL(splice_kernel, dim3((unsigned) nb), dim3(kPgThreads), 0, st, G->d_codes, G->d_nmask, U.acode,
                               U.amask, raw->d_os, raw->d_g, raw->d_r, raw->d_a, d_apaoff, (const int64_t *) d_ub, S->n_bases, S->d_codes, S->d_nmask);
            he = hipGetLastError();
        }
    }
    if (he != hipSuccess) { set_error("splice failed: %s", hipGetErrorString(he)); return fail_out(MS_ERR_RUNTIME); }
    if ((rc = seqset_launch_hints(S, st))) return fail_out(rc);
    he = hipEventRecord(c->ev[4], st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) { set_error("splice failed: %s", hipGetErrorString(he)); return fail_out(MS_ERR_RUNTIME); }
    float t = 0;
    (void) hipEventElapsedTime(&t, c->ev[0], c->ev[4]); raw->device_ms = t;
    (void) hipEventElapsedTime(&t, c->ev[0], c->ev[1]); raw->stage_ms[0] = t;
    (void) hipEventElapsedTime(&t, c->ev[1], c->ev[2]); raw->stage_ms[1] = t;
    (void) hipEventElapsedTime(&t, c->ev[2], c->ev[3]); raw->stage_ms[2] = t;
    (void) hipEventElapsedTime(&t, c->ev[3], c->ev[4]); raw->stage_ms[3] = t;
    pool_free(c, wblk, wgot);
    *out = reinterpret_cast<ms_genome *>(S);
    if (map) *map = raw; else ms_liftmap_free(raw);
    return MS_OK;
}

int ms_liftmap_shape(const ms_liftmap *m, int32_t *n_chroms, int64_t *n_variants, int64_t *n_applied) {
    if (!m) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (n_chroms) *n_chroms = m->C;
    if (n_variants) *n_variants = m->V;
    if (n_applied) *n_applied = m->n_applied;
    return MS_OK;
}

int ms_liftmap_status(const ms_liftmap *m, uint8_t *status) {
    if (!m || (!status && m->V > 0)) { set_error("NULL argument"); return MS_ERR_INVALID; }
    std::copy(m->status.begin(), m->status.end(), status);
    return MS_OK;
}

int ms_liftmap_ref_mismatch(const ms_liftmap *m, uint8_t *out) {
    if (!m || (!out && m->V > 0)) { set_error("NULL argument"); return MS_ERR_INVALID; }
    std::copy(m->mismatch.begin(), m->mismatch.end(), out);
    return MS_OK;
}

int ms_liftmap_chrom_sizes(const ms_liftmap *m, int64_t *ref_len, int64_t *alt_len) {
    if (!m) { set_error("NULL argument"); return MS_ERR_INVALID; }
    for (int32_t c = 0; c < m->C; c++) {
        if (ref_len) ref_len[c] = m->ref_off[(size_t) c + 1] - m->ref_off[(size_t) c];
        if (alt_len) alt_len[c] = m->alt_off[(size_t) c + 1] - m->alt_off[(size_t) c];
    }
    return MS_OK;
}

int ms_liftmap_lift(const ms_liftmap *m, int direction, const int32_t *chrom, const int64_t *pos, int64_t n, int64_t *out_pos, uint8_t *inside) {
    if (!m) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (direction != MS_LIFT_REF_TO_ALT && direction != MS_LIFT_ALT_TO_REF) { set_error("invalid lift direction %d", direction); return MS_ERR_INVALID; }
    if (n < 0 || (n > 0 && (!chrom || !pos || !out_pos))) { set_error("bad query arrays"); return MS_ERR_INVALID; }
    const std::vector<int64_t> &off = direction == MS_LIFT_ALT_TO_REF ? m->alt_off : m->ref_off;
    for (int64_t i = 0; i < n; i++) {
        if (chrom[i] < 0 || chrom[i] >= m->C) { set_error("query %lld: chromosome index %d out of range", (long long) i, chrom[i]); return MS_ERR_INVALID; }
        const int64_t len = off[(size_t) chrom[i] + 1] - off[(size_t) chrom[i]];
        if (pos[i] < 0 || pos[i] > len) {
            set_error("query %lld: position %lld is outside [0, %lld] of chromosome %d", (long long) i, (long long) pos[i], (long long) len, chrom[i]);
            return MS_ERR_INVALID;
        }
    }
    if (n == 0) return MS_OK;
    DeviceCtx *c;
    int rc = get_ctx(m->device, &c);
    if (rc) return rc;
    const size_t nz = (size_t) n;
    Carve cv;
    const auto s_c = cv.add<int32_t>(nz);
    const auto s_p = cv.add<int64_t>(nz), s_o = cv.add<int64_t>(nz);
    const auto s_in = cv.add<uint8_t>(nz);
    void *blk = nullptr;
    size_t got = 0;
    if ((rc = pool_alloc(c, cv.bytes(), &blk, &got))) return rc;
    int32_t *d_c = Carve::at(blk, s_c);
    int64_t *d_p = Carve::at(blk, s_p), *d_o = Carve::at(blk, s_o);
    uint8_t *d_in = Carve::at(blk, s_in);
    std::lock_guard<std::mutex> lk_dev(c->mu);
    const hipStream_t st = c->stream;
    hipError_t he = hipMemcpyAsync(d_c, chrom, 4 * nz, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(d_p, pos, 8 * nz, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) {
        hipLaunchKernelGGL(lift_kernel, dim3((unsigned) ((n + kLiftThreads - 1) / kLiftThreads)), dim3(kLiftThreads), 0, st, direction == MS_LIFT_ALT_TO_REF ? 1 : 0,
                           (const int64_t *) m->d_g, (const int64_t *) m->d_os, (const int32_t *) m->d_r, (const int32_t *) m->d_a, (const int64_t *) m->d_goff,
                           (const int64_t *) m->d_noff, (const int64_t *) m->d_cstart, (const int32_t *) d_c, (const int64_t *) d_p, n, d_o, inside ? d_in : (uint8_t *) nullptr);
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpyAsync(out_pos, d_o, 8 * nz, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess && inside) he = hipMemcpyAsync(inside, d_in, nz, hipMemcpyDeviceToHost, st);
    const hipError_t hs = hipStreamSynchronize(st);
    if (he == hipSuccess) he = hs;
    pool_free(c, blk, got);
    if (he != hipSuccess) { set_error("lift failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    return MS_OK;
}

int ms_liftmap_device_ms(const ms_liftmap *m, double *ms) {
    if (!m || !ms) { set_error("NULL argument"); return MS_ERR_INVALID; }
    *ms = m->device_ms;
    return MS_OK;
}

int ms_debug_liftmap_stage_ms(const ms_liftmap *m, double out[4]) {
    if (!m || !out) { set_error("NULL argument"); return MS_ERR_INVALID; }
    std::copy(m->stage_ms, m->stage_ms + 4, out);
    return MS_OK;
}

int ms_debug_personal_dims(int32_t out[4]) {
    if (!out) { set_error("NULL argument"); return MS_ERR_INVALID; }
    out[0] = kPgBlockBases;
    out[1] = kPgStage;
    out[2] = kLiftThreads;
    out[3] = 0;
    return MS_OK;
}

}  // extern "C"
