// ms_allele_dev.h -- what the kernels over sequence-resolved alleles share (ms_alleles.hip: the records of the windows that pass;
// ms_allelebest.hip: the best window per haplotype; ms_personal.hip: the whole variant set spliced into a new genome): the validation of
// the variant arguments, a variant's prep record, the count of the windows an allele touches, the alt planes and the spliced read of an
// alt-haplotype step, the upload of a call's variants (al_upload) and the column step of the scoring walk (tab_step).  ms_alleles.hip's
// header comment has the geometry.
#pragma once
#include <algorithm>

#include "ms_device.h"
#include "ms_handles.h"

namespace ms {

namespace {

// The variant arguments of ms_scan_alleles, ms_scan_alleles_best and ms_genome_apply_alleles, validated in one place (the header's
// MS_ERR_INVALID cases, in this order); on MS_OK ref_off [V + 1] holds the prefix of ref_len, *A the alt bytes and *Rn the REF bytes
// (0 when ref_bases is NULL).
inline int validate_alleles(const ms_seqset *G, const int32_t *chrom, const int64_t *pos, const int32_t *ref_len, const char *alt_bases,
                            const int64_t *alt_offsets, const char *ref_bases, int64_t V, std::vector<int64_t> &ref_off, int64_t *A, int64_t *Rn) {
    if (V < 0 || (V > 0 && (!chrom || !pos || !ref_len || !alt_offsets))) { set_error("bad variant arrays"); return MS_ERR_INVALID; }
    const int64_t n_chroms = G->R;
    const int64_t *goff = G->offsets.data();
    if (V > 0 && alt_offsets[0] != 0) { set_error("alt_offsets[0] must be 0"); return MS_ERR_INVALID; }
    try { ref_off.assign((size_t) V + 1, 0); } catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    for (int64_t v = 0; v < V; v++) {
        if (chrom[v] < 0 || chrom[v] >= n_chroms) { set_error("variant %lld: chromosome index %d out of range", (long long) v, chrom[v]); return MS_ERR_INVALID; }
        const int64_t len = goff[chrom[v] + 1] - goff[chrom[v]], x = pos[v], r = ref_len[v], a = alt_offsets[v + 1] - alt_offsets[v];
        if (a < 0) { set_error("variant %lld: alt_offsets must not decrease", (long long) v); return MS_ERR_INVALID; }
        if (x < 0 || x > len || r < 0 || x + r > len) {
            set_error("variant %lld: reference bases [%lld, %lld) are outside chromosome %d of length %lld", (long long) v, (long long) x, (long long) (x + r),
                      chrom[v], (long long) len);
            return MS_ERR_INVALID;
        }
        if (r + a == 0) { set_error("variant %lld: both alleles are empty", (long long) v); return MS_ERR_INVALID; }
        if (r > MS_ALLELE_MAX_LEN || a > MS_ALLELE_MAX_LEN) {
            set_error("variant %lld: an allele of %lld bases is longer than MS_ALLELE_MAX_LEN (%d)", (long long) v, (long long) std::max(r, a), MS_ALLELE_MAX_LEN);
            return MS_ERR_INVALID;
        }
        ref_off[(size_t) v + 1] = ref_off[(size_t) v] + r;
    }
    *A = V > 0 ? alt_offsets[V] : 0;
    *Rn = ref_bases ? ref_off[(size_t) V] : 0;
    if (*A > 0 && !alt_bases) { set_error("alt_bases is NULL"); return MS_ERR_INVALID; }
    return MS_OK;
}

constexpr int32_t kAlFar = 1 << 30;
constexpr int kAlPlanePad = 4;                  // zero words behind either alt plane: code_window reads 3 words, n_window 2

struct AlRec {                                   // what an item needs of its variant
    int64_t g;                                   // position of x in the packed genome
    int64_t aoff;                                // first alt base in the alt planes
    int32_t lo;                                  // bases of the chromosome in front of x (clamped to kAlFar)
    int32_t hi;                                  // ... and from x + r on
    int32_t r, a;
};

// windows of a haplotype whose allele has len bases, lo bases in front of it and hi behind (the header of ms_alleles.hip)
__host__ __device__ __forceinline__ uint32_t allele_windows(int32_t lo, int32_t hi, int32_t len, int W) {
    const int64_t n = (int64_t) len + (hi - W + 1 < 0 ? hi - W + 1 : 0) + (lo < W - 1 ? lo : W - 1);
    return n > 0 ? (uint32_t) n : 0u;
}

// convert_seq (cscore.c:81-114) for 32 alt bytes a thread: two code words and a mask word in the genome's layout
__global__ void __launch_bounds__(256) al_pack_kernel(const uint8_t *__restrict__ alt, int64_t A, uint32_t *__restrict__ acodes, uint32_t *__restrict__ amask) {
    const int64_t w = (int64_t) blockIdx.x * blockDim.x + threadIdx.x, b0 = w * 32;
    if (b0 >= A) return;
    uint64_t code = 0;
    uint32_t mask = 0;
    const int n = (int) (A - b0 < 32 ? A - b0 : 32);
    for (int k = 0; k < n; k++) {
        const uint32_t ch = (uint32_t) alt[b0 + k] | 0x20u;                            // fold case (cscore.c:93-108)
        const bool acgt = ch == 0x61u || ch == 0x63u || ch == 0x67u || ch == 0x74u;
        if (acgt) code |= (uint64_t) (((ch >> 1) ^ (ch >> 2)) & 3u) << (2 * k);
        else mask |= 1u << k;
    }
    acodes[2 * w] = (uint32_t) code;
    acodes[2 * w + 1] = (uint32_t) (code >> 32);
    amask[w] = mask;
}

// the variant's place and clip distances, and (ref != nullptr) its REF string against the genome: case-insensitive, a non-ACGT genome
// base matches any letter that is not A, C, G or T
__global__ void __launch_bounds__(256) al_prep_kernel(const uint32_t *__restrict__ codes, const uint32_t *__restrict__ nmask,
                                                      const int64_t *__restrict__ offsets, const int32_t *__restrict__ chrom,
                                                      const int64_t *__restrict__ pos, const int32_t *__restrict__ ref_len,
                                                      const int64_t *__restrict__ alt_off, const uint8_t *__restrict__ ref,
                                                      const int64_t *__restrict__ ref_off, int64_t V, AlRec *__restrict__ rec,
                                                      uint8_t *__restrict__ mismatch) {
    const int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int64_t beg = offsets[chrom[v]], end = offsets[chrom[v] + 1], x = pos[v], g = beg + x;
    const int32_t r = ref_len[v];
    AlRec q;
    q.g = g;
    q.aoff = alt_off[v];
    q.lo = (int32_t) (x < kAlFar ? x : kAlFar);
    q.hi = (int32_t) (end - g - r < kAlFar ? end - g - r : kAlFar);
    q.r = r;
    q.a = (int32_t) (alt_off[v + 1] - alt_off[v]);
    rec[v] = q;
    uint32_t bad = 0u;
    if (ref) {
        const uint8_t *__restrict__ s = ref + ref_off[v];
        for (int32_t i = 0; i < r; i++) {
            const int64_t p = g + i;
            const uint32_t code = (codes[p >> 4] >> (2u * ((uint32_t) p & 15u))) & 3u;
            const uint32_t isn = (nmask[p >> 5] >> ((uint32_t) p & 31u)) & 1u;
            const uint32_t ch = (uint32_t) s[i] | 0x20u;
            const bool acgt = ch == 0x61u || ch == 0x63u || ch == 0x67u || ch == 0x74u;
            const uint32_t want = ((ch >> 1) ^ (ch >> 2)) & 3u;
            bad |= acgt ? (isn || code != want) : !isn;
        }
    }
    mismatch[v] = (uint8_t) bad;
}

// The variant arrays of a call on the device: its arguments as given, the REF prefix of validate_alleles, the alt planes (each with
// kAlPlanePad zero words behind it), the prep records and the REF-mismatch flags.  As slots of the call's work block (al_upload_slots)
// and, once the block is there, as pointers (al_upload_at).
template <template <typename> class H>
struct AlArrays {
    H<int32_t> chrom;
    H<int64_t> pos;
    H<int32_t> rlen;
    H<int64_t> aoff, roff;                       // [V + 1]
    H<uint8_t> alt, ref;
    H<uint32_t> acode, amask;                    // side by side: one memset clears both
    H<AlRec> rec;
    H<uint8_t> mis;
};
template <typename T>
using AlPtr = T *;
using AlSlots = AlArrays<Carve::Slot>;
using AlDev = AlArrays<AlPtr>;

inline size_t al_plane_words(int64_t A) { return (size_t) ((A + 31) / 32); }    // mask words of the alt plane; twice as many code words

inline AlSlots al_upload_slots(Carve &cv, int64_t V, int64_t A, int64_t Rn) {
    const size_t Vz = (size_t) std::max<int64_t>(V, 1), a_words = al_plane_words(A);
    AlSlots s;
    s.chrom = cv.add<int32_t>(Vz);
    s.pos = cv.add<int64_t>(Vz);
    s.rlen = cv.add<int32_t>(Vz);
    s.aoff = cv.add<int64_t>(Vz + 1);
    s.roff = cv.add<int64_t>(Vz + 1);
    s.alt = cv.add<uint8_t>((size_t) std::max<int64_t>(A, 1));
    s.ref = cv.add<uint8_t>((size_t) std::max<int64_t>(Rn, 1));
    s.acode = cv.add<uint32_t>(2 * a_words + kAlPlanePad);
    s.amask = cv.add<uint32_t>(a_words + kAlPlanePad);
    s.rec = cv.add<AlRec>(Vz);
    s.mis = cv.add<uint8_t>(Vz);
    return s;
}

inline AlDev al_upload_at(void *base, const AlSlots &s) {
    return AlDev{Carve::at(base, s.chrom), Carve::at(base, s.pos),   Carve::at(base, s.rlen),  Carve::at(base, s.aoff),
                 Carve::at(base, s.roff),  Carve::at(base, s.alt),   Carve::at(base, s.ref),   Carve::at(base, s.acode),
                 Carve::at(base, s.amask), Carve::at(base, s.rec),   Carve::at(base, s.mis)};
}

// The V > 0 variants of a call onto the device, on `st`: the copies, the alt planes packed, the prep records, and the REF-mismatch flags
// back into mismatch[V] (valid once the stream has been waited for).  ref_off, A and Rn are validate_alleles's.
inline hipError_t al_upload(const ms_seqset *G, const AlDev &d, const int32_t *chrom, const int64_t *pos, const int32_t *ref_len, const char *alt_bases,
                            const int64_t *alt_offsets, const char *ref_bases, const std::vector<int64_t> &ref_off, int64_t V, int64_t A, int64_t Rn,
                            uint8_t *mismatch, hipStream_t st) {
    const size_t Vs = (size_t) V, a_words = al_plane_words(A);
    hipError_t he = hipMemcpyAsync(d.chrom, chrom, 4 * Vs, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(d.pos, pos, 8 * Vs, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(d.rlen, ref_len, 4 * Vs, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(d.aoff, alt_offsets, 8 * (Vs + 1), hipMemcpyHostToDevice, st);
    if (he == hipSuccess && ref_bases) he = hipMemcpyAsync(d.roff, ref_off.data(), 8 * (Vs + 1), hipMemcpyHostToDevice, st);
    if (he == hipSuccess && A > 0) he = hipMemcpyAsync(d.alt, alt_bases, (size_t) A, hipMemcpyHostToDevice, st);
    if (he == hipSuccess && Rn > 0) he = hipMemcpyAsync(d.ref, ref_bases, (size_t) Rn, hipMemcpyHostToDevice, st);
    if (he == hipSuccess)                                      // (the two planes lie side by side: one memset, their padding too)
        he = hipMemsetAsync(d.acode, 0, (size_t) ((char *) d.amask - (char *) d.acode) + 4 * (a_words + kAlPlanePad), st);
    if (he == hipSuccess && A > 0) {
        hipLaunchKernelGGL(al_pack_kernel, dim3((unsigned) ((a_words + 255) / 256)), dim3(256), 0, st, d.alt, A, d.acode, d.amask);
        he = hipGetLastError();
    }
    if (he == hipSuccess) {
        hipLaunchKernelGGL(al_prep_kernel, dim3((unsigned) ((V + 255) / 256)), dim3(256), 0, st, G->d_codes, G->d_nmask, G->d_offsets, d.chrom, d.pos, d.rlen,
                           d.aoff, ref_bases ? d.ref : (const uint8_t *) nullptr, d.roff, V, d.rec, d.mis);
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpyAsync(mismatch, d.mis, Vs, hipMemcpyDeviceToHost, st);
    return he;
}

__device__ __forceinline__ uint64_t low_mask2(int n) { return n >= 32 ? ~0ULL : ((1ULL << (2 * n)) - 1ULL); }

// columns [0, n) of the 32-column step that starts d bases behind x on the alt haplotype of q (d < 0: in front of x): the code word and
// the non-ACGT mask, whatever lies past column n undefined.  Every read stays inside its array: a genome read starts inside the
// chromosome (the window does), an alt-plane read at one of the allele's own bases.
__device__ __forceinline__ void alt_step(const uint32_t *__restrict__ codes, const uint32_t *__restrict__ nmask, const uint32_t *__restrict__ acodes,
                                         const uint32_t *__restrict__ amask, const AlRec &q, int d, int n, uint64_t &cw, uint32_t &nw) {
    if (d + n <= 0) {                                          // wholly left of the allele
        cw = code_window(codes, q.g + d);
        nw = n_window(nmask, q.g + d);
        return;
    }
    if (d >= q.a) {                                            // wholly right of it
        const int64_t g = q.g + q.r + (d - q.a);
        cw = code_window(codes, g);
        nw = n_window(nmask, g);
        return;
    }
    const int nl = d < 0 ? -d : 0;                             // columns of the genome left of x: < n <= 32
    const int ja = d < 0 ? 0 : d;                              // first alt base of the step
    const int na = (q.a - ja) < (32 - nl) ? (q.a - ja) : (32 - nl);
    const int nr0 = nl + na;                                   // first column of the genome from x + r on
    cw = 0;
    nw = 0;
    if (nl > 0) {
        cw = code_window(codes, q.g + d) & low_mask2(nl);
        nw = n_window(nmask, q.g + d) & low_mask(nl);
    }
    if (na > 0) {
        cw |= (code_window(acodes, q.aoff + ja) & low_mask2(na)) << (2 * nl);
        nw |= (n_window(amask, q.aoff + ja) & low_mask(na)) << nl;
    }
    if (nr0 < n) {                                             // (then the allele ends in this step: column nr0 is base x + r)
        cw |= code_window(codes, q.g + q.r) << (2 * nr0);
        nw |= n_window(nmask, q.g + q.r) << nr0;
    }
}

// ---- the scoring walk's table: a motif's tab2 entries in LDS behind an all-zero entry, or read from HBM

// lds[0 .. W * 4) = the motif's entries, lds[W * 4] = the zero entry for the columns that add nothing (the caller has the barrier)
template <int THREADS>
__device__ __forceinline__ void tab_stage(double2 *lds, const double2 *__restrict__ tab_g, int W) {
    for (int i = threadIdx.x; i < W * 4; i += THREADS) lds[i] = tab_g[i];
    if (threadIdx.x == 0) lds[W * 4] = make_double2(0.0, 0.0);
}

// N columns from c1 on of the 32-column step at column c0, added in column order; the reads are issued together.  TWO: a second pair of
// sums takes entry tk in place of the table's at column kk (the alt allele of a substitution).
template <bool LDS_TAB, bool TWO, int N>
__device__ __forceinline__ void tab_cols(const double2 *lds, const double2 *__restrict__ tab_g, uint32_t zero, int c0, int n, int c1, uint64_t cw,
                                         uint32_t skip, int kk, double2 tk, double &rf, double &rr, double &af, double &ar) {
    double2 t[N];
#pragma unroll
    for (int u = 0; u < N; u++) {
        const int c = c1 + u;
        const bool nothing = (skip >> c) & 1u;                          // adds +0.0: a sum that started at +0.0 is never -0.0
        if constexpr (LDS_TAB) {
            t[u] = lds[nothing ? zero : (uint32_t) (c0 + c) * 4u + ((uint32_t) (cw >> (2 * c)) & 3u)];
        } else {
            const int cc = c < n ? c : n - 1;                           // clamped: always an entry of the motif
            t[u] = tab_g[(uint32_t) (c0 + cc) * 4u + ((uint32_t) (cw >> (2 * cc)) & 3u)];
            if (nothing) t[u] = make_double2(0.0, 0.0);
        }
    }
#pragma unroll
    for (int u = 0; u < N; u++) {
        rf += t[u].x;
        rr += t[u].y;
        if constexpr (TWO) {
            const double2 ta = (c1 + u == kk) ? tk : t[u];
            af += ta.x;
            ar += ta.y;
        }
    }
}

// the n <= 32 columns of the step at c0: eight columns a time while more than four are left, then four
template <bool LDS_TAB, bool TWO>
__device__ __forceinline__ void tab_step(const double2 *lds, const double2 *__restrict__ tab_g, uint32_t zero, int c0, int n, uint64_t cw, uint32_t nw,
                                         int kk, double2 tk, double &rf, double &rr, double &af, double &ar) {
    const uint32_t skip = nw | ~low_mask(n);                            // bit c: column c0 + c adds nothing
    int c1 = 0;
    for (; n - c1 > 4; c1 += 8) tab_cols<LDS_TAB, TWO, 8>(lds, tab_g, zero, c0, n, c1, cw, skip, kk, tk, rf, rr, af, ar);
    if (n - c1 > 0) tab_cols<LDS_TAB, TWO, 4>(lds, tab_g, zero, c0, n, c1, cw, skip, kk, tk, rf, rr, af, ar);
}

// ---- the record kernels' placement (var_scan_kernel, al_scan_kernel): a block of THREADS walks its items in rounds, item order is
// output order, an item gives a '+' record, a '-' record, both or none

// One round: hit_f / hit_r say which records this thread's item gives.  Returns the records of the round in front of this thread's
// (`before`: a ballot prefix inside the wave, the earlier waves' totals through s_wtot) and of the whole round (`all`).  Has a barrier.
// (two buffers: a wave may write round r + 1's total while another still reads round r's)
template <int THREADS>
__device__ __forceinline__ void place_round(uint32_t (&s_wtot)[2][THREADS / 64], int round, bool hit_f, bool hit_r, uint32_t &before, uint32_t &all) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long bf = __ballot(hit_f), br = __ballot(hit_r), lt = (1ULL << lane) - 1ULL;
    const int buf = round & 1;
    if (lane == 0u) s_wtot[buf][wave] = (uint32_t) (__popcll(bf) + __popcll(br));
    __syncthreads();
    before = (uint32_t) (__popcll(bf & lt) + __popcll(br & lt));
    all = 0u;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t) (THREADS / 64); w++) {
        const uint32_t x = s_wtot[buf][w];
        all += x;
        if (w < wave) before += x;
    }
}

// The count pass's last step: is_lost / is_gained say it of this thread's variant of the tile (false for a thread without one).
// (integer sums: the same in any order)
__device__ __forceinline__ void tally_motif(bool is_lost, bool is_gained, unsigned long long *__restrict__ lost, unsigned long long *__restrict__ gained) {
    const unsigned long long bl = __ballot(is_lost), bg = __ballot(is_gained);
    if ((threadIdx.x & 63u) == 0u) {
        if (bl) atomicAdd(lost, (unsigned long long) __popcll(bl));
        if (bg) atomicAdd(gained, (unsigned long long) __popcll(bg));
    }
}

}  // namespace

}  // namespace ms
