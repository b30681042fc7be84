// ms_fp64.hip -- the fp64 stage of a scan: scoring in the reference's order of operations and the reference's hit test
// (cscore.c:356-358, 373-375), and the hit list it appends to.
//
//   tab2    per motif W*4 double2: tab2[c*4+b] = { M[b][c], M[3-b][W-1-c] }  (forward entry and
//           the reverse-strand entry the reference adds at the same column step, cscore.c:348-352)
//
//   exact_tiled_kernel / exact_all_kernel  every window of the motifs the pre-filter cannot take (the motif's table in LDS / in HBM)
//   rescore_kernel         the pre-filter's candidates (ms_kernels.hip); short candidate lists
//   rescore_carry_kernel   the same for long lists: chunks of the list in motif order, the windows read in list order and
//                          carried through an in-LDS counting sort (few cache lines per read either way)
//
// The hit list comes in two forms.  The plain one (HitOut): one counter word, a block appends its staged hits behind whatever the list holds.
// The BUCKETED one (BucketHitOut; rescore_carry_kernel's second instantiation, for the predicted-size scans bucket_gate passes, ms_scan_geom.h):
// 256 buckets of the lowest digit d0 = (key >> L) & 255 the radix passes would sort, each with its own fill word and its own stretch of the
// list.  A flush counts its staged hits per bucket in LDS, reserves room with one atomicAdd per non-empty bucket, and writes each hit to its
// bucket: a chunk of the candidate list covers ~26 position spots, so ~26 buckets get ~60 hits apiece -- coarser than a radix pass's own
// scatter.  The stable LSD sort's pass over d0 is then the identity and is not run (scan_back, ms_scan.hip).  A hit that finds its bucket
// full is dropped and the overflow word set; nobody waits for anybody.
#include "ms_device.h"

namespace ms {

// The middle field of a hit key: (region << pbits) | position inside the region when the set's regions are short
// enough for that to fit (H.pbits > 0: finalize then only unpacks bits), else the global base position.
__device__ __forceinline__ int64_t hit_coord(const HitOut &H, const DevSeq &S, int64_t r, int64_t g) {
    return H.pbits ? (int64_t) (((uint64_t) r << H.pbits) | (uint64_t) (g - S.offsets[r])) : g;
}

__device__ __forceinline__ void emit_hit(const HitOut &H, uint32_t motif, int64_t g, uint32_t sbit, double score) {
    const unsigned long long i = atomicAdd(H.n_hits, 1ULL);
    if (i < H.cap) {
        H.keys[i] = ((uint64_t) motif << (H.gbits + 1)) | ((uint64_t) g << 1) | sbit;
        H.vals[i] = score;
    }
}

// the reference's normalisation and threshold test, verbatim (cscore.c:356-358 / 373-375)
__device__ __forceinline__ void test_and_emit(const HitOut &H, const DevPwm &Pw, uint32_t motif, int64_t g,
                                              double fwd, double rev, int strand_mask) {
    // raw_floor: (cutoff - 1e-10) * max_raw minus 2000x the worst fp64 rounding of the sum, the divide and
    // the subtract (ms_pwmset.hip, pwmset_upload): below it the reference's test is false whatever the roundings do, so the
    // two IEEE divides are only paid by windows that can actually be hits
    const double floor_ = Pw.raw_floor[motif];
    const bool try_f = (strand_mask & 1) && !(fwd < floor_);
    const bool try_r = (strand_mask & 2) && !(rev < floor_);
    if (!try_f && !try_r) return;
    const double max_raw = Pw.max_raw[motif];
    const double cutoff = Pw.cutoff[motif];
    const double s_f = try_f ? fwd / max_raw : 0.0, s_r = try_r ? rev / max_raw : 0.0;
    const bool hit_f = try_f && s_f - cutoff >= -1e-10, hit_r = try_r && s_r - cutoff >= -1e-10;
    if (hit_f) emit_hit(H, motif, g, 0u, s_f);
    if (hit_r) emit_hit(H, motif, g, 1u, s_r);
}

// Block-level staging of hits in LDS: one global atomicAdd per ~2000 hits instead of one per wave
// (all hit writers of the chip share ONE counter word; it sustains only ~90 M atomics/s).
constexpr int kHitStage = 2048;
template <int N>
struct HitStageN {
    static constexpr int kCap = N;
    uint64_t keys[N];
    double vals[N];
    unsigned int n;
    unsigned long long base;
};
typedef HitStageN<kHitStage> HitStage;

// ... into its bucket: a stage that is full sends its hits here one by one
// (*key_out: the hit's key; returns whether the bucket holds it, which is what fill_tail_buckets_kernel counts as a hit of the list)
__device__ __forceinline__ bool emit_hit(const BucketHitOut &H, uint32_t motif, int64_t g, uint32_t sbit, double score, uint64_t *key_out) {
    const uint64_t key = ((uint64_t) motif << (H.gbits + 1)) | ((uint64_t) g << 1) | sbit;
    const uint32_t b = (uint32_t) (key >> H.B.shift) & 255u;
    const unsigned long long i = atomicAdd(&H.B.fill[b], 1ULL);
    const unsigned long long at = H.B.base[b] + i;
    if (i < H.B.cap[b] && at < H.cap) { H.keys[at] = key; H.vals[at] = score; }
    else *H.B.overflow = 1ULL;
    *key_out = key;
    return i < H.B.cap[b];
}

// a full stage's hit, straight to HBM (the bucketed stage also counts it: emit_direct(RwStageBk &, ...) below)
template <class ST>
__device__ __forceinline__ void emit_direct(ST &, const HitOut &H, uint32_t motif, int64_t g, uint32_t sbit, double score) {
    emit_hit(H, motif, g, sbit, score);
}

template <class ST, class HO>
__device__ __forceinline__ void stage_hit(ST &st, const HO &H, uint32_t motif, int64_t g, uint32_t sbit, double score) {
    const unsigned int i = atomicAdd(&st.n, 1u);
    if (i < (unsigned int) ST::kCap) {
        st.keys[i] = ((uint64_t) motif << (H.gbits + 1)) | ((uint64_t) g << 1) | sbit;
        st.vals[i] = score;
    } else {
        emit_direct(st, H, motif, g, sbit, score);     // stage full: straight to HBM
    }
}

// all threads of the block, at a block-uniform point
template <class ST>
__device__ __forceinline__ void stage_flush(ST &st, const HitOut &H) {
    __syncthreads();
    const unsigned int n = st.n < (unsigned int) ST::kCap ? st.n : (unsigned int) ST::kCap;
    if (threadIdx.x == 0 && n > 0) st.base = atomicAdd(H.n_hits, (unsigned long long) n);
    __syncthreads();
    const unsigned long long base = st.base;
    for (unsigned int i = threadIdx.x; i < n; i += blockDim.x)
        if (base + i < H.cap) { H.keys[base + i] = st.keys[i]; H.vals[base + i] = st.vals[i]; }
    __syncthreads();
    if (threadIdx.x == 0) st.n = 0;
    __syncthreads();
}

// floor32: FieldMeta::floor32, the raw-sum floor of test_and_emit rounded DOWN to a float (it came with the field's record: windows
// that cannot be hits read nothing more); the rest of the test reads {max_raw, cutoff} side by side
template <class ST, class HO>
__device__ __forceinline__ void test_and_stage(ST &st, const HO &H, const DevPwm &Pw, uint32_t motif, int64_t g,
                                               double fwd, double rev, int strand_mask, float floor32) {
    const double floor_ = (double) floor32;
    const bool try_f = (strand_mask & 1) && !(fwd < floor_);
    const bool try_r = (strand_mask & 2) && !(rev < floor_);
    if (!try_f && !try_r) return;
    const double2 mc = *reinterpret_cast<const double2 *>(Pw.thresh + 4 * (size_t) motif);      // {max_raw, cutoff}: one read
    const double max_raw = mc.x, cutoff = mc.y;
    if (try_f) {
        const double s = fwd / max_raw;
        if (s - cutoff >= -1e-10) stage_hit(st, H, motif, g, 0u, s);
    }
    if (try_r) {
        const double s = rev / max_raw;
        if (s - cutoff >= -1e-10) stage_hit(st, H, motif, g, 1u, s);
    }
}

// grid = (ceil(n_bases/256), n_exact motifs).  Fallback for motifs the pre-filter cannot take
// (W > 63, max_raw <= 0, non-finite values, a cutoff so low that (almost) every window passes).
__global__ void __launch_bounds__(256) exact_all_kernel(const DevSeq S, const DevPwm Pw, const int32_t *__restrict__ motifs,
                                                        int strand_mask, const HitOut H) {
    const int64_t g = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= S.n_bases) return;
    const int32_t p = motifs[blockIdx.y];
    const int W = Pw.width[p];
    const int64_t r = find_region(S, g);
    if (g + W > S.offsets[r + 1]) return;
    double fwd, rev;
    score_window(S, Pw.tab2 + Pw.tab_off[p], W, g, fwd, rev);
    test_and_emit(H, Pw, (uint32_t) p, hit_coord(H, S, r, g), fwd, rev, strand_mask);
}

// The same with the motif's table in LDS (round 6): exact_all_kernel reads a table entry per (window, column) through the
// texture addressers -- the unit the fp64 stage is bound by (profiles/r03t_rescore_ta.log) -- although a wave's 64 lanes want at most four
// different entries of a column.  Here a block stages its motif's W x 4 entries (+ an all-zero entry for the columns that add nothing) once,
// scans kExactIter strips of 256 window starts against them, and a column is one 16-byte LDS read (a broadcast: <= 5 distinct addresses per
// wave) + the two fp64 adds, in the reference's column order; a column that adds nothing ADDS the zero entry (score_window32's argument: a
// running sum that started at +0.0 is never -0.0, so x + (+0.0) = x bit for bit).  Motifs wider than kExactTileMaxW keep exact_all_kernel.
constexpr int kExactTileMaxW = 1024;       // 64 KB of LDS for the table
constexpr int kExactIter = 8;

__global__ void __launch_bounds__(256) exact_tiled_kernel(const DevSeq S, const DevPwm Pw, const int32_t *__restrict__ motifs, int strand_mask, const HitOut H) {
    extern __shared__ double2 tab_lds[];                       // [W * 4 + 1]
    const int32_t p = motifs[blockIdx.y];
    const int W = Pw.width[p];
    {
        const double2 *__restrict__ tab = Pw.tab2 + Pw.tab_off[p];
        for (int i = threadIdx.x; i < W * 4; i += 256) tab_lds[i] = tab[i];
        if (threadIdx.x == 0) tab_lds[W * 4] = make_double2(0.0, 0.0);
    }
    __syncthreads();
    const uint32_t zero = (uint32_t) W * 4u;
    for (int it = 0; it < kExactIter; it++) {
        const int64_t g = ((int64_t) blockIdx.x * kExactIter + it) * 256 + threadIdx.x;
        if (g >= S.n_bases) break;
        const int64_t r = find_region(S, g);
        if (g + W > S.offsets[r + 1]) continue;
        double fwd = 0.0, rev = 0.0;
        for (int c0 = 0; c0 < W; c0 += 32) {
            const uint64_t cw = code_window(S.codes, g + c0);
            const int n = (W - c0) < 32 ? (W - c0) : 32;
            const uint32_t skip = n_window(S.nmask, g + c0) | ~low_mask(n);           // bit c: column c0 + c adds nothing
            for (int c1 = 0; c1 < n; c1 += 8) {
                double2 t[8];
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int c = c1 + k;
                    const uint32_t idx = (uint32_t) (c0 + c) * 4u + ((uint32_t) (cw >> (2 * c)) & 3u);
                    t[k] = tab_lds[((skip >> c) & 1u) ? zero : idx];
                }
#pragma unroll
                for (int k = 0; k < 8; k++) { fwd += t[k].x; rev += t[k].y; }
            }
        }
        test_and_emit(H, Pw, (uint32_t) p, hit_coord(H, S, r, g), fwd, rev, strand_mask);
    }
}

// U candidate records per thread and round, their loads issued side by side: the kernel is a chain of dependent gathers
// (record -> region hint / sequence words / motif id -> offsets / width / table offset -> table entries), so the records in
// flight per thread -- not the arithmetic -- set its speed; one barrier pair per round of U records instead of per record.
constexpr int kRescoreU = 4;

__global__ void __launch_bounds__(256) rescore_kernel(const DevSeq S, const DevPwm Pw, const uint64_t *__restrict__ cand,
                                                      const unsigned long long *__restrict__ n_cand, uint64_t n_static, uint64_t cand_cap,
                                                      const FieldMeta *__restrict__ field_meta, int strand_mask,
                                                      const HitOut H) {
    __shared__ HitStage st;
    if (threadIdx.x == 0) st.n = 0;
    __syncthreads();
    unsigned long long n = n_static + *n_cand;            // the waves' own first blocks, then the blocks they reserved from the counter
    if (n > cand_cap) n = cand_cap;
    constexpr int U = kRescoreU;
    const bool both = strand_mask == 3;                  // both strands: fields 2k, 2k + 1 = motif slot k forward, reverse; one strand: field n = slot n
    const unsigned long long per_sub = (unsigned long long) gridDim.x * blockDim.x;
    const unsigned long long per_round = per_sub * U;
    const unsigned long long rounds = (n + per_round - 1) / per_round;
    const int4 *__restrict__ meta4 = reinterpret_cast<const int4 *>(field_meta);
    for (unsigned long long rd = 0; rd < rounds; rd++) {
        const unsigned long long i0 = rd * per_round + (unsigned long long) blockIdx.x * blockDim.x + threadIdx.x;
        uint64_t c[U];
        bool live[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            live[u] = i0 + u * per_sub < n;
            c[u] = live[u] ? cand[i0 + u * per_sub] : 0;
        }
        // independent of each other: the region's place (one read), sequence words, N words, the first flagged field's motif / width / table (one read)
        int64_t g[U];
        int4 bi[U];
        uint64_t cw[U];
        uint32_t nw[U], flags[U];
        int32_t group[U];
        int4 fm[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            g[u] = (int64_t) (c[u] >> 30);
            group[u] = (int32_t) ((c[u] >> 16) & 0x3FFFu);
            const uint32_t f = (uint32_t) c[u] & 0xFFFFu;              // bit n = field n
            flags[u] = both ? (f | (f >> 1)) & 0x5555u : f;             // a motif's two strands are re-scored together anyway
            bi[u] = S.blkinfo[g[u] >> 6];
            cw[u] = code_window(S.codes, g[u]);
            nw[u] = n_window(S.nmask, g[u]);
            fm[u] = flags[u] ? meta4[group[u] * kGroupFields + (__ffs((int) flags[u]) - 1)] : make_int4(-1, 0, 0, 0);
        }
        // the region's bounds: out of the block's record; only tiny regions (a third region start within the block's reach) and
        // starts beyond 32 bits need the offsets themselves
        int64_t r[U], beg[U], end[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t base = g[u] & ~(int64_t) 63;
            int64_t lo = bi[u].x, o0 = base + bi[u].y, o1 = base + bi[u].z, o2 = base + bi[u].w;
            if (bi[u].x < 0) {
                lo = S.blk2reg[g[u] >> 6];
                o0 = S.offsets[lo]; o1 = S.offsets[lo + 1];
                o2 = lo + 2 <= S.R ? S.offsets[lo + 2] : o1;
            }
            if (g[u] < o1) { r[u] = lo; beg[u] = o0; end[u] = o1; }
            else if (g[u] < o2) { r[u] = lo + 1; beg[u] = o1; end[u] = o2; }
            else { r[u] = find_region(S, g[u]); beg[u] = S.offsets[r[u]]; end[u] = S.offsets[r[u] + 1]; }      // tiny regions
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (!live[u]) continue;
            const int64_t gk = H.pbits ? (int64_t) (((uint64_t) r[u] << H.pbits) | (uint64_t) (g[u] - beg[u])) : g[u];
            bool first = true;
            while (flags[u]) {
                const int field = __ffs((int) flags[u]) - 1;
                flags[u] &= flags[u] - 1u;
                int4 f4 = fm[u];
                if (!first) f4 = meta4[group[u] * kGroupFields + field];           // further motifs of the group: rare
                first = false;
                const int32_t m = f4.x;
                const int w = f4.y;
                if (m < 0) continue;
                if (g[u] + w > end[u]) continue;                         // window runs past its region (cscore.c:340)
                double fwd, rev;
                if (w <= 32 && Pw.tab32) score_window32(Pw.tab2, (uint32_t) f4.z, Pw.zero_bytes, w, cw[u], nw[u], fwd, rev);     // non-ACGT bases add nothing (cscore.c:345-353)
                else score_window(S, Pw.tab2 + Pw.tab_off[m], w, g[u], fwd, rev);
                test_and_stage(st, H, Pw, (uint32_t) m, gk, fwd, rev, strand_mask, __int_as_float(f4.w));
            }
        }
        __syncthreads();
        const bool full = st.n > (unsigned int) (kHitStage - 256 * 2 * U);
        __syncthreads();                     // every thread has read st.n before any wave can append again: the decision is block-uniform
        if (full) stage_flush(st, H);
    }
    stage_flush(st, H);
}

int launch_exact_all(const DevSeq &S, const DevPwm &Pw, const int32_t *motifs, int32_t n_motifs, int strand_mask,
                     const HitOut &H, hipStream_t st, int max_width) {
    if (S.n_bases == 0 || n_motifs == 0) return MS_OK;
    const bool tiled = max_width >= 1 && max_width <= kExactTileMaxW && !measure_env("MS_EXACT_UNTILED");      // (A/B and test aid: the round-1 kernel)
    const size_t lds = tiled ? ((size_t) max_width * 4 + 1) * sizeof(double2) : 0;
    if (tiled && lds > 48 * 1024)                                    // (motifs of more than 767 columns: rare enough to ask the driver every time, on whatever device is current)
        MS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(exact_tiled_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
    for (int32_t m0 = 0; m0 < n_motifs; m0 += 32768) {               // grid.y limit
        const int32_t n = n_motifs - m0 < 32768 ? n_motifs - m0 : 32768;
        if (tiled) {
            dim3 grid((unsigned) ((S.n_bases + 256 * kExactIter - 1) / (256 * kExactIter)), (unsigned) n);
            hipLaunchKernelGGL(exact_tiled_kernel, grid, dim3(256), lds, st, S, Pw, motifs + m0, strand_mask, H);
        } else {
            dim3 grid((unsigned) ((S.n_bases + 255) / 256), (unsigned) n);
            hipLaunchKernelGGL(exact_all_kernel, grid, dim3(256), 0, st, S, Pw, motifs + m0, strand_mask, H);
        }
        MS_HIP(hipGetLastError());
    }
    return MS_OK;
}

int launch_rescore(const DevSeq &S, const DevPwm &Pw, const uint64_t *cand, const unsigned long long *n_cand, uint64_t n_static,
                   uint64_t cand_cap, const FieldMeta *field_meta, int strand_mask, const HitOut &H, int n_blocks,
                   hipStream_t st) {
    hipLaunchKernelGGL(rescore_kernel, dim3((unsigned) n_blocks), dim3(256), 0, st, S, Pw, cand, n_cand, n_static, cand_cap,
                       field_meta, strand_mask, H);
    MS_HIP(hipGetLastError());
    return MS_OK;
}

// ---- the fp64 stage for LONG candidate lists: chunks of the list in motif order, the window carried through the sort.
// A scattered read costs the texture addressers ~1.9 cycles per distinct 64-byte line its 64 lanes touch, whatever its width
// (tools/ubench/gather_rate.hip: 122 cycles for 64 lines, 22 for 8), and ~16 of the ~21 reads per candidate are table entries -- one
// line per (motif, column).  In list order a wave's lanes hold ~16 different motifs; in motif order far fewer -- but then the three
// position-bound reads (block record, code words, mask words), whose lanes sit in one or two pre-filter units in list order, would
// touch 64 lines each.  So a block takes 4096 candidates, reads the position-bound data in LIST order, packs what the scoring needs
// into 24 bytes per candidate -- the window's 32 codes, its mask bits, (group, flags), the hit coordinate and how much room the region
// leaves -- brings THAT into (table group, first flagged field) order with a counting sort in LDS on a hash of the record (no memory
// read), and the scoring pass reads only per-motif data.  profiles/r03z_rescore_sorted.log: 2.01 ms per 500 Mbase against 2.73 in list
// order (rescore_kernel, which short lists keep: a chunk per block leaves most of the device idle below ~2e6 candidates).
constexpr int kRwThreads = 1024;
constexpr int kRwPerThread = 4;
constexpr int kRwChunk = kRwThreads * kRwPerThread;       // 4096 candidates: 96 KB of LDS
constexpr int kRwBins = 4096;
typedef HitStageN<2048> RwStage;
struct RwStageBk : RwStage {                // the bucketed flush's words per bucket: staged hits, room left in the bucket, first slot of this flush's hits
    unsigned int cnt[kOrderBuckets], room[kOrderBuckets];
    unsigned long long lo[kOrderBuckets];
    unsigned int hist[kBucketHistPlaces * 256];      // the block's hits by the digits of the radix passes that are left (BucketOut::hist), all chunks together
};

// one hit the buckets hold, into the block's digit counts: the places [shift + 8 + 8 p, + 8), p < hist_places (a hit key has no bit at or
// above the scan's end bit, so a last place of fewer than eight bits needs no mask of its own)
__device__ __forceinline__ void count_places(RwStageBk &st, const BucketOut &B, uint64_t key) {
    for (int p = 0; p < B.hist_places; p++) atomicAdd(&st.hist[p * 256 + ((uint32_t) (key >> (B.shift + 8 + 8 * p)) & 255u)], 1u);
}
// (one LDS add per hit and place.  One add per wave and distinct digit, by ballots, was measured and is far slower -- the fp64 stage
// 3.30 ms against 2.18: the stage holds its hits in the order its sixteen waves appended them, so a wave's 64 keys share few digits.)

__device__ __forceinline__ void emit_direct(RwStageBk &st, const BucketHitOut &H, uint32_t motif, int64_t g, uint32_t sbit, double score) {
    uint64_t key;
    if (emit_hit(H, motif, g, sbit, score, &key)) count_places(st, H.B, key);
}

// start and end of a block of rescore_carry_kernel: the plain stage keeps no counts
__device__ __forceinline__ void stage_hist_clear(RwStage &) {}
__device__ __forceinline__ void stage_hist_clear(RwStageBk &st) {
    for (unsigned int i = threadIdx.x; i < (unsigned int) (kBucketHistPlaces * 256); i += kRwThreads) st.hist[i] = 0;
}
__device__ __forceinline__ void stage_hist_add(RwStage &, const HitOut &) {}
__device__ __forceinline__ void stage_hist_add(RwStageBk &st, const BucketHitOut &H) {       // behind the last stage_flush's barrier
    for (unsigned int i = threadIdx.x; i < (unsigned int) (H.B.hist_places * 256); i += kRwThreads)
        if (st.hist[i]) atomicAdd(&H.B.hist[i], (unsigned long long) st.hist[i]);
}

// the bucketed form of stage_flush, for the kRwThreads threads of rescore_carry_kernel: every staged hit goes to bucket (key >> shift) & 255
__device__ __forceinline__ void stage_flush(RwStageBk &st, const BucketHitOut &H) {
    constexpr int kPer = RwStageBk::kCap / kRwThreads;
    static_assert(kPer * kRwThreads == RwStageBk::kCap && kOrderBuckets <= kRwThreads, "stage_flush: one pass of the block over the stage");
    __syncthreads();
    const unsigned int n = st.n < (unsigned int) RwStageBk::kCap ? st.n : (unsigned int) RwStageBk::kCap;
    if (threadIdx.x < (unsigned int) kOrderBuckets) st.cnt[threadIdx.x] = 0;
    __syncthreads();
    uint32_t bk[kPer], rank[kPer];
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const unsigned int i = threadIdx.x + (unsigned int) (k * kRwThreads);
        bk[k] = i < n ? (uint32_t) (st.keys[i] >> H.B.shift) & 255u : 0u;
        rank[k] = i < n ? atomicAdd(&st.cnt[bk[k]], 1u) : 0u;
    }
    __syncthreads();
    if (threadIdx.x < (unsigned int) kOrderBuckets && st.cnt[threadIdx.x] > 0) {
        const unsigned int b = threadIdx.x, c = st.cnt[b];
        const unsigned long long f = atomicAdd(&H.B.fill[b], (unsigned long long) c), cap = H.B.cap[b];
        const unsigned long long left = f < cap ? cap - f : 0ULL;
        st.lo[b] = H.B.base[b] + f;
        st.room[b] = left < (unsigned long long) c ? (unsigned int) left : c;
        if (left < (unsigned long long) c) *H.B.overflow = 1ULL;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const unsigned int i = threadIdx.x + (unsigned int) (k * kRwThreads);
        if (i < n && rank[k] < st.room[bk[k]]) {
            const unsigned long long at = st.lo[bk[k]] + rank[k];
            const uint64_t key = st.keys[i];
            if (at < H.cap) { H.keys[at] = key; H.vals[at] = st.vals[i]; }
            count_places(st, H.B, key);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) st.n = 0;
    __syncthreads();
}

// HO / ST: HitOut / RwStage -- the plain hit list; BucketHitOut / RwStageBk -- the bucketed one (the header comment)
template <class HO, class ST>
__global__ void __launch_bounds__(kRwThreads) rescore_carry_kernel(const DevSeq S, const DevPwm Pw, const uint64_t *__restrict__ cand,
                                                                   const unsigned long long *__restrict__ n_cand, uint64_t n_static, uint64_t cand_cap,
                                                                   const FieldMeta *__restrict__ field_meta, int strand_mask, const HO H) {
    extern __shared__ uint4 rw_lds4[];
    uint64_t *s_cw = reinterpret_cast<uint64_t *>(rw_lds4);                                 // [kRwChunk] the window's codes
    uint64_t *s_gk = s_cw + kRwChunk;                                                       // [kRwChunk] hit coordinate << 8 | room (bases to the region's end, <= 255)
    uint32_t *s_nw = reinterpret_cast<uint32_t *>(s_gk + kRwChunk);                         // [kRwChunk] the window's non-ACGT bits
    uint32_t *s_gf = s_nw + kRwChunk;                                                       // [kRwChunk] group << 16 | flags (0: nothing)
    uint32_t *bins = s_gf + kRwChunk;                                                       // [kRwBins]
    uint32_t *wave_tot = bins + kRwBins;                                                    // [16]
    ST &st = *reinterpret_cast<ST *>(wave_tot + 32);
    if (threadIdx.x == 0) st.n = 0;
    stage_hist_clear(st);                      // (the chunk loop's first barrier stands between this and the first count)
    unsigned long long n = n_static + *n_cand;
    if (n > cand_cap) n = cand_cap;
    const bool both = strand_mask == 3;
    const int4 *__restrict__ meta4 = reinterpret_cast<const int4 *>(field_meta);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t pmask = H.pbits ? ((1ULL << H.pbits) - 1ULL) : 0ULL;
    const unsigned long long n_chunks = (n + kRwChunk - 1) / kRwChunk;
    for (unsigned long long ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        for (uint32_t i = threadIdx.x; i < (uint32_t) kRwBins; i += kRwThreads) bins[i] = 0;
        __syncthreads();
        {
            // ---- list order: everything that depends on the POSITION
            uint64_t cw[kRwPerThread], gk[kRwPerThread];
            uint32_t nw[kRwPerThread], gf[kRwPerThread], key[kRwPerThread], rank[kRwPerThread];
            int64_t g[kRwPerThread];
            int4 bi[kRwPerThread];
#pragma unroll
            for (int k = 0; k < kRwPerThread; k++) {
                const unsigned long long i = ch * kRwChunk + (unsigned long long) k * kRwThreads + threadIdx.x;
                const uint64_t rec = i < n ? cand[i] : 0ULL;
                g[k] = (int64_t) (rec >> 30);
                gf[k] = (uint32_t) rec & 0x3FFFFFFFu;                                       // group << 16 | flags
                if (!(gf[k] & 0xFFFFu)) { gf[k] = 0; g[k] = 0; }
                bi[k] = S.blkinfo[g[k] >> 6];
                cw[k] = code_window(S.codes, g[k]);
                nw[k] = n_window(S.nmask, g[k]);
            }
#pragma unroll
            for (int k = 0; k < kRwPerThread; k++) {
                const int64_t base = g[k] & ~(int64_t) 63;
                int64_t lo = bi[k].x, o0 = base + bi[k].y, o1 = base + bi[k].z, o2 = base + bi[k].w, r, beg, end;
                if (bi[k].x < 0) {
                    lo = S.blk2reg[g[k] >> 6];
                    o0 = S.offsets[lo]; o1 = S.offsets[lo + 1];
                    o2 = lo + 2 <= S.R ? S.offsets[lo + 2] : o1;
                }
                if (g[k] < o1) { r = lo; beg = o0; end = o1; }
                else if (g[k] < o2) { r = lo + 1; beg = o1; end = o2; }
                else { r = find_region(S, g[k]); beg = S.offsets[r]; end = S.offsets[r + 1]; }      // tiny regions
                const uint64_t coord = H.pbits ? (((uint64_t) r << H.pbits) | (uint64_t) (g[k] - beg)) : (uint64_t) g[k];
                const int64_t room = end - g[k];
                gk[k] = (coord << 8) | (uint64_t) (room > 255 ? 255 : (room < 0 ? 0 : room));
                const uint32_t f = gf[k] & 0xFFFFu;
                const uint32_t fl = both ? (f | (f >> 1)) & 0x5555u : f;
                key[k] = fl ? (((gf[k] >> 16) << 4) | (uint32_t) (__ffs((int) fl) - 1)) & (uint32_t) (kRwBins - 1) : (uint32_t) (kRwBins - 1);
            }
#pragma unroll
            for (int k = 0; k < kRwPerThread; k++) rank[k] = atomicAdd(&bins[key[k]], 1u);
            __syncthreads();
            {   // exclusive prefix over the bins: four per thread, wave scans, wave totals
                const uint32_t b0 = bins[4 * threadIdx.x], b1 = bins[4 * threadIdx.x + 1], b2 = bins[4 * threadIdx.x + 2], b3 = bins[4 * threadIdx.x + 3];
                const uint32_t tot = b0 + b1 + b2 + b3;
                uint32_t v = tot;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t o = __shfl_up(v, d);
                    if ((int) lane >= d) v += o;
                }
                if (lane == 63u) wave_tot[wave] = v;
                __syncthreads();
                uint32_t base = 0;
                for (uint32_t w = 0; w < wave; w++) base += wave_tot[w];
                const uint32_t excl = base + v - tot;
                bins[4 * threadIdx.x] = excl;
                bins[4 * threadIdx.x + 1] = excl + b0;
                bins[4 * threadIdx.x + 2] = excl + b0 + b1;
                bins[4 * threadIdx.x + 3] = excl + b0 + b1 + b2;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kRwPerThread; k++) {
                const uint32_t at = bins[key[k]] + rank[k];
                s_cw[at] = cw[k]; s_gk[at] = gk[k]; s_nw[at] = nw[k]; s_gf[at] = gf[k];
            }
        }
        __syncthreads();
        // ---- motif order: two rounds of two candidates per thread, per-motif reads only
        for (int round = 0; round < 2; round++) {
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const uint32_t at = (uint32_t) (round * 2 + u) * kRwThreads + threadIdx.x;
                const uint32_t gfu = s_gf[at];
                const uint32_t f = gfu & 0xFFFFu;
                uint32_t flags = both ? (f | (f >> 1)) & 0x5555u : f;
                if (!flags) continue;
                const uint64_t cwu = s_cw[at], gku = s_gk[at];
                const uint32_t nwu = s_nw[at];
                const int32_t group = (int32_t) (gfu >> 16);
                const int room = (int) (gku & 0xFFu);
                const int64_t coord = (int64_t) (gku >> 8);
                while (flags) {
                    const int field = __ffs((int) flags) - 1;
                    flags &= flags - 1u;
                    const int4 f4 = meta4[group * kGroupFields + field];
                    const int32_t m = f4.x;
                    const int w = f4.y;
                    if (m < 0) continue;
                    if (w > room) continue;                                  // window runs past its region (cscore.c:340)
                    double fwd, rev;
                    if (w <= 32 && Pw.tab32) score_window32(Pw.tab2, (uint32_t) f4.z, Pw.zero_bytes, w, cwu, nwu, fwd, rev);
                    else {
                        const int64_t gpos = H.pbits ? S.offsets[coord >> H.pbits] + (int64_t) ((uint64_t) coord & pmask) : coord;
                        score_window(S, Pw.tab2 + Pw.tab_off[m], w, gpos, fwd, rev);
                    }
                    test_and_stage(st, H, Pw, (uint32_t) m, coord, fwd, rev, strand_mask, __int_as_float(f4.w));
                }
            }
            stage_flush(st, H);
        }
    }
    stage_hist_add(st, H);
}

template <class ST>
static size_t rescore_carry_lds_bytes() { return (size_t) kRwChunk * 24 + (size_t) kRwBins * 4 + 32 * 4 + sizeof(ST) + 64; }
int rescore_carry_set_lds() {
    MS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(rescore_carry_kernel<HitOut, RwStage>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int) rescore_carry_lds_bytes<RwStage>()));
    MS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(rescore_carry_kernel<BucketHitOut, RwStageBk>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int) rescore_carry_lds_bytes<RwStageBk>()));
    return MS_OK;
}
int launch_rescore_carry(const DevSeq &S, const DevPwm &Pw, const uint64_t *cand, const unsigned long long *n_cand, uint64_t n_static,
                         uint64_t cand_cap, const FieldMeta *field_meta, int strand_mask, const HitOut &H, int n_blocks, hipStream_t st) {
    hipLaunchKernelGGL((rescore_carry_kernel<HitOut, RwStage>), dim3((unsigned) n_blocks), dim3(kRwThreads), rescore_carry_lds_bytes<RwStage>(), st, S, Pw,
                       cand, n_cand, n_static, cand_cap, field_meta, strand_mask, H);
    MS_HIP(hipGetLastError());
    return MS_OK;
}
int launch_rescore_carry_bucketed(const DevSeq &S, const DevPwm &Pw, const uint64_t *cand, const unsigned long long *n_cand, uint64_t n_static,
                                  uint64_t cand_cap, const FieldMeta *field_meta, int strand_mask, const HitOut &H, const BucketOut &B, int n_blocks,
                                  hipStream_t st) {
    BucketHitOut HB;
    static_cast<HitOut &>(HB) = H;
    HB.B = B;
    hipLaunchKernelGGL((rescore_carry_kernel<BucketHitOut, RwStageBk>), dim3((unsigned) n_blocks), dim3(kRwThreads), rescore_carry_lds_bytes<RwStageBk>(), st,
                       S, Pw, cand, n_cand, n_static, cand_cap, field_meta, strand_mask, HB);
    MS_HIP(hipGetLastError());
    return MS_OK;
}

}  // namespace ms
