// ms_order.hip -- the last step of a scan's ordering: sorted hit keys -> seq_idx, pos, strand, per-motif offsets and region counts.
// Which kernels run depends on the key layout (HitOut, ms_kernels.h) and on the key bits the radix passes covered (scan_back):
//   pbits > 0 (region, position in it), sorted over [L, end_bit), L > 0   order_finalize_kernel, order_overflow_kernel: a region set's usual path
//   pbits > 0, sorted over every bit (short lists, ms_scan_regions_once)  finalize_rp_kernel: only bits to unpack
//   pbits == 0 (global base position: regions too long for the field)     sort_fixup_kernel if the sort left out the low kSortLowBits, then
//                                                                         finalize_kernel, which looks every hit's region up
//   either layout, a scan with predicted sizes                            fill_tail_kernel first: all-ones keys behind the hits sort last
//   ... whose fp64 stage wrote the hits in buckets of the digit at L       bucket_plan_kernel in front of the fp64 stage (the buckets' places for
//   (ms_fp64.hip's header; L > 0, pbits > 0)                              this scan), fill_tail_buckets_kernel behind it: all-ones keys into every
//                                                                         bucket's unused slots, the hit count from the buckets' fills
//
// A bucketed list is ordered by the digit (key >> L) & 255 already, but for the all-ones keys strewn through it.  The radix passes then cover
// [L + 8, end_bit) only: they are stable, so hits that agree in those bits keep the list's order -- ascending in the digit at L -- and the
// all-ones keys, wherever they stood, end up behind every hit.  order_finalize_kernel sees what three passes used to leave it.
//
// The radix passes (ms_sort.hip) order the keys over the bits [L, end_bit) only.  Hits that agree in those bits -- a RUN -- are then
// neighbours, in no particular order among themselves.  order_finalize_kernel finishes the order of every run in LDS and writes the
// result arrays in the same pass: seq_idx, pos and strand, the score moved to its final slot of d_score, the per-motif offsets and
// the per-motif region counts (the semantics of finalize_rp_kernel, below).  This replaces a fix-up kernel plus a finalize
// kernel (one read of keys and scores fewer), and L up to 24 lets the radix sort drop up to two of its eight-bit passes.
//
//   order_finalize_kernel  block b owns the runs that START in slots [b * kTile, (b + 1) * kTile); it stages the keys of those slots and of
//                          the kExt after them in LDS, ranks each element inside its run (a scan's keys are distinct: no ties),
//                          and decodes.  A run that does not close inside the staged window, or that is longer than run_cap, goes to
//                          the overflow list instead (an atomic append of its first slot).
//   order_overflow_kernel  one block per listed run (grid-stride over the list): finds the run's end, sorts it by an LSD radix sort
//                          of eight-bit digits in global memory (ping-pong with the scan's spare key / score buffers, stable by wave
//                          ballots), then decodes it like the kernel above.  Correct for a run as long as the whole list.
//
// Per-motif offsets and region counts need each hit's predecessor in the FINAL order.  Inside a run that is the sorted neighbour.  For
// the first hit of a run it is the last hit of the previous run -- but every test made on it (motif changed? (motif, region) pair
// changed?) gives the same answer for ANY hit of the previous run: with L <= gbits + 1 the motif bits are above L, so they are the
// same for the whole run; the pair bits are either above L too (L <= pbits + 1), or they include bits above L, which differ between
// two runs, so the pair changes.  The radix-order predecessor is therefore enough, and no block depends on another block's output.
#include <algorithm>
#include <cmath>

#include "ms_device.h"

namespace ms {

namespace {

constexpr int kOrderThreads = 256;
// order_finalize_kernel<kTile, kExt>: kTile slots a block owns the run starts of, kExt slots staged past them to close the tile's last run.
// Every run of <= kExt hits is sorted in LDS, whatever kExt is; a longer one that does not close inside the window goes to the overflow kernel.
// The slots past the tile are read twice (by this block and by the one that owns them), so the host takes the short extension where the
// expected run n / (P x 2^(gbits + 1 - L)) is at most kOrderShortMeanRun hits.  That is the mean over the motifs, and a motif set's hit
// rates are far from equal: the benchmark's busiest motif hits 21 times as often as the average one.  At its L = 16 (mean run 6.8, the
// busiest motif's 142) 26 % of the hits stand in runs of more than 64, and a 960 + 64 window would leave 0.8 % of them (7 000 runs a scan)
// to the overflow kernel; 1024 + 256 leaves 3e-22.  A mean of at most one hit keeps the busiest motif's runs near 20.
constexpr int kOrderTileShort = 960, kOrderExtShort = 64;      // 1024 staged slots, 6.7 % of them read twice; 12.2 KB of LDS per block
constexpr int kOrderTileLong = 1024, kOrderExtLong = 256;      // 1280 staged slots, 25 % read twice; 15.2 KB (the form before: 31.5)
constexpr double kOrderShortMeanRun = 1.0;
constexpr int kOverflowBlocks = 256;

struct OrderRun {
    int64_t start;      // first slot of the run
    uint64_t prev;      // a key of the run in front of it (start > 0)
};

struct OrderOut {
    int64_t *seq_idx;
    int64_t *pos;
    int8_t *strand;
    double *score;
    int64_t *motif_first;
    unsigned long long *region_counts;
    int rbits, pbits;
    int32_t P;
};

// one hit at final slot g: key k, score v, predecessor pk (has_prev: g > 0).  Returns whether it opens a (motif, region) pair.
__device__ __forceinline__ bool decode_hit(const OrderOut &O, int64_t g, int64_t n, uint64_t k, double v, bool has_prev, uint64_t pk,
                                           uint32_t *motif_out) {
    const int ms = O.rbits + O.pbits + 1;
    const uint64_t pair = k >> (O.pbits + 1);
    const uint32_t motif = (uint32_t) (k >> ms);
    O.seq_idx[g] = (int64_t) (pair & ((1ULL << O.rbits) - 1ULL));
    O.pos[g] = (int64_t) ((k >> 1) & ((1ULL << O.pbits) - 1ULL));
    O.strand[g] = (int8_t) ((k & 1ULL) ? 2 : 1);
    O.score[g] = v;
    const uint32_t pm = has_prev ? (uint32_t) (pk >> ms) : 0u;
    if (!has_prev || pm != motif)                                       // every motif after the previous hit's up to this one starts here
        for (int64_t q = has_prev ? (int64_t) pm + 1 : 0; q <= (int64_t) motif; q++) O.motif_first[q] = g;
    if (g == n - 1)                                                    // motifs after the last hit: empty
        for (int64_t q = (int64_t) motif + 1; q <= O.P; q++) O.motif_first[q] = n;
    *motif_out = motif;
    return !has_prev || (pk >> (O.pbits + 1)) != pair;
}

// regions with >= 1 hit per motif (stats.py:29-31): one add per (wave, motif), into the block's LDS counters for the motifs
// [m_base, m_base + kOrderMotifSlots) (lds != nullptr), else straight to the global ones.  Every lane of the wave calls this.
constexpr int kOrderMotifSlots = 8;
__device__ __forceinline__ void count_pairs(unsigned long long *region_counts, bool new_pair, uint32_t motif, unsigned int *lds, uint32_t m_base) {
    unsigned long long todo = __ballot(new_pair);
    while (todo) {
        const int leader = __ffsll((long long) todo) - 1;
        const uint32_t m = __shfl(motif, leader);
        const unsigned long long same = __ballot(new_pair && motif == m);
        if ((int) (threadIdx.x & 63) == leader) {
            if (lds && m - m_base < (uint32_t) kOrderMotifSlots) atomicAdd(&lds[m - m_base], (unsigned int) __popcll(same));
            else atomicAdd(&region_counts[m], (unsigned long long) __popcll(same));
        }
        todo &= ~same;
    }
}

// Slot i = tid + kOrderThreads * k of the staged window is thread tid's k-th: its key and score stay in registers from the load to the
// stores, and its wave's ballot of run starts (one 64-slot segment) gives the run's bounds without walking the keys, unless a bound lies in
// another segment (seg_first / seg_last).  The keys are all LDS holds: the rank loop over a hit's run gives its final slot and, as the
// largest smaller key, its predecessor there, so every hit is decoded and stored from its own thread's registers -- the stores of a wave
// fall into the cache lines of its 64 slots (and of a run that straddles them), in another order.
template <int kTile, int kExt>
__global__ void __launch_bounds__(kOrderThreads) order_finalize_kernel(const uint64_t *__restrict__ keys, int64_t n, const unsigned long long *__restrict__ n_dev,
                                                                      int L, int run_cap, OrderOut O, OrderRun *__restrict__ ovf,
                                                                      unsigned long long *__restrict__ ovf_n, uint64_t ovf_cap) {
    constexpr int kWin = kTile + kExt, kPer = kWin / kOrderThreads, kSegs = kWin / 64;
    static_assert(kWin % kOrderThreads == 0 && kTile % 64 == 0 && kExt % 64 == 0, "whole waves per round, whole segments per tile");
    __shared__ uint64_t K[kWin];               // radix order
    __shared__ uint32_t K32[kWin];             // its low words, for the rank loop
    __shared__ int seg_first[kSegs], seg_last[kSegs];                // first / last run start of each 64-slot segment (none: kWin / -1)
    __shared__ unsigned int rc[kOrderMotifSlots];                    // the block's region counts of its first motifs (a block of a long list spans one or two)
    if (n_dev) { const unsigned long long nd = *n_dev; if ((unsigned long long) n > nd) n = (int64_t) nd; }
    const int64_t s0 = (int64_t) blockIdx.x * kTile;
    if (s0 >= n) return;
    const int tid = (int) threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wn = (int) std::min<int64_t>(kWin, n - s0);           // staged slots
    const int tn = std::min(kTile, wn);                               // owned run starts lie in [0, tn)
    uint64_t kr[kPer];
    double vr[kPer];                           // (scores of slots another block owns are read too, and never used)
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const int i = tid + kOrderThreads * k;
        kr[k] = i < wn ? keys[s0 + i] : ~0ULL;
        vr[k] = i < wn ? O.score[s0 + i] : 0.0;
        K[i] = kr[k];
        K32[i] = (uint32_t) kr[k];
    }
    if (tid < kOrderMotifSlots) rc[tid] = 0;
    const uint64_t prevk = s0 > 0 ? keys[s0 - 1] : 0ULL;
    __syncthreads();
    unsigned long long msk[kPer];              // run starts of each of this thread's segments
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const int i = tid + kOrderThreads * k;
        const bool start = i < wn && (i == 0 ? (s0 == 0 || (prevk >> L) != (kr[k] >> L)) : (K[i - 1] >> L) != (kr[k] >> L));
        msk[k] = __ballot(start);
        if (lane == 0) {
            const int seg = w + (kOrderThreads / 64) * k;
            seg_first[seg] = msk[k] ? seg * 64 + __ffsll((long long) msk[k]) - 1 : kWin;
            seg_last[seg] = msk[k] ? seg * 64 + 63 - __clzll((long long) msk[k]) : -1;
        }
    }
    __syncthreads();
    int lo = kWin, hi = wn;                    // owned slots: [lo, hi) -- from the first run start in the tile to the first one past it
    for (int q = 0; q < kSegs; q++) lo = std::min(lo, seg_first[q]);
    if (tn == kTile)
        for (int q = kTile / 64; q < kSegs; q++) hi = std::min(hi, seg_first[q]);
    if (lo >= tn) return;                      // no run starts in this tile
    const bool closed = hi < wn || s0 + wn == n;                      // else the last owned run runs on past the window
    const int ms = O.rbits + O.pbits + 1;
    const uint32_t m_base = (uint32_t) (K[lo] >> ms);
    const unsigned long long le = lane == 63 ? ~0ULL : (2ULL << lane) - 1ULL;
#pragma unroll
    for (int k = 0; k < kPer; k++) {           // whole waves: count_pairs
        const int i = tid + kOrderThreads * k, seg = w + (kOrderThreads / 64) * k;
        bool new_pair = false;
        uint32_t motif = 0;
        if (i >= lo && i < hi) {
            int a = -1, b = wn;
            if (msk[k] & le) a = seg * 64 + 63 - __clzll((long long) (msk[k] & le));
            else for (int q = seg - 1; q >= 0 && a < 0; q--) a = seg_last[q];
            if (msk[k] & ~le) b = seg * 64 + __ffsll((long long) (msk[k] & ~le)) - 1;
            else for (int q = seg + 1; q < kSegs && b == wn; q++) b = std::min(wn, seg_first[q]);
            if ((b == hi && !closed) || b - a > run_cap) {
                if (i == a) {
                    const unsigned long long e = atomicAdd(ovf_n, 1ULL);
                    if (e < ovf_cap) ovf[e] = OrderRun{s0 + a, a > 0 ? K[a - 1] : prevk};
                }
            } else {
                // rank in the run, and the largest key of the run under this one (a scan's keys are distinct).  This loop is where the
                // kernel's instructions go once runs are long (a wave takes as many turns as its longest run has hits), so with
                // L <= 32 it compares the keys' low words only -- the run agrees in every bit from L up -- four to a turn.
                int rank = 0;
                uint64_t below = 0ULL;
                if (L <= 32) {
                    const uint32_t me = (uint32_t) kr[k];
                    uint32_t under = 0u;
                    int j = a;
                    for (; j + 4 <= b; j += 4) {
                        const uint32_t k0 = K32[j], k1 = K32[j + 1], k2 = K32[j + 2], k3 = K32[j + 3];
                        rank += (k0 < me ? 1 : 0) + (k1 < me ? 1 : 0) + (k2 < me ? 1 : 0) + (k3 < me ? 1 : 0);
                        under = std::max(std::max(under, k0 < me ? k0 : 0u), k1 < me ? k1 : 0u);
                        under = std::max(std::max(under, k2 < me ? k2 : 0u), k3 < me ? k3 : 0u);
                    }
                    for (; j < b; j++) {
                        const uint32_t kj = K32[j];
                        rank += kj < me ? 1 : 0;
                        under = std::max(under, kj < me ? kj : 0u);
                    }
                    below = (kr[k] & ~0xFFFFFFFFULL) | under;
                } else {
                    for (int j = a; j < b; j++) {
                        const uint64_t kj = K[j];
                        if (kj < kr[k]) { rank++; below = std::max(below, kj); }
                    }
                }
                // the run's first hit in the final order: its predecessor is any hit of the run in front (the header's last paragraph)
                const uint64_t pk = rank > 0 ? below : (a > 0 ? K[a - 1] : prevk);
                const int64_t g = s0 + a + rank;
                new_pair = decode_hit(O, g, n, kr[k], vr[k], g > 0, pk, &motif);
            }
        }
        count_pairs(O.region_counts, new_pair, motif, rc, m_base);
    }
    __syncthreads();
    if (tid < kOrderMotifSlots && rc[tid]) atomicAdd(&O.region_counts[m_base + tid], (unsigned long long) rc[tid]);
}

__global__ void __launch_bounds__(kOrderThreads) order_overflow_kernel(uint64_t *keys, uint64_t *tmp_keys, double *tmp_vals,
                                                                      int64_t n, const unsigned long long *__restrict__ n_dev, int L, OrderOut O,
                                                                      const OrderRun *__restrict__ ovf, const unsigned long long *__restrict__ ovf_n,
                                                                      uint64_t ovf_cap) {
    __shared__ uint32_t base[256];
    __shared__ uint32_t wcnt[kOrderThreads / 64][256];
    __shared__ int64_t s_end;
    if (n_dev) { const unsigned long long nd = *n_dev; if ((unsigned long long) n > nd) n = (int64_t) nd; }
    const unsigned long long cnt = std::min<unsigned long long>(*ovf_n, ovf_cap);
    const int tid = (int) threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long lt = (1ULL << lane) - 1ULL;
    for (unsigned long long e = blockIdx.x; e < cnt; e += gridDim.x) {
        const int64_t s = ovf[e].start;
        const uint64_t prev = ovf[e].prev;
        const uint64_t h = keys[s] >> L;       // (only this block moves the run's keys; another block's run never holds these bits)
        if (tid == 0) s_end = n;
        __syncthreads();
        for (int64_t c = s + 1; c < n; c += kOrderThreads) {
            const int64_t j = c + tid;
            if (j < n && (keys[j] >> L) != h) atomicMin((unsigned long long *) &s_end, (unsigned long long) j);
            __syncthreads();
            if (s_end < n) break;
            __syncthreads();
        }
        const int64_t b = s_end;
        uint64_t *sk = keys, *dk = tmp_keys;
        double *sv = O.score, *dv = tmp_vals;
        for (int shift = 0; shift < L; shift += 8) {
            base[tid] = 0;
            for (int q = 0; q < kOrderThreads / 64; q++) wcnt[q][tid] = 0;
            __syncthreads();
            for (int64_t j = s + tid; j < b; j += kOrderThreads) atomicAdd(&base[(uint32_t) (sk[j] >> shift) & 255u], 1u);
            __syncthreads();
            if (tid == 0) {
                uint32_t acc = 0;
                for (int d = 0; d < 256; d++) { const uint32_t c = base[d]; base[d] = acc; acc += c; }
            }
            __syncthreads();
            for (int64_t c = s; c < b; c += kOrderThreads) {          // stable scatter, 256 hits at a time
                const int64_t j = c + tid;
                const bool live = j < b;
                const uint64_t k = live ? sk[j] : 0ULL;
                const double v = live ? sv[j] : 0.0;
                const uint32_t d = (uint32_t) (k >> shift) & 255u;
                unsigned long long peers = __ballot(live);
#pragma unroll
                for (int bit = 0; bit < 8; bit++) {
                    const unsigned long long m = __ballot((d >> bit) & 1u);
                    peers &= ((d >> bit) & 1u) ? m : ~m;
                }
                if (live && (peers >> lane) == 1ULL) wcnt[w][d] = (uint32_t) __popcll(peers);   // the last lane of its digit in the wave
                __syncthreads();
                if (live) {
                    uint32_t off = base[d] + (uint32_t) __popcll(peers & lt);
                    for (int q = 0; q < w; q++) off += wcnt[q][d];
                    dk[s + off] = k;
                    dv[s + off] = v;
                }
                __syncthreads();
                uint32_t add = 0;
                for (int q = 0; q < kOrderThreads / 64; q++) { add += wcnt[q][tid]; wcnt[q][tid] = 0; }
                base[tid] += add;
                __syncthreads();
            }
            uint64_t *tk = sk; sk = dk; dk = tk;
            double *tv = sv; sv = dv; dv = tv;
        }
        for (int64_t c = s; c < b; c += kOrderThreads) {              // whole waves: count_pairs
            const int64_t j = c + tid;
            bool new_pair = false;
            uint32_t motif = 0;
            if (j < b) new_pair = decode_hit(O, j, n, sk[j], sv[j], j > 0, j == s ? prev : sk[j - 1], &motif);
            count_pairs(O.region_counts, new_pair, motif, nullptr, 0);
        }
        __syncthreads();                       // (s_end and the LDS counters are reused by the next run)
    }
}

}  // namespace

size_t order_overflow_bytes(size_t n, int run_cap) {
    const size_t min_len = (size_t) std::min(std::max(run_cap, 1), kOrderExtShort) + 1;     // every listed run is longer than this minus one, with either extension
    return (n / min_len + 1) * sizeof(OrderRun);
}

int launch_order_finalize(uint64_t *keys, double *score, int64_t n, const unsigned long long *n_dev, int L, int rbits, int pbits, int32_t P,
                          int64_t *seq_idx, int64_t *pos, int8_t *strand, int64_t *motif_first, unsigned long long *region_counts,
                          uint64_t *tmp_keys, double *tmp_vals, void *ovf_buf, size_t ovf_bytes, unsigned long long *ovf_n, int run_cap,
                          hipStream_t st) {
    if (n == 0 || n_dev) {                           // no hits: every per-motif offset is 0 (with n_dev the kernel overwrites them unless the count is 0)
        MS_HIP(hipMemsetAsync(motif_first, 0, ((size_t) P + 1) * sizeof(int64_t), st));
        if (n == 0) return MS_OK;
    }
    run_cap = std::max(run_cap, 1);
    OrderOut O;
    O.seq_idx = seq_idx; O.pos = pos; O.strand = strand; O.score = score; O.motif_first = motif_first; O.region_counts = region_counts;
    O.rbits = rbits; O.pbits = pbits; O.P = P;
    OrderRun *ovf = static_cast<OrderRun *>(ovf_buf);
    const uint64_t ovf_cap = ovf_bytes / sizeof(OrderRun);
    // the expected run: n hits over P x 2^(gbits + 1 - L) values of the key bits above L, gbits = rbits + pbits (scan_geom's order_low_bits)
    const bool short_ext = std::ldexp((double) n / (double) std::max(P, 1), L - rbits - pbits - 1) <= kOrderShortMeanRun;
    const int ext = short_ext ? kOrderExtShort : kOrderExtLong;
    if (short_ext)
        hipLaunchKernelGGL((order_finalize_kernel<kOrderTileShort, kOrderExtShort>), dim3((unsigned) ((n + kOrderTileShort - 1) / kOrderTileShort)),
                           dim3(kOrderThreads), 0, st, keys, n, n_dev, L, run_cap, O, ovf, ovf_n, ovf_cap);
    else
        hipLaunchKernelGGL((order_finalize_kernel<kOrderTileLong, kOrderExtLong>), dim3((unsigned) ((n + kOrderTileLong - 1) / kOrderTileLong)),
                           dim3(kOrderThreads), 0, st, keys, n, n_dev, L, run_cap, O, ovf, ovf_n, ovf_cap);
    MS_HIP(hipGetLastError());
    // a run is only listed when it is longer than run_cap or than the extension: with at most 2^L hits per run, not at L = 8 with the long one by default
    if (L < 63 && (1ULL << L) > (unsigned long long) std::min(run_cap, ext)) {
        hipLaunchKernelGGL(order_overflow_kernel, dim3(kOverflowBlocks), dim3(kOrderThreads), 0, st, keys, tmp_keys, tmp_vals, n, n_dev, L, O,
                           ovf, ovf_n, ovf_cap);
        MS_HIP(hipGetLastError());
    }
    return MS_OK;
}

// --------------------------------------- fill_tail, and the tail of the other two paths --

// keys[i] = all ones for i in [min(*n_dev, cap), cap): the unused rest of a predicted-size hit list sorts behind every hit
__global__ void __launch_bounds__(256) fill_tail_kernel(uint64_t *__restrict__ keys, const unsigned long long *__restrict__ n_dev, uint64_t cap) {
    const unsigned long long n = *n_dev < cap ? *n_dev : cap;
    for (unsigned long long i = n + (unsigned long long) blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += (unsigned long long) gridDim.x * blockDim.x)
        keys[i] = ~0ULL;
}

// The radix sort orders a scan's hits over the key bits ABOVE kSortLowBits only (one eight-bit pass fewer over 62 M pairs of 16 bytes);
// hits that agree in those bits -- the same motif, region and 128-base stretch: a motif's two strands at one position, mostly -- are
// neighbours afterwards, in the order the list held them.  This kernel finishes the order: the first hit of every such run sorts its
// run in place by the whole key (runs hold <= 2^kSortLowBits hits: the keys of a scan are distinct; all-ones padding keys are left alone).
__global__ void __launch_bounds__(256) sort_fixup_kernel(uint64_t *__restrict__ keys, double *__restrict__ vals, int64_t n, const unsigned long long *__restrict__ n_dev) {
    if (n_dev) { const unsigned long long nd = *n_dev; if ((unsigned long long) n > nd) n = (int64_t) nd; }
    const int64_t i0 = ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) * 4;     // four consecutive hits per thread: two 16-byte reads
    if (i0 >= n) return;
    uint64_t k[4] = {0, 0, 0, 0};
    uint64_t hi[6];                                                               // the high bits of hits i0 - 1 ... i0 + 4 (all-ones: none)
    hi[0] = i0 > 0 ? keys[i0 - 1] >> kSortLowBits : ~0ULL;
    if (i0 + 4 <= n) {
        const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(keys + i0), b = *reinterpret_cast<const ulonglong2 *>(keys + i0 + 2);
        k[0] = a.x; k[1] = a.y; k[2] = b.x; k[3] = b.y;
    } else {
        for (int q = 0; q < 4; q++) k[q] = i0 + q < n ? keys[i0 + q] : ~0ULL;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) hi[1 + q] = i0 + q < n ? k[q] >> kSortLowBits : ~0ULL;
    hi[5] = i0 + 4 < n ? keys[i0 + 4] >> kSortLowBits : ~0ULL;
    // (the high bits of a run's members do not change while another thread sorts the run: what is compared here is stable)
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int64_t i = i0 + q;
        if (i + 1 >= n || hi[1 + q] == hi[q] || hi[1 + q] != hi[2 + q]) continue;   // not the first of a run of two or more
        if (q < 3 && hi[3 + q] != hi[1 + q]) {
            // a run of exactly two, both in this thread's registers (a motif's two strands at one position: nearly every run):
            // half of them are in order already and touch nothing more
            if (k[q] > k[q + 1]) {
                keys[i] = k[q + 1];
                keys[i + 1] = k[q];
                const double v0 = vals[i], v1 = vals[i + 1];
                vals[i] = v1;
                vals[i + 1] = v0;
            }
            continue;
        }
        const uint64_t h = hi[1 + q];
        int64_t len = 2;
        while (i + len < n && len < ((int64_t) 1 << kSortLowBits) && (keys[i + len] >> kSortLowBits) == h) len++;
        for (int64_t a = 1; a < len; a++) {                                      // insertion sort: short runs
            const uint64_t ka = keys[i + a];
            const double va = vals[i + a];
            int64_t b = a;
            while (b > 0 && keys[i + b - 1] > ka) { keys[i + b] = keys[i + b - 1]; vals[i + b] = vals[i + b - 1]; b--; }
            keys[i + b] = ka;
            vals[i + b] = va;
        }
    }
}

int launch_sort_fixup(uint64_t *keys, double *vals, int64_t n, const unsigned long long *n_dev, hipStream_t st) {
    if (n == 0) return MS_OK;
    hipLaunchKernelGGL(sort_fixup_kernel, dim3((unsigned) ((n + 1023) / 1024)), dim3(256), 0, st, keys, vals, n, n_dev);
    MS_HIP(hipGetLastError());
    return MS_OK;
}

// The places of the 256 buckets in a list of n_pred slots: the expressions of ms_scan_geom.cpp's bucket_caps, in its order of operations (the
// library is built with -ffp-contract=off, so neither side fuses the multiply-adds; should a capacity still come out a slot apart from the
// host's `need`, the running-sum cut below keeps every bucket inside the list).  The host only needs the sum of the needs, for its gate.  One block of kOrderBuckets threads.  tab: base, cap, fill, then the end of the last bucket (BucketOut, ms_kernels.h).
__global__ void __launch_bounds__(kOrderBuckets) bucket_plan_kernel(const BucketWeights bw, double mu, unsigned long long n_pred, unsigned long long need,
                                                                    unsigned long long cap_max, unsigned long long *__restrict__ tab) {
    __shared__ unsigned long long sum[kOrderBuckets];
    const int b = (int) threadIdx.x;
    const unsigned long long w = bw.w[b];
    unsigned long long cb = 0;
    if (w) {
        const double e = mu * (double) w / (double) bw.total;
        cb = (unsigned long long) ceil(e + 6.0 * __dsqrt_rn(e + 1.0)) + 1ULL;
        const unsigned long long extra = n_pred > need ? n_pred - need : 0ULL;
        cb += (unsigned long long) floor((double) extra * (double) w / (double) bw.total);
    }
    if (cb > cap_max) cb = cap_max;
    sum[b] = cb;
    __syncthreads();
    for (int d = 1; d < kOrderBuckets; d <<= 1) {
        const unsigned long long v = b >= d ? sum[b - d] : 0ULL;
        __syncthreads();
        sum[b] += v;
        __syncthreads();
    }
    const unsigned long long at = sum[b] - cb, base = at < n_pred ? at : n_pred;
    tab[b] = base;
    tab[kOrderBuckets + b] = cb < n_pred - base ? cb : n_pred - base;
    tab[2 * kOrderBuckets + b] = 0ULL;
    for (int p = 0; p < kBucketHistPlaces; p++) tab[kBucketHistAt + (size_t) p * 256 + b] = 0ULL;      // the digit counts (BucketOut::hist)
    if (b == kOrderBuckets - 1) tab[3 * kOrderBuckets] = sum[b] < n_pred ? sum[b] : n_pred;
}

// grid (x, kOrderBuckets + 1): row b < kOrderBuckets fills the unused slots of bucket b, the last row the slots behind the last bucket; its first block
// also sums the hits the buckets HOLD into *n_hits (what order_finalize_kernel reads as the list's length -- a dropped hit must not count: the slot
// it would stand for holds an all-ones key, whose "motif" no decode may touch; the scan is run again anyway, *overflow says so).  hist != nullptr:
// that block also adds the all-ones keys of the whole list -- every slot of the n_pred that holds no hit -- to the digit counts, place by
// place: bin 255, or the last place's 2^last_bits - 1 where the passes end inside it (a radix pass reads no bit at or above its end bit).
__global__ void __launch_bounds__(256) fill_tail_buckets_kernel(uint64_t *__restrict__ keys, const unsigned long long *__restrict__ tab, uint64_t n_pred,
                                                                unsigned long long *__restrict__ n_hits, unsigned long long *__restrict__ overflow,
                                                                unsigned long long *__restrict__ hist, int places, int last_bits) {
    const unsigned int b = blockIdx.y;
    unsigned long long lo, hi;
    if (b < (unsigned int) kOrderBuckets) {
        const unsigned long long base = tab[b], cap = tab[kOrderBuckets + b], fill = tab[2 * kOrderBuckets + b];
        lo = base + (fill < cap ? fill : cap);
        hi = base + cap;
        if (fill > cap && blockIdx.x == 0 && threadIdx.x == 0) *overflow = 1ULL;
    } else {
        lo = tab[3 * kOrderBuckets];
        hi = n_pred;
        if (blockIdx.x == 0) {
            __shared__ unsigned long long part[256];
            unsigned long long v = 0;
            for (int q = (int) threadIdx.x; q < kOrderBuckets; q += 256) {
                const unsigned long long cap = tab[kOrderBuckets + q], fill = tab[2 * kOrderBuckets + q];
                v += fill < cap ? fill : cap;
            }
            part[threadIdx.x] = v;
            __syncthreads();
            for (int d = 128; d > 0; d >>= 1) {
                if ((int) threadIdx.x < d) part[threadIdx.x] += part[threadIdx.x + d];
                __syncthreads();
            }
            if (threadIdx.x == 0) *n_hits = part[0];
            if (hist && (int) threadIdx.x < places && part[0] < n_pred)
                hist[threadIdx.x * 256 + ((int) threadIdx.x == places - 1 ? (1u << last_bits) - 1u : 255u)] += n_pred - part[0];
        }
    }
    if (hi > n_pred) hi = n_pred;
    for (unsigned long long i = lo + (unsigned long long) blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (unsigned long long) gridDim.x * blockDim.x)
        keys[i] = ~0ULL;
}

int launch_bucket_plan(const BucketWeights &bw, double mu, unsigned long long n_pred, unsigned long long need, unsigned long long cap_max,
                       unsigned long long *tab, hipStream_t st) {
    hipLaunchKernelGGL(bucket_plan_kernel, dim3(1), dim3(kOrderBuckets), 0, st, bw, mu, n_pred, need, cap_max, tab);
    MS_HIP(hipGetLastError());
    return MS_OK;
}

int launch_fill_tail_buckets(uint64_t *keys, const unsigned long long *tab, uint64_t n_pred, unsigned long long *n_hits, unsigned long long *overflow,
                             unsigned long long *hist, int hist_places, int hist_last_bits, hipStream_t st) {
    hipLaunchKernelGGL(fill_tail_buckets_kernel, dim3(16, kOrderBuckets + 1), dim3(256), 0, st, keys, tab, n_pred, n_hits, overflow, hist,
                       hist_places, hist_last_bits);
    MS_HIP(hipGetLastError());
    return MS_OK;
}

int launch_fill_tail(uint64_t *keys, const unsigned long long *n_dev, uint64_t cap, hipStream_t st) {
    if (cap == 0) return MS_OK;
    hipLaunchKernelGGL(fill_tail_kernel, dim3(256), dim3(256), 0, st, keys, n_dev, cap);
    MS_HIP(hipGetLastError());
    return MS_OK;
}

// n_dev != nullptr: the number of hits is only known on the device (a scan whose sizes were predicted, scan_locked): n is then
// the launch's capacity and the true count min(*n_dev, n) is read here.
__global__ void __launch_bounds__(256) finalize_kernel(const uint64_t *__restrict__ keys, int64_t n, const unsigned long long *__restrict__ n_dev,
                                                       int gbits, int32_t P, const DevSeq S,
                                                       int64_t *__restrict__ seq_idx, int64_t *__restrict__ pos,
                                                       int8_t *__restrict__ strand, int64_t *__restrict__ motif_first,
                                                       unsigned long long *__restrict__ region_counts) {
    if (n_dev) { const unsigned long long nd = *n_dev; if ((unsigned long long) n > nd) n = (int64_t) nd; }
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    uint32_t motif = 0xFFFFFFFFu;
    bool new_pair = false;
    if (live) {
        const uint64_t k = keys[i];
        const uint64_t gmask = (1ULL << gbits) - 1ULL;
        const int64_t g = (int64_t) ((k >> 1) & gmask);
        motif = (uint32_t) (k >> (gbits + 1));
        const int64_t r = find_region(S, g);
        seq_idx[i] = r;
        pos[i] = g - S.offsets[r];
        strand[i] = (int8_t) ((k & 1ULL) ? 2 : 1);
        bool first_of_motif = (i == 0);
        new_pair = true;
        int64_t q0 = 0;                                  // per-motif offsets: every motif after the previous hit's up to this one starts here
        if (i > 0) {
            const uint64_t kp = keys[i - 1];
            const uint32_t mp = (uint32_t) (kp >> (gbits + 1));
            first_of_motif = mp != motif;
            q0 = (int64_t) mp + 1;
            if (!first_of_motif) {
                const int64_t gp = (int64_t) ((kp >> 1) & gmask);
                new_pair = gp < S.offsets[r];            // previous hit of this motif lies in an earlier region
            }
        }
        if (first_of_motif) for (int64_t q = q0; q <= (int64_t) motif; q++) motif_first[q] = i;
        if (i == n - 1) for (int64_t q = (int64_t) motif + 1; q <= P; q++) motif_first[q] = n;     // motifs after the last hit: empty
    }
    // number of regions with >= 1 hit per motif (stats.py:29-31): one atomic per (wave, motif)
    unsigned long long todo = __ballot(live && new_pair);
    while (todo) {
        const int leader = __ffsll((long long) todo) - 1;
        const uint32_t m = __shfl(motif, leader);
        const unsigned long long same = __ballot(live && new_pair && motif == m);
        if ((int) (threadIdx.x & 63) == leader) atomicAdd(&region_counts[m], (unsigned long long) __popcll(same));
        todo &= ~same;
    }
}

// The same when the keys carry (region, position inside the region): nothing to look up, only bits to unpack.
// Four consecutive hits per thread: 16-byte loads and stores, the four strand bytes as one word.
__global__ void __launch_bounds__(256) finalize_rp_kernel(const uint64_t *__restrict__ keys, int64_t n, const unsigned long long *__restrict__ n_dev,
                                                          int rbits, int pbits, int32_t P,
                                                          int64_t *__restrict__ seq_idx, int64_t *__restrict__ pos,
                                                          int8_t *__restrict__ strand, int64_t *__restrict__ motif_first,
                                                          unsigned long long *__restrict__ region_counts) {
    if (n_dev) { const unsigned long long nd = *n_dev; if ((unsigned long long) n > nd) n = (int64_t) nd; }
    const int64_t i0 = 4 * ((int64_t) blockIdx.x * blockDim.x + threadIdx.x);
    const bool live = i0 < n;
    uint32_t motif0 = 0xFFFFFFFFu;
    int n_new = 0;                                              // new (motif, region) pairs among this thread's hits of motif0
    if (live) {
        uint64_t k[4];
        const bool full = i0 + 4 <= n;
        if (full) {
            const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(keys + i0), b2 = *reinterpret_cast<const ulonglong2 *>(keys + i0 + 2);
            k[0] = a.x; k[1] = a.y; k[2] = b2.x; k[3] = b2.y;
        } else {
            for (int j = 0; j < 4; j++) k[j] = i0 + j < n ? keys[i0 + j] : 0;
        }
        uint64_t prev = i0 > 0 ? keys[i0 - 1] >> (pbits + 1) : ~0ULL;
        int64_t sq[4], ps[4];
        uint32_t sd = 0;
        const uint64_t rmask = (1ULL << rbits) - 1ULL, pmask = (1ULL << pbits) - 1ULL;
        motif0 = (uint32_t) (k[0] >> (pbits + 1 + rbits));
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (i0 + j < n) {
                const uint64_t pair = k[j] >> (pbits + 1);      // (motif, region)
                const uint32_t motif = (uint32_t) (pair >> rbits);
                sq[j] = (int64_t) (pair & rmask);
                ps[j] = (int64_t) ((k[j] >> 1) & pmask);
                sd |= ((k[j] & 1ULL) ? 2u : 1u) << (8 * j);
                if (prev == ~0ULL || (uint32_t) (prev >> rbits) != motif)        // every motif after the previous hit's up to this one starts here
                    for (int64_t q = prev == ~0ULL ? 0 : (int64_t) (uint32_t) (prev >> rbits) + 1; q <= (int64_t) motif; q++) motif_first[q] = i0 + j;
                if (i0 + j == n - 1) for (int64_t q = (int64_t) motif + 1; q <= P; q++) motif_first[q] = n;   // motifs after the last hit: empty
                if (prev != pair) {
                    if (motif == motif0) n_new++;
                    else atomicAdd(&region_counts[motif], 1ULL);    // a thread's hits rarely span two motifs
                }
                prev = pair;
            }
        }
        if (full) {
            *reinterpret_cast<longlong2 *>(seq_idx + i0) = make_longlong2(sq[0], sq[1]);
            *reinterpret_cast<longlong2 *>(seq_idx + i0 + 2) = make_longlong2(sq[2], sq[3]);
            *reinterpret_cast<longlong2 *>(pos + i0) = make_longlong2(ps[0], ps[1]);
            *reinterpret_cast<longlong2 *>(pos + i0 + 2) = make_longlong2(ps[2], ps[3]);
            *reinterpret_cast<uint32_t *>(strand + i0) = sd;
        } else {
            for (int j = 0; j < 4 && i0 + j < n; j++) { seq_idx[i0 + j] = sq[j]; pos[i0 + j] = ps[j]; strand[i0 + j] = (int8_t) ((sd >> (8 * j)) & 0xFFu); }
        }
    }
    // regions with >= 1 hit per motif (stats.py:29-31): one atomic per (wave, motif)
    unsigned long long todo = __ballot(live && n_new > 0);
    while (todo) {
        const int leader = __ffsll((long long) todo) - 1;
        const uint32_t m = __shfl(motif0, leader);
        const unsigned long long same = __ballot(live && n_new > 0 && motif0 == m);
        int v = (live && motif0 == m) ? n_new : 0;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
        if ((int) (threadIdx.x & 63) == leader) atomicAdd(&region_counts[m], (unsigned long long) v);
        todo &= ~same;
    }
}

int launch_finalize(const uint64_t *keys, int64_t n, const unsigned long long *n_dev, int gbits, int rbits, int pbits, int32_t P, const DevSeq &S,
                    int64_t *seq_idx, int64_t *pos, int8_t *strand, int64_t *motif_first, unsigned long long *region_counts,
                    hipStream_t st) {
    if (n == 0 || n_dev) {                           // no hits: every per-motif offset is 0 (with n_dev the kernel overwrites them unless the count is 0)
        MS_HIP(hipMemsetAsync(motif_first, 0, ((size_t) P + 1) * sizeof(int64_t), st));
        if (n == 0) return MS_OK;
    }
    if (pbits > 0) {
        hipLaunchKernelGGL(finalize_rp_kernel, dim3((unsigned) ((n + 1023) / 1024)), dim3(256), 0, st, keys, n, n_dev, rbits, pbits, P,
                           seq_idx, pos, strand, motif_first, region_counts);
        MS_HIP(hipGetLastError());
        return MS_OK;
    }
    hipLaunchKernelGGL(finalize_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, st, keys, n, n_dev, gbits, P, S,
                       seq_idx, pos, strand, motif_first, region_counts);
    MS_HIP(hipGetLastError());
    return MS_OK;
}

}  // namespace ms
