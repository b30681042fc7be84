// ms_shuffle.hip -- ms_seqset_shuffle: a shuffled copy of a sequence set, made on the device (the control "the input itself, shuffled" of
// AME / HOMER / the TRAP null): MS_SHUFFLE_MONO keeps the base composition of every run of ACGT, MS_SHUFFLE_DINUC every dinucleotide count
// and both end bases of every run.  Non-ACGT positions stay where they are, so the count of valid windows of any width is unchanged.
//
// The RESULT IS A FUNCTION of (bases, kind, seed, sequence index) -- include/motifscan_amd.h states it, motifscan_amd/shuffle.py restates
// it sequentially, and the kernels below must give the restatement's bytes whatever the mapping.  In short, with
//     mix(x): x ^= x >> 30; x *= 0xbf58476d1ce4e5b9; x ^= x >> 27; x *= 0x94d049bb133111eb; x ^= x >> 31
//     h(seed, r, x, y) = mix(mix(mix(mix(seed + 0x9e3779b97f4a7c15) + r) + x) + y)
// a run that starts b bases into sequence r is, for mono, its bases ordered by (h(seed, r, b, p), p); for dinuc, Altschul-Erickson: an
// arborescence towards the run's last base f is drawn by Wilson's loop-erased walk on the 4 x 4 count matrix (draw d of the run is
// (h(seed, r, b, 2^62 | d) * tot) >> 64), the LAST edge p that realises next[u] is reserved as u's last exit, every other exit list is
// ordered by (h(seed, r, b, p), p), and the Euler walk from the run's first base reads the lists off.  Wilson, not rejection: rejection needs
// ~n tries on poly-A and microsatellite runs, the walk a few hundred draws at most.  The walk has NO cap (a cap would change the
// distribution).  The draw (h * tot) >> 64 is biased by less than tot / 2^64; that is part of the specification and must not be "fixed".
//
// The mapping.
//   1. sh_count_kernel, one thread per 32-base unit (blocks of kShBlockBases): the output's mask plane is the input's, its code words are
//      zeroed, and the runs' first and last bases are counted per block -- a run starts at an ACGT base that follows a non-ACGT base or
//      begins a sequence (sh_mark_kernel sets one bit per sequence start first).  One scan over the blocks; the host reads the run count.
//   2. sh_list_kernel: the k-th start and the k-th end of the set belong to the same run, so the two ranks give (start, end, sequence) of
//      every run with no search.  sh_long_kernel collects the runs of more than kShTile bases and sizes their scratch.
//   3. sh_tile_kernel: ONE WAVE PER RUN of up to kShTile bases, everything in LDS: the keys, a bitonic sort of (key, p), and for dinuc the
//      16 counts, the arborescence (lane 0), the reserved edges, the placement of the successors into four lists (ballot ranks over the
//      sorted order) and the Euler walk (lane 0: a dependent chain of LDS reads, eight successors per read, the four cursors in LDS).  The serial parts leave 63
//      lanes idle; the CU hides that with a dozen such waves side by side (12.4 KB of LDS each).
//      sh_long_kernel's runs take sh_global_kernel: the same code, one 256-thread block per run, keys and lists in pooled global scratch.
//   4. The shared-word rule: sequences are concatenated unaligned, so a 16-base code word can hold bases of several runs, sequences or
//      blocks.  A run stores the words it covers whole and ORs (vector atomicOr) its bits into the at most two words it shares; step 1 zeroed
//      them, non-ACGT bases keep code 0, and nothing is ever set past the last base -- the planes pass ms_genome_create_packed's validation.
#include <algorithm>
#include <memory>

#include "ms_device.h"
#include "ms_handles.h"

namespace ms {

namespace {

constexpr int kShUnitThreads = 256;                         // the unit-wise kernels: one thread per 32 bases
constexpr int kShBlockBases = kShUnitThreads * 32;
constexpr int kShTile = 1024;                               // the longest run one wave shuffles in LDS
constexpr int kShTileThreads = 64;
constexpr int kShLongThreads = 256;                         // sh_global_kernel: one block per longer run
constexpr unsigned kShMaxGrid = 1u << 22;                   // blocks of a run kernel (they stride over the runs)
constexpr uint64_t kShGolden = 0x9e3779b97f4a7c15ULL, kShDraw = 1ULL << 62;

struct ShTimes { double ms[4] = {0, 0, 0, 0}; bool set = false; };
std::mutex g_times_mu;
std::map<int, ShTimes> g_times;                             // the last call's stage times, per device (ms_debug_shuffle_stage_ms)

__host__ __device__ __forceinline__ uint64_t sh_mix(uint64_t x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27; x *= 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}

// ------------------------------------------------------------------ run discovery --

__global__ void __launch_bounds__(kShUnitThreads) sh_mark_kernel(const int64_t *__restrict__ offsets, int64_t R, uint32_t *__restrict__ seq_start) {
    const int64_t r = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int64_t o = offsets[r];
    if (offsets[r + 1] > o) atomicOr(&seq_start[o >> 5], 1u << (o & 31));
}

// the first and last bases of the runs in unit u: bit i = base 32 u + i
__device__ __forceinline__ void sh_unit_edges(const uint32_t *__restrict__ nmask, const uint32_t *__restrict__ seq_start, int64_t u, int64_t n_bases,
                                              uint32_t &first, uint32_t &last) {
    const int64_t left = n_bases - 32 * u;                  // > 0
    const uint32_t valid = left >= 32 ? 0xFFFFFFFFu : low_mask((int) left);
    const uint32_t nw = nmask[u], sw = seq_start[u];
    const uint32_t acgt = ~nw & valid;
    const uint32_t prev_n = u > 0 ? nmask[u - 1] >> 31 : 1u;
    first = acgt & (sw | (nw << 1) | prev_n);
    // the base behind bit i: a sequence start, a non-ACGT base, or past the end of the set (nmask and seq_start have readable zero words behind them)
    const uint32_t next_valid = left > 32 ? 1u : 0u;
    const uint32_t nxt = ((nw | sw) >> 1) | (((nmask[u + 1] | seq_start[u + 1]) & 1u) << 31);
    const uint32_t nxt_in = (valid >> 1) | (next_valid << 31);
    last = acgt & (nxt | ~nxt_in);
}

// exclusive prefix of a packed pair of counts (low and high 16 bits, block totals <= 8192 each) over the block's threads; total: the block's sum
__device__ __forceinline__ uint32_t sh_block_prefix(uint32_t v, uint32_t *lds, uint32_t &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kShUnitThreads / 64; w++) {
        const uint32_t t = lds[w];
        if (w < wave) base += t;
        total += t;
    }
    return base + inc - v;
}

__global__ void __launch_bounds__(kShUnitThreads) sh_count_kernel(const uint32_t *__restrict__ nmask, const uint32_t *__restrict__ seq_start, int64_t n_bases,
                                                                   int64_t n_units, uint32_t *__restrict__ out_codes, uint32_t *__restrict__ out_nmask,
                                                                   int64_t *__restrict__ blk_first, int64_t *__restrict__ blk_last) {
    __shared__ uint32_t lds[kShUnitThreads / 64];
    const int64_t u = (int64_t) blockIdx.x * kShUnitThreads + threadIdx.x;
    uint32_t v = 0;
    if (u < n_units) {
        uint32_t first, last;
        sh_unit_edges(nmask, seq_start, u, n_bases, first, last);
        v = (uint32_t) __popc(first) | ((uint32_t) __popc(last) << 16);
        out_nmask[u] = nmask[u];
        *reinterpret_cast<uint2 *>(out_codes + 2 * u) = make_uint2(0u, 0u);
    }
    uint32_t total;
    (void) sh_block_prefix(v, lds, total);
    if (threadIdx.x == 0) {
        blk_first[blockIdx.x] = total & 0xFFFFu;
        blk_last[blockIdx.x] = total >> 16;
    }
}

__global__ void __launch_bounds__(kShUnitThreads) sh_list_kernel(DevSeq S, const uint32_t *__restrict__ seq_start, int64_t n_units,
                                                                  const int64_t *__restrict__ blk_first, const int64_t *__restrict__ blk_last,
                                                                  int64_t *__restrict__ run_start, int64_t *__restrict__ run_end, int64_t *__restrict__ run_seq) {
    __shared__ uint32_t lds[kShUnitThreads / 64];
    const int64_t u = (int64_t) blockIdx.x * kShUnitThreads + threadIdx.x;
    uint32_t first = 0, last = 0;
    if (u < n_units) sh_unit_edges(S.nmask, seq_start, u, S.n_bases, first, last);
    uint32_t total;
    const uint32_t pre = sh_block_prefix((uint32_t) __popc(first) | ((uint32_t) __popc(last) << 16), lds, total);
    int64_t kf = blk_first[blockIdx.x] + (pre & 0xFFFFu), kl = blk_last[blockIdx.x] + (pre >> 16);
    if (first) {
        int64_t r = find_region(S, 32 * u + (__ffs(first) - 1));
        while (first) {
            const int64_t g = 32 * u + (__ffs(first) - 1);
            first &= first - 1;
            while (S.offsets[r + 1] <= g) r++;
            run_start[kf] = g;
            run_seq[kf] = r;
            kf++;
        }
    }
    while (last) {
        run_end[kl++] = 32 * u + __ffs(last);               // one past the run's last base
        last &= last - 1;
    }
}

// the runs the tile kernel leaves out, each with its place in the global scratch (order: as the atomics fall; the result does not depend on it)
__host__ __device__ __forceinline__ uint64_t sh_scratch_bytes(int64_t n) {
    uint64_t npad = 1;
    while ((int64_t) npad < n) npad <<= 1;
    const uint64_t nb = ((uint64_t) n + 7) & ~7ULL;
    return 16 * npad + 2 * nb + 64;                          // keys, indices | bases | exit lists (four, each 8-byte aligned)
}

__global__ void __launch_bounds__(kShUnitThreads) sh_long_kernel(const int64_t *__restrict__ run_start, const int64_t *__restrict__ run_end, int64_t n_runs,
                                                                  int64_t *__restrict__ long_run, unsigned long long *__restrict__ long_off,
                                                                  unsigned long long *__restrict__ counters) {
    const int64_t k = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_runs) return;
    const int64_t n = run_end[k] - run_start[k];
    if (n <= kShTile) return;
    const unsigned long long i = atomicAdd(&counters[0], 1ULL);
    long_run[i] = k;
    long_off[i] = atomicAdd(&counters[1], (unsigned long long) sh_scratch_bytes(n));
}

// ------------------------------------------------------------------- one run --

struct ShState {                                            // a block's small shared state
    unsigned long long cnt[16];                             // m[u][w]
    unsigned long long res[4];                              // 1 + the reserved edge of u, 0: none
    unsigned long long lstart[4];                           // where u's exit list starts in L (bytes, a multiple of 8)
    unsigned long long rowtot[4];
    unsigned long long word[4];                             // the Euler walk's cursors: the eight successors of u's list being read ...
    unsigned long long used[4];                             // ... and how many of the list are used
    int next[4];
};

// The run of n >= 1 bases at g0 (b bases into its sequence, pre = the hash of (seed, sequence, b)) by the T threads of a block.  hk / ix: npad
// keys and indices (npad = n rounded up to a power of two); s: the run's bases, n + 1 bytes; L: the four exit lists, n + 32 bytes, 8-byte aligned.
// The output bases are written over hk (it is dead once the sort's order has been read).
template <int T, typename IxT, typename N>
__device__ __forceinline__ void sh_shuffle_run(const uint32_t *__restrict__ codes_in, uint32_t *__restrict__ codes_out, int64_t g0, N n, uint64_t pre, uint64_t b,
                                               int kind, uint64_t *hk, IxT *ix, uint8_t *s, uint64_t *L, ShState &sm) {
    const int tid = threadIdx.x;
    uint8_t *out = reinterpret_cast<uint8_t *>(hk);
    uint8_t *Lb = reinterpret_cast<uint8_t *>(L);
    for (N i = tid; i < n; i += T) {
        const int64_t g = g0 + i;
        s[i] = (uint8_t) ((codes_in[g >> 4] >> (2 * ((uint32_t) g & 15u))) & 3u);
    }
    const bool copy = kind == MS_SHUFFLE_DINUC && n < 3;
    const N m = kind == MS_SHUFFLE_MONO ? n : n - 1;        // keys: one per base, or one per edge (p, p + 1)
    if (!copy) {
        N npad = 1;
        while (npad < m) npad <<= 1;
        if (tid < 16) sm.cnt[tid] = 0;
        if (tid < 4) { sm.res[tid] = 0; sm.next[tid] = -1; }
        for (N i = tid; i < npad; i += T) {
            hk[i] = i < m ? sh_mix(pre + b + (uint64_t) i) : ~0ULL;
            ix[i] = i < m ? (IxT) i : (IxT) ~(IxT) 0;
        }
        __syncthreads();
        // ---- (key, p) ascending: bitonic over npad slots, the padding (all ones, p = all ones) sorts last
        for (N k = 2; k <= npad; k <<= 1) {
            for (N j = k >> 1; j > 0; j >>= 1) {
                for (N t = tid; t < (npad >> 1); t += T) {
                    const N i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                    const uint64_t a = hk[i], c = hk[l];
                    const IxT ia = ix[i], ic = ix[l];
                    const bool gt = a > c || (a == c && ia > ic);
                    if (gt == ((i & k) == 0)) { hk[i] = c; hk[l] = a; ix[i] = ic; ix[l] = ia; }
                }
                __syncthreads();
            }
        }
    } else {
        __syncthreads();
    }
    if (copy) {
        for (N i = tid; i < n; i += T) out[i] = s[i];
    } else if (kind == MS_SHUFFLE_MONO) {
        for (N i = tid; i < n; i += T) out[i] = s[ix[i]];
    } else {
        // ---- 1. the 16 counts
        {
            unsigned long long c[16];
#pragma unroll
            for (int q = 0; q < 16; q++) c[q] = 0;
            for (N i = tid; i < m; i += T) {
                const int pair = s[i] * 4 + s[i + 1];
#pragma unroll
                for (int q = 0; q < 16; q++) c[q] += pair == q ? 1u : 0u;
            }
#pragma unroll
            for (int q = 0; q < 16; q++) if (c[q]) atomicAdd(&sm.cnt[q], c[q]);
        }
        __syncthreads();
        const int f = s[n - 1];
        // ---- 2. the arborescence towards f: Wilson's loop-erased walk, one lane
        if (tid == 0) {
            unsigned in_tree = 1u << f;
            uint64_t d = 0;
            unsigned long long at = 0;
            for (int v = 0; v < 4; v++) {
                const unsigned long long tot_v = sm.cnt[4 * v] + sm.cnt[4 * v + 1] + sm.cnt[4 * v + 2] + sm.cnt[4 * v + 3];
                sm.rowtot[v] = tot_v;
                sm.lstart[v] = at;
                at += (tot_v + 7) & ~7ULL;
                if ((in_tree >> v & 1u) || tot_v == 0) continue;
                int u = v;
                while (!(in_tree >> u & 1u)) {
                    const unsigned long long tot = sm.cnt[4 * u] + sm.cnt[4 * u + 1] + sm.cnt[4 * u + 2] + sm.cnt[4 * u + 3] - sm.cnt[5 * u];
                    if (tot == 0) { sm.next[u] = f; break; }                   // (cannot be: a base other than f that the run reaches has an exit to another base)
                    const unsigned long long x = __umul64hi(sh_mix(pre + (kShDraw | d)), tot);
                    d++;
                    unsigned long long acc = 0;
                    int w = 0;
                    for (int q = 0; q < 4; q++) {
                        if (q == u) continue;
                        acc += sm.cnt[4 * u + q];
                        w = q;
                        if (acc > x) break;
                    }
                    sm.next[u] = w;
                    u = w;
                }
                u = v;
                while (!(in_tree >> u & 1u)) { in_tree |= 1u << u; u = sm.next[u]; }
            }
        }
        __syncthreads();
        // ---- 3. the reserved edge of u: the last p with s[p] = u, s[p + 1] = next[u]
        {
            unsigned long long best[4] = {0, 0, 0, 0};
            const int n0 = sm.next[0], n1 = sm.next[1], n2 = sm.next[2], n3 = sm.next[3];
            for (N i = tid; i < m; i += T) {
                const int u = s[i], w = s[i + 1];
                const int nu = u == 0 ? n0 : u == 1 ? n1 : u == 2 ? n2 : n3;
                if (u != f && w == nu) {
#pragma unroll
                    for (int q = 0; q < 4; q++) if (u == q) best[q] = (unsigned long long) i + 1;      // (i ascends per thread)
                }
            }
#pragma unroll
            for (int q = 0; q < 4; q++) if (best[q]) atomicMax(&sm.res[q], best[q]);
        }
        __syncthreads();
        // ---- 4. the successors into the four exit lists, in sorted order, the reserved one last: wave 0, ranks from ballots
        if (tid < 64) {
            const unsigned long long lt = (1ULL << tid) - 1ULL;
            unsigned long long fill[4] = {0, 0, 0, 0};
            for (N j0 = 0; j0 < m; j0 += 64) {
                const N j = j0 + tid;
                const bool valid = j < m;
                const N e = valid ? (N) ix[j] : 0;
                const int u = valid ? s[e] : 0, w = valid ? s[e + 1] : 0;
                const bool is_res = valid && sm.res[u] == (unsigned long long) e + 1;
                unsigned long long pos = 0;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const unsigned long long mask = __ballot(valid && !is_res && u == q);
                    if (u == q) pos = fill[q] + (unsigned long long) __popcll(mask & lt);
                    fill[q] += (unsigned long long) __popcll(mask);
                }
                if (valid) Lb[sm.lstart[u] + (is_res ? sm.rowtot[u] - 1 : pos)] = (uint8_t) w;
            }
        }
        __syncthreads();
        // ---- 5. the Euler walk, one lane: eight successors per read of a list.  The four cursors live in LDS, indexed by the current base:
        // in registers they cost a chain of selects per step, and a wave that walks is bound by the instructions it issues for one lane.
        if (tid == 0) {
            for (int u = 0; u < 4; u++) { sm.word[u] = 0; sm.used[u] = 0; }
            int cur = s[0];
            out[0] = (uint8_t) cur;
            for (N k = 1; k < n; k++) {
                const unsigned long long pc = sm.used[cur];
                unsigned long long wc = sm.word[cur];
                if ((pc & 7) == 0) {
                    if (pc >= sm.rowtot[cur]) break;                          // (cannot be: the walk ends on f with every list read to its end)
                    wc = L[(sm.lstart[cur] + pc) >> 3];
                    sm.word[cur] = wc;
                }
                sm.used[cur] = pc + 1;
                cur = (int) (wc >> (8 * (int) (pc & 7))) & 3;
                out[k] = (uint8_t) cur;
            }
        }
    }
    __syncthreads();
    // ---- the code words: the words inside the run whole, the shared ones at its ends by atomicOr (they were zeroed, see the file header)
    const int64_t wf = g0 >> 4, wl = (g0 + (int64_t) n - 1) >> 4;
    for (int64_t w = wf + tid; w <= wl; w += T) {
        const int64_t lo = g0 > 16 * w ? g0 : 16 * w, hi = g0 + (int64_t) n < 16 * w + 16 ? g0 + (int64_t) n : 16 * w + 16;
        uint32_t v = 0;
        for (int64_t g = lo; g < hi; g++) v |= (uint32_t) out[g - g0] << (2 * ((uint32_t) g & 15u));
        if (hi - lo == 16) codes_out[w] = v;
        else if (v) atomicOr(&codes_out[w], v);
    }
    __syncthreads();
}

struct ShArgs {
    const uint32_t *codes_in;
    uint32_t *codes_out;
    const int64_t *offsets;
    const int64_t *run_start, *run_end, *run_seq;
    int64_t n_runs;
    uint64_t seed0;                                         // mix(seed + golden)
    int64_t seq_index_base;
    int kind;
};

__device__ __forceinline__ uint64_t sh_prefix(const ShArgs &A, int64_t k, int64_t g0, uint64_t &b) {
    const int64_t r = A.run_seq[k];
    b = (uint64_t) (g0 - A.offsets[r]);
    return sh_mix(sh_mix(A.seed0 + (uint64_t) (A.seq_index_base + r)) + b);
}

__global__ void __launch_bounds__(kShTileThreads) sh_tile_kernel(ShArgs A) {
    __shared__ uint64_t hk[kShTile];
    __shared__ uint64_t L[(kShTile + 32) / 8];
    __shared__ uint16_t ix[kShTile];
    __shared__ uint8_t s[kShTile + 8];
    __shared__ ShState sm;
    for (int64_t k = blockIdx.x; k < A.n_runs; k += gridDim.x) {
        const int64_t g0 = A.run_start[k], n = A.run_end[k] - g0;
        if (n > kShTile) continue;
        uint64_t b;
        const uint64_t pre = sh_prefix(A, k, g0, b);
        sh_shuffle_run<kShTileThreads, uint16_t, int>(A.codes_in, A.codes_out, g0, (int) n, pre, b, A.kind, hk, ix, s, L, sm);
    }
}

__global__ void __launch_bounds__(kShLongThreads) sh_global_kernel(ShArgs A, const int64_t *__restrict__ long_run, const unsigned long long *__restrict__ long_off,
                                                                    int64_t n_long, uint8_t *__restrict__ scratch) {
    __shared__ ShState sm;
    for (int64_t q = blockIdx.x; q < n_long; q += gridDim.x) {
        const int64_t k = long_run[q];
        const int64_t g0 = A.run_start[k], n = A.run_end[k] - g0;
        uint64_t npad = 1;
        while ((int64_t) npad < n) npad <<= 1;
        uint8_t *p = scratch + long_off[q];
        uint64_t *hk = reinterpret_cast<uint64_t *>(p);
        uint64_t *ix = hk + npad;
        uint8_t *s = p + 16 * npad;
        uint64_t *L = reinterpret_cast<uint64_t *>(s + (((uint64_t) n + 7) & ~7ULL));
        uint64_t b;
        const uint64_t pre = sh_prefix(A, k, g0, b);
        sh_shuffle_run<kShLongThreads, uint64_t, int64_t>(A.codes_in, A.codes_out, g0, n, pre, b, A.kind, hk, ix, s, L, sm);
    }
}


}  // namespace

}  // namespace ms

using namespace ms;

extern "C" {

int ms_debug_shuffle_dims(int32_t out[4]) {
    if (!out) { set_error("NULL output"); return MS_ERR_INVALID; }
    out[0] = kShTile;                                        // (no lane tier: the shortest runs take a wave as well)
    out[1] = kShTile;
    out[2] = kShBlockBases;
    out[3] = 0;
    return MS_OK;
}

int ms_debug_shuffle_stage_ms(double out[4]) {
    if (!out) { set_error("NULL output"); return MS_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(g_times_mu);
    const auto it = g_times.find(current_device());
    if (it == g_times.end() || !it->second.set) { set_error("no ms_seqset_shuffle call has run on this device"); return MS_ERR_INVALID; }
    for (int i = 0; i < 4; i++) out[i] = it->second.ms[i];
    return MS_OK;
}

int ms_seqset_shuffle(const ms_seqset *seqs, int kind, uint64_t seed, int64_t seq_index_base, uint32_t flags, ms_seqset **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    if (!require_device()) return MS_ERR_RUNTIME;
    if (!seqs) { set_error("NULL handle"); return MS_ERR_INVALID; }
    if (kind != MS_SHUFFLE_MONO && kind != MS_SHUFFLE_DINUC) { set_error("invalid shuffle kind %d (1 mono, 2 dinuc)", kind); return MS_ERR_INVALID; }
    if (flags != 0u) { set_error("unknown shuffle flags 0x%x", flags); return MS_ERR_INVALID; }
    if (seq_index_base < 0) { set_error("seq_index_base must be >= 0"); return MS_ERR_INVALID; }
    if (!seqs->built || seqs->pack_pending || !seqs->block) { set_error("the set's planes are not on the device yet (packed by its first scan)"); return MS_ERR_INVALID; }
    DeviceCtx *c;
    int rc = get_ctx(seqs->device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk_dev(c->mu);
    MS_HIP(hipSetDevice(c->device));
    const hipStream_t st = c->stream;
    const int64_t R = seqs->R, n_bases = seqs->n_bases, n_units = (n_bases + 31) / 32;
    const int64_t n_blk = (n_units + kShUnitThreads - 1) / kShUnitThreads;

    ms_seqset *S = nullptr;
    if ((rc = seqset_create_unpacked(seqs->offsets.data(), R, c->device, &S))) return rc;
    void *wblk = nullptr, *rblk = nullptr, *sblk = nullptr;
    size_t wgot = 0, rgot = 0, sgot = 0;
    auto fail = [&](int code) {
        (void) hipStreamSynchronize(st);                     // (nothing queued may still use the blocks)
        if (wblk) pool_free(c, wblk, wgot);
        if (rblk) pool_free(c, rblk, rgot);
        if (sblk) pool_free(c, sblk, sgot);
        ms_seqset_free(S);
        return code;
    };
    auto hip_fail = [&](hipError_t e, const char *what) { set_error("%s failed: %s", what, hipGetErrorString(e)); return fail(e == hipErrorOutOfMemory ? MS_ERR_NOMEM : MS_ERR_RUNTIME); };
    hipError_t he = hipEventRecord(c->ev[0], st);
    if (he != hipSuccess) return hip_fail(he, "event");
    int64_t n_runs = 0;
    unsigned long long h_cnt[2] = {0, 0};

    if (n_units > 0) {
        // ---- 1. the mask plane, zeroed code words, the runs' ends counted per block
        size_t t_scan = 0;
        if ((rc = exclusive_sum_i64(nullptr, &t_scan, nullptr, nullptr, (size_t) n_blk + 1, st))) return fail(rc);
        const size_t b_ss = up256(4 * ((size_t) n_units + 2)), b_blk = up256(8 * ((size_t) n_blk + 1)), b_tmp = up256(std::max<size_t>(t_scan, 1));
        if ((rc = pool_alloc(c, b_ss + 4 * b_blk + b_tmp + 256, &wblk, &wgot))) return fail(rc);
        char *p = static_cast<char *>(wblk);
        uint32_t *d_ss = reinterpret_cast<uint32_t *>(p); p += b_ss;
        int64_t *d_cf = reinterpret_cast<int64_t *>(p); p += b_blk;
        int64_t *d_cl = reinterpret_cast<int64_t *>(p); p += b_blk;
        int64_t *d_bf = reinterpret_cast<int64_t *>(p); p += b_blk;
        int64_t *d_bl = reinterpret_cast<int64_t *>(p); p += b_blk;
        void *d_tmp = p; p += b_tmp;
        unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(p);
        he = hipMemsetAsync(d_ss, 0, 4 * ((size_t) n_units + 2), st);
        if (he == hipSuccess) he = hipMemsetAsync(d_cf + n_blk, 0, 8, st);
        if (he == hipSuccess) he = hipMemsetAsync(d_cl + n_blk, 0, 8, st);
        if (he == hipSuccess) he = hipMemsetAsync(d_cnt, 0, 16, st);
        if (he != hipSuccess) return hip_fail(he, "clearing the work block");
        hipLaunchKernelGGL(sh_mark_kernel, dim3((unsigned) ((R + kShUnitThreads - 1) / kShUnitThreads)), dim3(kShUnitThreads), 0, st, seqs->d_offsets, R, d_ss);
        if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "sequence marks");
        hipLaunchKernelGGL(sh_count_kernel, dim3((unsigned) n_blk), dim3(kShUnitThreads), 0, st, seqs->d_nmask, (const uint32_t *) d_ss, n_bases, n_units, S->d_codes,
                           S->d_nmask, d_cf, d_cl);
        if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "run count");
        size_t tb = t_scan;
        if ((rc = exclusive_sum_i64(d_tmp, &tb, d_cf, d_bf, (size_t) n_blk + 1, st))) return fail(rc);
        tb = t_scan;
        if ((rc = exclusive_sum_i64(d_tmp, &tb, d_cl, d_bl, (size_t) n_blk + 1, st))) return fail(rc);
        he = hipMemcpyAsync(&n_runs, d_bf + n_blk, 8, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipEventRecord(c->ev[1], st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        if (he != hipSuccess) return hip_fail(he, "run count");

        // ---- 2. the run list, and the runs beyond the LDS tile
        const size_t nz = (size_t) std::max<int64_t>(n_runs, 0) + 8, n_long_max = (size_t) (n_bases / (kShTile + 1)) + 1;
        if ((rc = pool_alloc(c, 3 * up256(8 * nz) + 2 * up256(8 * n_long_max), &rblk, &rgot))) return fail(rc);
        p = static_cast<char *>(rblk);
        int64_t *d_rs = reinterpret_cast<int64_t *>(p); p += up256(8 * nz);
        int64_t *d_re = reinterpret_cast<int64_t *>(p); p += up256(8 * nz);
        int64_t *d_rq = reinterpret_cast<int64_t *>(p); p += up256(8 * nz);
        int64_t *d_lr = reinterpret_cast<int64_t *>(p); p += up256(8 * n_long_max);
        unsigned long long *d_lo = reinterpret_cast<unsigned long long *>(p);
        if (n_runs > 0) {
            hipLaunchKernelGGL(sh_list_kernel, dim3((unsigned) n_blk), dim3(kShUnitThreads), 0, st, dev_seq(seqs), (const uint32_t *) d_ss, n_units, (const int64_t *) d_bf,
                               (const int64_t *) d_bl, d_rs, d_re, d_rq);
            if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "run list");
            hipLaunchKernelGGL(sh_long_kernel, dim3((unsigned) ((n_runs + kShUnitThreads - 1) / kShUnitThreads)), dim3(kShUnitThreads), 0, st, (const int64_t *) d_rs,
                               (const int64_t *) d_re, n_runs, d_lr, d_lo, d_cnt);
            if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "long runs");
        }
        he = hipMemcpyAsync(h_cnt, d_cnt, 16, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipEventRecord(c->ev[2], st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        if (he != hipSuccess) return hip_fail(he, "run list");

        // ---- 3. the runs
        ShArgs A;
        A.codes_in = seqs->d_codes; A.codes_out = S->d_codes; A.offsets = seqs->d_offsets;
        A.run_start = d_rs; A.run_end = d_re; A.run_seq = d_rq; A.n_runs = n_runs;
        A.seed0 = sh_mix(seed + kShGolden);
        A.seq_index_base = seq_index_base;
        A.kind = kind;
        const int64_t n_long = (int64_t) h_cnt[0];
        if (n_long > 0) {
            if ((rc = pool_alloc(c, (size_t) h_cnt[1] + 256, &sblk, &sgot))) return fail(rc);
            hipLaunchKernelGGL(sh_global_kernel, dim3((unsigned) std::min<int64_t>(n_long, kShMaxGrid)), dim3(kShLongThreads), 0, st, A, (const int64_t *) d_lr,
                               (const unsigned long long *) d_lo, n_long, static_cast<uint8_t *>(sblk));
            if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "long-run shuffle");
        }
        if (n_runs > n_long) {
            hipLaunchKernelGGL(sh_tile_kernel, dim3((unsigned) std::min<int64_t>(n_runs, kShMaxGrid)), dim3(kShTileThreads), 0, st, A);
            if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "shuffle");
        }
    } else {
        he = hipEventRecord(c->ev[1], st);
        if (he == hipSuccess) he = hipEventRecord(c->ev[2], st);
        if (he != hipSuccess) return hip_fail(he, "event");
    }
    he = hipEventRecord(c->ev[3], st);
    if (he != hipSuccess) return hip_fail(he, "event");
    if ((rc = seqset_launch_hints(S, st))) return fail(rc);
    he = hipEventRecord(c->ev[4], st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) return hip_fail(he, "shuffle");
    {
        ShTimes t;
        float f = 0;
        for (int i = 0; i < 4; i++) { (void) hipEventElapsedTime(&f, c->ev[i], c->ev[i + 1]); t.ms[i] = f; }
        t.set = true;
        std::lock_guard<std::mutex> lk(g_times_mu);
        g_times[c->device] = t;
    }
    if (wblk) pool_free(c, wblk, wgot);
    if (rblk) pool_free(c, rblk, rgot);
    if (sblk) pool_free(c, sblk, sgot);
    *out = S;
    return MS_OK;
}

}  // extern "C"
