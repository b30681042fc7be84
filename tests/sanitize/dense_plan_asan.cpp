// tests/sanitize/dense_plan_asan.cpp -- the host's plan of the dense walks (motifscan_amd/csrc/ms_dense_plan.h: segments of the regions,
// tiles of the motifs, the layout of the plan in a work block) under AddressSanitizer + UndefinedBehaviorSanitizer, compiled by plain g++
// from the header the library is built from.  Every case is compared, field for field, with a brute-force restatement that takes one
// region and one motif at a time and keeps no running state; then the plan is copied into arrays of exactly the promised sizes and
// walked as the kernels walk it, so a step past an array stops the run.  CPU build container only (`make -C motifscan_amd/csrc sanitize`).
#include "ms_dense_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static int n_cases = 0;

struct Input {
    ms::DenseGeom g;
    std::vector<int64_t> off;                            // [R + 1]
    std::vector<int32_t> widths;                         // [P]
    std::vector<uint8_t> walked;                         // [P]
    int64_t R() const { return (int64_t) off.size() - 1; }
    int32_t P() const { return (int32_t) widths.size(); }
    int64_t len(int64_t r) const { return off[(size_t) r + 1] - off[(size_t) r]; }
};

// ---- the restatement: every quantity from the input alone, summed from scratch wherever it is asked for
static int64_t segs_of(const Input &in, int64_t r) {
    const int64_t n = (in.len(r) + in.g.seg_windows - 1) / in.g.seg_windows;
    return n < 1 ? 1 : n;                                // an empty region still has one segment
}
static bool any_long(const Input &in) {
    for (int64_t r = 0; r < in.R(); r++)
        if (in.len(r) > in.g.seg_windows) return true;
    return false;
}
static int64_t segs_before(const Input &in, int64_t r) {
    int64_t n = 0;
    for (int64_t q = 0; q < r; q++) n += segs_of(in, q);
    return n;
}
static int64_t parts_before(const Input &in, int64_t r) {
    int64_t n = 0;
    for (int64_t q = 0; q < r; q++) n += segs_of(in, q) > 1 ? segs_of(in, q) : 0;
    return n;
}
static bool in_lds(const Input &in, int32_t m) { return m >= 0 && m < in.P() && in.walked[(size_t) m] && in.widths[(size_t) m] <= in.g.tile_max_w; }
static bool is_wide(const Input &in, int32_t m) { return in.walked[(size_t) m] && in.widths[(size_t) m] > in.g.tile_max_w; }
static size_t entries(const Input &in, int32_t a, int32_t b) {      // of the motifs a .. b
    size_t e = 0;
    for (int32_t m = a; m <= b; m++) e += (size_t) in.widths[(size_t) m] * 4;
    return e;
}
// the first motif of the LDS tile that holds motif m: from the start of m's run of consecutive LDS motifs, tiles are filled greedily
static int32_t tile_start(const Input &in, int32_t m) {
    int32_t a = m;
    while (in_lds(in, a - 1)) a--;
    for (int32_t s = a;;) {
        int32_t j = s;
        while (in_lds(in, j + 1) && entries(in, s, j + 1) <= (size_t) in.g.tile_entries) j++;
        if (m <= j) return s;
        s = j + 1;
    }
}
static int32_t tile_end(const Input &in, int32_t s) {               // the last motif of the tile that starts at s
    int32_t j = s;
    while (in_lds(in, j + 1) && tile_start(in, j + 1) == s) j++;
    return j;
}

static ms::DensePlan expected(const Input &in) {
    ms::DensePlan e;
    const int64_t R = in.R();
    const bool cut = any_long(in);
    e.n_seg = cut ? segs_before(in, R) : R;
    if (cut) {
        for (int64_t r = 0; r <= R; r++) e.seg_first.push_back(segs_before(in, r));
        if (in.g.partials) {
            for (int64_t r = 0; r <= R; r++) e.part_first.push_back(parts_before(in, r));
            for (int64_t r = 0; r < R; r++)
                if (segs_of(in, r) > 1) e.long_regions.push_back(r);
            e.n_part = parts_before(in, R);
        }
    }
    for (int32_t m = 0; m < in.P(); m++)
        if (!in.walked[(size_t) m]) e.skipped.push_back(m);
    for (int32_t m = 0; m < in.P(); m++)
        if (in_lds(in, m)) {
            if (tile_start(in, m) == m) {
                e.tile_first.push_back((int32_t) e.mot.size());
                e.max_tile = std::max(e.max_tile, entries(in, m, tile_end(in, m)));
            }
            e.mot.push_back(m);
        }
    e.tile_first.push_back((int32_t) e.mot.size());      // closes the last tile; alone, it says "no LDS tile"
    e.wide_first.push_back((int32_t) e.mot.size());
    for (int32_t m = 0; m < in.P(); m++)
        if (is_wide(in, m)) { e.mot.push_back(m); e.wide_first.push_back((int32_t) e.mot.size()); }
    return e;
}

// a copy of exactly v.size() elements on the heap: ASan sees a step past it
template <typename T>
static std::unique_ptr<T[]> exact(const std::vector<T> &v) {
    std::unique_ptr<T[]> p(new T[v.size()]);
    if (!v.empty()) std::memcpy(p.get(), v.data(), sizeof(T) * v.size());
    return p;
}

template <typename T>
static void place(void *base, size_t total, ms::Carve::Slot<T> s, const std::vector<T> &v, size_t &end) {
    CHECK(s.off % ms::Carve::kAlign == 0 && s.off >= end && s.off + sizeof(T) * v.size() <= total);
    if (!v.empty()) std::memcpy(ms::Carve::at(base, s), v.data(), sizeof(T) * v.size());
    end = s.off + sizeof(T) * v.size();
}

static void check_case(const Input &in) {
    n_cases++;
    ms::DensePlan pl;
    ms::dense_plan(in.g, in.widths.data(), in.P(), in.off.data(), in.R(), [&](int32_t m) { return in.walked[(size_t) m] != 0; }, &pl);
    const ms::DensePlan e = expected(in);
    CHECK(pl.seg_first == e.seg_first);
    CHECK(pl.part_first == e.part_first);
    CHECK(pl.long_regions == e.long_regions);
    CHECK(pl.mot == e.mot);
    CHECK(pl.tile_first == e.tile_first);
    CHECK(pl.wide_first == e.wide_first);
    CHECK(pl.skipped == e.skipped);
    CHECK(pl.n_seg == e.n_seg && pl.n_part == e.n_part && pl.max_tile == e.max_tile);

    // what the cases are about, said directly
    const int64_t R = in.R();
    const int seg = in.g.seg_windows;
    if (!any_long(in)) CHECK(pl.seg_first.empty() && pl.part_first.empty() && pl.long_regions.empty() && pl.n_seg == R && pl.n_part == 0);
    if (!in.g.partials) CHECK(pl.part_first.empty() && pl.long_regions.empty() && pl.n_part == 0);
    CHECK(pl.max_tile <= (size_t) in.g.tile_entries);
    CHECK(pl.mot.size() + pl.skipped.size() == (size_t) in.P());
    CHECK(!pl.tile_first.empty() && pl.tile_first[0] == 0 && !pl.wide_first.empty() && pl.wide_first[0] == pl.tile_first.back());
    CHECK(pl.wide_first.back() == (int32_t) pl.mot.size());

    // the walk of the kernels over arrays of exactly the promised sizes
    const auto seg_first = exact(pl.seg_first), part_first = exact(pl.part_first), long_regions = exact(pl.long_regions);
    const auto mot = exact(pl.mot), tile_first = exact(pl.tile_first), wide_first = exact(pl.wide_first);
    std::vector<uint8_t> part_seen((size_t) pl.n_part, 0);
    int64_t n_long = 0;
    for (int64_t s = 0; s < pl.n_seg; s++) {
        int64_t r = s, s_in = 0;
        bool whole = true;
        if (!pl.seg_first.empty()) {
            int64_t lo = 0, hi = R;                      // the region whose segments hold s (find_region_bsearch's contract)
            while (hi - lo > 1) { const int64_t mid = (lo + hi) / 2; if (seg_first[mid] <= s) lo = mid; else hi = mid; }
            r = lo;
            CHECK(seg_first[r] <= s && s < seg_first[r + 1]);
            s_in = s - seg_first[r];
            whole = seg_first[r + 1] - seg_first[r] == 1;
        }
        CHECK(r >= 0 && r < R);
        const int64_t L = in.len(r), p0 = s_in * seg;
        CHECK(p0 == 0 || p0 < L);                        // no segment starts past its region
        CHECK(p0 + seg >= L || !whole);                  // a region of one segment is covered by it
        if (L == seg) CHECK(whole);                      // exactly one segment: no partial
        if (L == seg + 1) CHECK(!whole && seg_first[r + 1] - seg_first[r] == 2);
        if (!whole && in.g.partials) {
            const int64_t at = part_first[r] + s_in;
            CHECK(at >= 0 && at < pl.n_part && !part_seen[(size_t) at]);
            part_seen[(size_t) at] = 1;
            CHECK(part_first[r + 1] - part_first[r] == seg_first[r + 1] - seg_first[r]);
        }
    }
    for (size_t i = 0; i < pl.long_regions.size(); i++) {
        const int64_t r = long_regions[i];
        CHECK(r >= 0 && r < R && seg_first[r + 1] - seg_first[r] > 1);
        n_long += seg_first[r + 1] - seg_first[r];
    }
    CHECK(n_long == pl.n_part);
    for (uint8_t seen : part_seen) CHECK(seen);
    std::vector<uint8_t> walked_once((size_t) in.P(), 0);
    const int32_t n_tiles = (int32_t) pl.tile_first.size() - 1, n_wide = (int32_t) pl.wide_first.size() - 1;
    for (int32_t t = 0; t < n_tiles; t++) {
        const int32_t k0 = tile_first[t], k1 = tile_first[t + 1];
        CHECK(k0 < k1);
        size_t e = 0;
        for (int32_t k = k0; k < k1; k++) {
            const int32_t m = mot[k];
            CHECK(in.walked[(size_t) m] && in.widths[(size_t) m] <= in.g.tile_max_w && !walked_once[(size_t) m]);
            if (k > k0) CHECK(m == mot[k - 1] + 1);     // consecutive in tab2: one contiguous copy stages the tile
            walked_once[(size_t) m] = 1;
            e += (size_t) in.widths[(size_t) m] * 4;
        }
        CHECK(e <= (size_t) in.g.tile_entries && e <= pl.max_tile);
    }
    for (int32_t t = 0; t < n_wide; t++) {
        CHECK(wide_first[t + 1] - wide_first[t] == 1);
        const int32_t m = mot[wide_first[t]];
        CHECK(in.walked[(size_t) m] && in.widths[(size_t) m] > in.g.tile_max_w && !walked_once[(size_t) m]);
        walked_once[(size_t) m] = 1;
    }
    for (int32_t m = 0; m < in.P(); m++) CHECK(walked_once[(size_t) m] == in.walked[(size_t) m]);
    // a skipped motif between two walked ones starts a new tile
    for (int32_t m = 1; m + 1 < in.P(); m++)
        if (!in.walked[(size_t) m] && in_lds(in, m - 1) && in_lds(in, m + 1)) CHECK(tile_start(in, m + 1) == m + 1);

    // the plan in a work block: every slot inside the block, in order, none over another; an own slot behind them
    ms::Carve cv;
    const ms::DenseSlots ds = ms::dense_slots(cv, pl);
    const auto s_own = cv.add<double>(3);
    const size_t total = cv.bytes();
    CHECK(total % ms::Carve::kAlign == 0 && total >= ms::Carve::kAlign);
    void *base = std::aligned_alloc(ms::Carve::kAlign, total);
    CHECK(base != nullptr);
    size_t end = 0;
    place(base, total, ds.seg_first, pl.seg_first, end);
    place(base, total, ds.part_first, pl.part_first, end);
    place(base, total, ds.long_regions, pl.long_regions, end);
    place(base, total, ds.mot, pl.mot, end);
    place(base, total, ds.tile_first, pl.tile_first, end);
    place(base, total, ds.wide_first, pl.wide_first, end);
    place(base, total, ds.skipped, pl.skipped, end);
    place(base, total, s_own, std::vector<double>(3, 1.0), end);
    CHECK(end <= total);
    std::free(base);
}

// every R in {0, 1, 3} with every combination of the lengths, for one set of motifs
static void over_regions(Input in) {
    const int seg = in.g.seg_windows;
    const int64_t lens[] = {0, 1, seg - 1, seg, seg + 1, 2 * seg, 2 * seg + 1};
    in.off = {0};
    check_case(in);                                      // R = 0
    for (int64_t a : lens) {
        in.off = {0, a};
        check_case(in);                                  // R = 1
    }
    for (int64_t a : lens)
        for (int64_t b : lens)
            for (int64_t c : lens) {
                in.off = {0, a, a + b, a + b + c};
                check_case(in);                          // R = 3
            }
}

static void over_motifs(const ms::DenseGeom &g) {
    const int32_t W = g.tile_max_w;
    Input in;
    in.g = g;
    over_regions(in);                                    // P = 0
    const int32_t one[] = {1, W, W + 1};                 // P = 1: a narrow motif, the widest tiled one, the narrowest wide one
    for (int32_t w : one)
        for (int walked = 0; walked < 2; walked++) {
            in.widths = {w};
            in.walked = {(uint8_t) walked};
            over_regions(in);
        }
    // P = 5.  The entries of a tile are 4 W: W one-column motifs fill it exactly.
    const std::vector<std::vector<int32_t>> five = {
        {1, 1, 1, 1, 1},                                 // (the tiny geometry: four fill a tile exactly, the fifth is one entry over)
        {W - 2, 1, 1, 1, 1},                             // exactly full after three, the fourth one over
        {W - 1, 1, 1, W, W},                             // full after two; a motif of W columns is a tile of its own
        {W, W + 1, 1, W + 1, 2},                         // W tiled, W + 1 wide: listed behind all LDS tiles; a wide motif breaks a run
        {W + 1, W + 1, W + 1, W + 1, W + 1},             // no LDS tile at all
        {2, 3, W, 1, W - 1},
    };
    const std::vector<std::vector<uint8_t>> walks = {{1, 1, 1, 1, 1}, {0, 0, 0, 0, 0}, {1, 1, 0, 1, 1}, {0, 1, 1, 1, 0}};
    for (const auto &w : five)
        for (const auto &k : walks) {
            in.widths = w;
            in.walked = k;
            over_regions(in);
        }
}

int main() {
    over_motifs({8, 4, 16, true});                       // tiny: every edge is a handful of elements
    over_motifs({8, 4, 16, false});
    // the sizes the three kernels are compiled with (ms_best_dev.h, ms_scorehist.hip; the GPU tests read them through ms_debug_*_dims)
    over_motifs({512, 1024, 4096, true});                // ms_scan_best and ms_scan_affinity: one walk, one geometry
    over_motifs({512, 928, 3712, false});                // ms_scan_score_histogram: no partials
    std::printf("dense_plan_asan: ok (%d cases)\n", n_cases);
    return 0;
}
