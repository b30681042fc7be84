// ms_dense_plan.h -- the host's plan of a dense walk (ms_scan_best, ms_scan_affinity, ms_scan_score_histogram, ms_affinity_expected_counts, ms_scan_best_dimodels: every window of every
// (motif, region) cell) and its layout in a work block: segments of the regions, tiles of the motifs.  Plain C++, no HIP include, so
// that it is checked on the CPU (tests/sanitize/dense_plan_asan.cpp), as ms_place.h is.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "ms_place.h"

namespace ms {

// The sizes of a walk: what its kernel is compiled with.
struct DenseGeom {
    int seg_windows;                                     // window starts per segment of a region
    int tile_max_w;                                      // widest motif whose table goes into an LDS tile
    int tile_entries;                                    // tab2 entries per tile (4 per column)
    bool partials;                                       // a region of more than one segment gets a partial per segment, folded by a reduce kernel
};

struct DensePlan {
    std::vector<int64_t> seg_first;                      // [R + 1] first segment of the region (every region has at least one); empty: one segment per region
    std::vector<int64_t> part_first;                     // [R + 1] first partial of the region (regions of one segment have none); empty with seg_first, and without partials
    std::vector<int64_t> long_regions;                   // the regions of more than one segment; empty without partials
    std::vector<int32_t> mot;                            // the motifs that are walked: the LDS tiles' one after the other, then the wide ones
    std::vector<int32_t> tile_first;                     // [LDS tiles + 1] into mot
    std::vector<int32_t> wide_first;                     // [wide motifs + 1] into mot: one "tile" per motif of more than tile_max_w columns
    std::vector<int32_t> skipped;                        // the motifs that are not walked: their rows are filled
    int64_t n_seg = 0, n_part = 0;
    size_t max_tile = 0;                                 // entries of the largest LDS tile
};

// widths[P], off[R + 1]; walked(m): motif m is scored.  LDS tiles first: runs of consecutive walked motifs of <= tile_max_w columns whose
// entries fit a tile (consecutive motifs are consecutive in tab2: one contiguous copy stages a tile; a skipped motif breaks the run);
// then one tile per wider motif.  May throw std::bad_alloc.
template <typename Walked>
inline void dense_plan(const DenseGeom &g, const int32_t *widths, int32_t P, const int64_t *off, int64_t R, Walked walked, DensePlan *pl) {
    pl->n_seg = R;
    pl->n_part = 0;
    bool any_long = false;
    for (int64_t r = 0; r < R && !any_long; r++) any_long = off[r + 1] - off[r] > g.seg_windows;
    if (any_long) {
        pl->seg_first.resize((size_t) R + 1);
        if (g.partials) pl->part_first.resize((size_t) R + 1);
        pl->n_seg = 0;
        for (int64_t r = 0; r < R; r++) {
            const int64_t n = std::max<int64_t>(1, (off[r + 1] - off[r] + g.seg_windows - 1) / g.seg_windows);
            pl->seg_first[(size_t) r] = pl->n_seg;
            pl->n_seg += n;
            if (!g.partials) continue;
            pl->part_first[(size_t) r] = pl->n_part;
            if (n > 1) { pl->n_part += n; pl->long_regions.push_back(r); }
        }
        pl->seg_first[(size_t) R] = pl->n_seg;
        if (g.partials) pl->part_first[(size_t) R] = pl->n_part;
    }
    pl->tile_first.push_back(0);
    size_t in_tile = 0;
    int32_t prev = -2;
    for (int32_t m = 0; m < P; m++) {
        if (!walked(m)) { pl->skipped.push_back(m); continue; }
        const size_t e = (size_t) widths[m] * 4;
        if (widths[m] > g.tile_max_w) continue;
        if (in_tile > 0 && (prev != m - 1 || in_tile + e > (size_t) g.tile_entries)) { pl->tile_first.push_back((int32_t) pl->mot.size()); in_tile = 0; }
        pl->mot.push_back(m);
        in_tile += e;
        pl->max_tile = std::max(pl->max_tile, in_tile);
        prev = m;
    }
    if (in_tile > 0) pl->tile_first.push_back((int32_t) pl->mot.size());
    pl->wide_first.push_back((int32_t) pl->mot.size());
    for (int32_t m = 0; m < P; m++)
        if (widths[m] > g.tile_max_w && walked(m)) { pl->mot.push_back(m); pl->wide_first.push_back((int32_t) pl->mot.size()); }
}

// A plan's arrays in the caller's work block: dense_slots adds them to the block's layout, each at the length the plan has (an empty
// one takes no room); dense_upload (ms_best.hip) copies them there.  The caller adds its own slots to the same Carve.
struct DenseSlots {
    Carve::Slot<int64_t> seg_first, part_first, long_regions;
    Carve::Slot<int32_t> mot, tile_first, wide_first, skipped;
};

inline DenseSlots dense_slots(Carve &cv, const DensePlan &pl) {
    DenseSlots s;
    s.seg_first = cv.add<int64_t>(pl.seg_first.size());
    s.part_first = cv.add<int64_t>(pl.part_first.size());
    s.long_regions = cv.add<int64_t>(pl.long_regions.size());
    s.mot = cv.add<int32_t>(pl.mot.size());
    s.tile_first = cv.add<int32_t>(pl.tile_first.size());
    s.wide_first = cv.add<int32_t>(pl.wide_first.size());
    s.skipped = cv.add<int32_t>(pl.skipped.size());
    return s;
}

}  // namespace ms
