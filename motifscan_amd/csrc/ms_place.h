// ms_place.h -- the host arithmetic of the two-pass record placement (place_records, ms_variants.hip) and of a work block's layout: plain
// C++, no HIP call, so that it is checked on the CPU (tests/sanitize/place_asan.cpp), as ms_scan_geom.cpp is.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ms {

// One device block carved into arrays.  add<T>(n) reserves n elements and returns their slot, bytes() is what to allocate, at(base, slot)
// the array's pointer in a block of that size.  Every slot is rounded up to kAlign bytes; a slot of no elements takes none.
struct Carve {
    static constexpr size_t kAlign = 256;
    static constexpr size_t up(size_t x) { return (x + kAlign - 1) & ~(kAlign - 1); }
    template <typename T>
    struct Slot { size_t off = 0; };
    template <typename T>
    Slot<T> add(size_t n) {
        const Slot<T> s{total_};
        total_ += up(n * sizeof(T));
        return s;
    }
    size_t bytes() const { return total_; }
    template <typename T>
    static T *at(void *base, Slot<T> s) { return reinterpret_cast<T *>(static_cast<char *>(base) + s.off); }

private:
    size_t total_ = 0;
};

// V variants in chunks, so that one chunk's (motif, tile) counts stay bounded: `setting` variants a chunk (ms_debug_varscan_chunk), or
// with setting <= 0 as many tiles of `tile` variants as keep the P rows of counts within max_tiles.
struct PlaceChunks {
    int64_t chunk = 1;            // variants per chunk (the last chunk may have fewer)
    int64_t n_chunks = 0;
    int64_t ntx_max = 1;          // tiles of a full chunk
    size_t n_cells = 1;           // counts of a full chunk: [P][ntx_max] and the entry that closes their prefix sums
};

inline PlaceChunks place_chunks(int64_t V, int32_t P, int tile, int64_t max_tiles, int64_t setting) {
    PlaceChunks c;
    c.chunk = setting > 0 ? setting : std::max<int64_t>(1, max_tiles / std::max<int32_t>(P, 1)) * tile;
    c.chunk = std::min<int64_t>(c.chunk, std::max<int64_t>(V, 1));
    c.n_chunks = V > 0 ? (V + c.chunk - 1) / c.chunk : 0;
    c.ntx_max = (c.chunk + tile - 1) / tile;
    c.n_cells = (size_t) c.ntx_max * (size_t) std::max<int32_t>(P, 1) + 1;
    return c;
}

// Out of h_tot[n_chunks][P], the records of every (chunk, motif): motif_offsets[P + 1], and h_base[n_chunks][P], where the records of
// (chunk, motif) start -- the output is motif-major, a motif's chunks in order.  Returns the number of records.
inline uint64_t place_offsets(const uint64_t *h_tot, int64_t n_chunks, int32_t P, int64_t *motif_offsets, uint64_t *h_base) {
    uint64_t at = 0;
    for (int32_t m = 0; m < P; m++) {
        motif_offsets[m] = (int64_t) at;
        for (int64_t k = 0; k < n_chunks; k++) {
            h_base[(size_t) k * P + m] = at;
            at += h_tot[(size_t) k * P + m];
        }
    }
    motif_offsets[P] = (int64_t) at;
    return at;
}

}  // namespace ms
