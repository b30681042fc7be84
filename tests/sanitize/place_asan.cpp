// tests/sanitize/place_asan.cpp -- the host arithmetic of the variant scans' record placement (motifscan_amd/csrc/ms_place.h: the chunk
// plan, the record offsets, the layout of a carved block) under AddressSanitizer + UndefinedBehaviorSanitizer, compiled by plain g++ from
// the header the library is built from.  Every array is allocated at exactly the size the plan promises, so a walk past it stops the run.
// CPU build container only (`make -C motifscan_amd/csrc sanitize`).
#include "ms_place.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static int n_plans = 0;

// the plan's invariants, then the placement driver's walk over it with arrays of the promised sizes
static void check_plan(int64_t V, int32_t P, int tile, int64_t max_tiles, int64_t setting, std::mt19937_64 &rng) {
    const ms::PlaceChunks c = ms::place_chunks(V, P, tile, max_tiles, setting);
    n_plans++;
    const int32_t Pz = P > 0 ? P : 1;
    CHECK(c.chunk >= 1 && c.chunk <= (V > 0 ? V : 1));
    if (setting > 0) CHECK(c.chunk == (setting < (V > 0 ? V : 1) ? setting : (V > 0 ? V : 1)));
    CHECK(c.n_chunks * c.chunk >= V && V > (c.n_chunks - 1) * c.chunk);
    CHECK(c.ntx_max == (c.chunk + tile - 1) / tile && c.ntx_max >= 1);
    CHECK(c.n_cells == (size_t) c.ntx_max * (size_t) Pz + 1);
    if (setting <= 0 && c.n_chunks > 1) CHECK(c.chunk % tile == 0 && c.ntx_max * Pz <= (max_tiles > Pz ? max_tiles : Pz));

    // the counts of every chunk fit the count array: [P][ntx] and the entry that closes the prefix sums
    std::vector<uint32_t> cnt(c.n_cells);
    std::vector<uint64_t> h_tot((size_t) c.n_chunks * P), h_base((size_t) c.n_chunks * P);
    std::vector<int64_t> motif_offsets((size_t) P + 1, -1);
    int64_t seen = 0;
    uint64_t sum = 0;
    for (int64_t k = 0; k < c.n_chunks; k++) {
        const int64_t v0 = k * c.chunk, nv = c.chunk < V - v0 ? c.chunk : V - v0, ntx = (nv + tile - 1) / tile;
        CHECK(nv >= 1 && ntx <= c.ntx_max);
        const size_t cells = (size_t) ntx * (size_t) P;
        CHECK(cells + 1 <= c.n_cells);
        std::memset(cnt.data(), 0, 4 * (cells + 1));
        for (int32_t m = 0; m < P; m++) {
            uint64_t row = 0;
            for (int64_t t = 0; t < ntx; t++) { cnt[(size_t) m * ntx + t] = (uint32_t) (rng() % 5); row += cnt[(size_t) m * ntx + t]; }
            h_tot[(size_t) k * P + m] = row;
            sum += row;
        }
        seen += nv;
    }
    CHECK(seen == V);
    if (V == 15 && setting == 7) CHECK(c.n_chunks == 3 && V - 2 * c.chunk == 1);

    const uint64_t n = ms::place_offsets(h_tot.data(), c.n_chunks, P, motif_offsets.data(), h_base.data());
    CHECK(n == sum && motif_offsets[(size_t) P] == (int64_t) sum && motif_offsets[0] == 0);
    uint64_t at = 0;                                  // h_base ascends in (motif, chunk) order, every run right behind the one before
    for (int32_t m = 0; m < P; m++) {
        CHECK(motif_offsets[(size_t) m] == (int64_t) at);
        for (int64_t k = 0; k < c.n_chunks; k++) {
            CHECK(h_base[(size_t) k * P + m] == at);
            at += h_tot[(size_t) k * P + m];
        }
    }
    CHECK(at == sum);
}

template <typename T>
static void touch(void *base, ms::Carve::Slot<T> s, size_t n, size_t total, std::vector<std::pair<size_t, size_t>> &spans) {
    CHECK(s.off % 256 == 0);
    CHECK(s.off + n * sizeof(T) <= total);
    T *p = ms::Carve::at(base, s);
    CHECK(reinterpret_cast<char *>(p) == static_cast<char *>(base) + s.off);
    for (size_t i = 0; i < n; i++) p[i] = T();
    spans.emplace_back(s.off, s.off + n * sizeof(T));
}

static void check_carve() {
    struct Rec { int64_t a, b; int32_t c, d; };
    const size_t lens[] = {0, 1, 255, 256, 257, 1000};
    for (size_t n0 : lens)
        for (size_t n1 : lens) {
            ms::Carve cv;
            CHECK(cv.bytes() == 0);
            const auto s0 = cv.add<int32_t>(n0);
            const auto s1 = cv.add<uint8_t>(n1);
            const auto s2 = cv.add<Rec>(3);
            const auto s3 = cv.add<int64_t>(0);       // a slot of no elements among them
            const auto s4 = cv.add<double>(n0 + n1);
            const auto s5 = cv.add<char>(1);
            const size_t total = cv.bytes();
            CHECK(total % 256 == 0 && total >= 256);
            void *base = std::aligned_alloc(256, total);
            CHECK(base != nullptr);
            std::vector<std::pair<size_t, size_t>> spans;
            touch(base, s0, n0, total, spans);
            touch(base, s1, n1, total, spans);
            touch(base, s2, 3, total, spans);
            touch(base, s3, 0, total, spans);
            touch(base, s4, n0 + n1, total, spans);
            touch(base, s5, 1, total, spans);
            for (size_t i = 1; i < spans.size(); i++) CHECK(spans[i - 1].second <= spans[i].first);      // in order, none over another
            std::free(base);
        }
    CHECK(ms::Carve::up(0) == 0 && ms::Carve::up(1) == 256 && ms::Carve::up(256) == 256 && ms::Carve::up(257) == 512);
}

int main() {
    std::mt19937_64 rng(11);
    const int tile = 128;
    const int64_t Vs[] = {0, 1, 127, 128, 129}, settings[] = {0, 7, 128, 129}, caps[] = {1, 2, 1LL << 24};
    const int32_t Ps[] = {0, 1, 3};
    for (int64_t V : Vs)
        for (int32_t P : Ps)
            for (int64_t setting : settings)
                for (int64_t cap : caps) check_plan(V, P, tile, cap, setting, rng);
    for (int32_t P : Ps) check_plan(15, P, tile, 1LL << 24, 7, rng);       // three chunks, the last of one variant
    for (int32_t P : Ps) check_plan(1000, P, tile, 2, 0, rng);             // chunks sized by the cap: more than one
    check_carve();
    std::printf("place_asan: ok (%d plans)\n", n_plans);
    return 0;
}
