// ms_best_dev.h -- what the "best window of a cell" kernels share (ms_best.hip: per region; ms_allelebest.hip: per variant haplotype):
// the total-order wave reduction and the test for a motif the reference never reports a site of; and, with ms_scorehist.hip (the score
// histogram walks the windows as ms_best.hip does), the column loop over an LDS tile of tables.
#pragma once
#include <cmath>
#include <limits>

#include "ms_device.h"
#include "ms_handles.h"

namespace ms {

namespace {

constexpr uint64_t kNoKey = ~0ULL;

// (q, key) of the wave's lanes -> the winner in every lane: the greater q, equal q to the smaller key = pos << 2 | strand
__device__ __forceinline__ void wave_best(double &q, uint64_t &key) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double oq = __shfl_xor(q, d);
        const unsigned long long ok = __shfl_xor((unsigned long long) key, d);
        if (oq > q || (oq == q && ok < key)) { q = oq; key = ok; }
    }
}

// (the dense walks over an LDS tile of tables: best_kernel, scorehist_kernel) up to 32 columns out of the registers: table entries tb + 4 c of the LDS tile, in column order; bit c of skip: the column adds entry 0
__device__ __forceinline__ void best_cols32(const double2 *__restrict__ lds, uint32_t tb, int n, uint64_t cw, uint32_t skip, double &fwd, double &rev) {
    for (int c1 = 0; c1 < n; c1 += 8) {
        const uint32_t bits = (uint32_t) (cw >> (2 * c1)), sk = skip >> c1;
        double2 t[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t idx = tb + (uint32_t) (c1 + k) * 4u + ((bits >> (2 * k)) & 3u);
            t[k] = lds[((sk >> k) & 1u) ? 0u : idx];
        }
#pragma unroll
        for (int k = 0; k < 8; k++) { fwd += t[k].x; rev += t[k].y; }
    }
}

// the reference never reports a site of such a motif: max_raw is not a finite number > 0, or an entry is NaN or +inf
inline bool scorable(const ms_pwmset *p, int32_t m) {
    const double mr = p->max_raw[(size_t) m];
    if (!(std::isfinite(mr) && mr > 0.0)) return false;
    const double *v = p->values.data() + p->val_off[(size_t) m];
    const int64_t n = 4 * (int64_t) p->widths[(size_t) m];
    for (int64_t i = 0; i < n; i++)
        if (std::isnan(v[i]) || v[i] == std::numeric_limits<double>::infinity()) return false;
    return true;
}

}  // namespace

}  // namespace ms
