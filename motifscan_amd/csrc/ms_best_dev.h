// ms_best_dev.h -- what the "best window of a cell" kernels share (ms_best.hip: per region; ms_allelebest.hip: per variant haplotype):
// the total-order wave reduction and the test for a motif the reference never reports a site of.
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
