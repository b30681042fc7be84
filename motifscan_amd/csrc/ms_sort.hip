// ms_sort.hip -- ordering of the sparse hit list (keys = motif | position | strand bit,
// values = fp64 scores).  The hit list is ~1e-4 of the scanned units, so this is not the hot
// kernel; rocPRIM's device radix sort (AMD's own header-only primitives) is used as is -- but for sort_hit_pairs_counted, which
// runs the same passes from digit counts the caller brings.
// Kept in its own translation unit because the rocPRIM headers dominate compile time.  Also here, for the same reason: the scans of
// ms_personal.hip and the row sorts of ms_ranksum.hip.
#include <algorithm>
#include <cstring>
#include <variant>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "ms_internal.h"

namespace ms {

int sort_hit_pairs(void *temp, size_t *temp_bytes, const uint64_t *keys_in, uint64_t *keys_out,
                   const double *vals_in, double *vals_out, size_t n, int begin_bit, int end_bit, hipStream_t stream) {
    if (end_bit < 1) end_bit = 1;
    if (end_bit > 64) end_bit = 64;
    if (begin_bit < 0 || begin_bit >= end_bit) begin_bit = 0;
    // (rocPRIM's gfx950 configuration for 8-byte keys with 8-byte values: 1024 threads x 8 items, 8 bits per pass, "match" ranking.
    // Ten bits per pass -- four passes instead of five over a scan's 38 ... 41 key bits -- measured slower: 3.25 against 2.81 ms for
    // 6.2e7 pairs, profiles/r03l_sort_bits.log.)
    MS_HIP(rocprim::radix_sort_pairs(temp, *temp_bytes, keys_in, keys_out, vals_in, vals_out, n, (unsigned int) begin_bit, (unsigned int) end_bit, stream));
    return MS_OK;
}

// The same passes on a list whose digit counts the caller has (a bucketed hit list: BucketOut::hist, ms_kernels.h): the steps of rocPRIM's
// radix_sort_onesweep_impl without its histogram kernel -- the same partition of the temporary storage, an exclusive scan of every place's
// counts into the place's digit offsets, then radix_sort_onesweep_iteration per place, which resets its own lookback states.  That is an
// interface of rocPRIM's detail namespace, so this is tied to the version it was read in; any other takes the public call.
namespace {
// (counts that do not add up to the list's length would send a pass's scatter out of the list: such a place gets zero offsets, which keep
// every key inside it -- in no useful order; the counts of a scan that is kept always add up)
__global__ void __launch_bounds__(256) digit_offsets_kernel(const unsigned long long *__restrict__ counts, size_t *__restrict__ offsets, size_t n) {
    __shared__ unsigned long long s[256];
    const int d = (int) threadIdx.x;
    const unsigned long long c = counts[blockIdx.x * 256 + d];
    s[d] = c;
    __syncthreads();
    for (int k = 1; k < 256; k <<= 1) {
        const unsigned long long v = d >= k ? s[d - k] : 0ULL;
        __syncthreads();
        s[d] += v;
        __syncthreads();
    }
    offsets[blockIdx.x * 256 + d] = s[255] == (unsigned long long) n ? (size_t) (s[d] - c) : (size_t) 0;
}
}  // namespace

int sort_hit_pairs_counted(void *temp, size_t *temp_bytes, const uint64_t *keys_in, uint64_t *keys_out, const double *vals_in, double *vals_out,
                           size_t n, int begin_bit, int end_bit, const unsigned long long *counts, bool *done, hipStream_t stream) {
    *done = false;
#if ROCPRIM_VERSION == 400200
    namespace rd = rocprim::detail;
    if (n == 0 || begin_bit < 0 || end_bit > 64 || begin_bit >= end_bit || (temp && !counts)) return MS_OK;
    using config = rd::wrapped_radix_sort_onesweep_config<rocprim::default_config, uint64_t, double>;
    rd::target_arch target_arch;
    MS_HIP(rd::host_target_arch(stream, target_arch));
    const rd::radix_sort_onesweep_config_params params = rd::dispatch_target_arch<config, false>(target_arch);
    if (params.radix_bits_per_place != 8) return MS_OK;
    bool use_atomic_block_id;
    MS_HIP(rd::check_if_using_atomic_block_id(stream, use_atomic_block_id));
    const auto variant = rd::constexpr_value_variant<bool, false, true>::create(use_atomic_block_id);
    hipError_t err = hipSuccess;
    std::visit(
        [&](auto atomic_id) {
            using ordered_bid_type = rd::block_id_wrapper<unsigned int, atomic_id>;
            const unsigned int items_per_block = params.sort.block_size * params.sort.items_per_thread;
            const unsigned int full_batch = (1u << 30) - (1u << 30) % items_per_block;
            const unsigned int places = (unsigned int) (end_bit - begin_bit + 7) / 8;
            const unsigned int items_per_batch = (unsigned int) std::min<size_t>(n, full_batch);
            const unsigned int num_lookback_states = 256u * rd::ceiling_div(items_per_batch, items_per_block);
            size_t *offsets = nullptr, *offsets_tmp = nullptr;
            rd::onesweep_lookback_state *lookback_states = nullptr;
            uint64_t *keys_tmp = nullptr;
            double *vals_tmp = nullptr;
            typename ordered_bid_type::id_type *bid_storage = nullptr;
            size_t need = 0;
            for (int pass = 0; pass < 2 && err == hipSuccess; pass++) {            // the size, then the pointers
                size_t bytes = pass ? *temp_bytes : 0;
                err = rd::temp_storage::partition(
                    pass ? temp : nullptr, bytes,
                    rd::temp_storage::make_linear_partition(
                        rd::temp_storage::ptr_aligned_array(&offsets, 256u * places), rd::temp_storage::ptr_aligned_array(&offsets_tmp, 256u),
                        rd::temp_storage::ptr_aligned_array(&lookback_states, num_lookback_states), rd::temp_storage::ptr_aligned_array(&keys_tmp, n),
                        rd::temp_storage::ptr_aligned_array(&vals_tmp, n),
                        rd::temp_storage::make_partition(&bid_storage, ordered_bid_type::get_temp_storage_layout())));
                if (!pass) {
                    need = bytes;
                    if (!temp) { *temp_bytes = need; *done = true; return; }         // the size query
                    if (need > *temp_bytes) return;
                }
            }
            if (err != hipSuccess) return;
            auto ordered_bid = ordered_bid_type::create(bid_storage);
            hipLaunchKernelGGL(digit_offsets_kernel, dim3(places), dim3(256), 0, stream, counts, offsets, n);
            if ((err = hipGetLastError()) != hipSuccess) return;
            bool to_output = (places - 1) % 2 == 0, from_input = true;
            for (unsigned int bit = (unsigned int) begin_bit, place = 0; bit < (unsigned int) end_bit; bit += 8, place++) {
                err = rd::radix_sort_onesweep_iteration<rocprim::default_config, false>(
                    keys_in, keys_tmp, keys_out, vals_in, vals_tmp, vals_out, n, offsets + place * 256, offsets_tmp, lookback_states, from_input,
                    to_output, rocprim::identity_decomposer{}, bit, (unsigned int) end_bit, ordered_bid, stream, false);
                if (err != hipSuccess) return;
                from_input = false;
                to_output = !to_output;
            }
            *done = true;
        },
        variant);
    MS_HIP(err);
#endif
    return MS_OK;
}

int sort_keys(void *temp, size_t *temp_bytes, const uint64_t *keys_in, uint64_t *keys_out, size_t n, int end_bit, hipStream_t stream) {
    if (end_bit < 1) end_bit = 1;
    if (end_bit > 64) end_bit = 64;
    MS_HIP(rocprim::radix_sort_keys(temp, *temp_bytes, keys_in, keys_out, n, 0u, (unsigned int) end_bit, stream));
    return MS_OK;
}

namespace {
struct RowOffset {                                  // segment i of a [rows][n] array starts at i * n
    unsigned int n;
    __host__ __device__ unsigned int operator()(unsigned int i) const { return i * n; }
};
}  // namespace

int sort_key_rows(void *temp, size_t *temp_bytes, const uint64_t *in, uint64_t *out, size_t rows, size_t n, bool segmented, hipStream_t stream) {
    if (segmented) {
        const auto begin = rocprim::make_transform_iterator(rocprim::make_counting_iterator<unsigned int>(0u), RowOffset{(unsigned int) n});
        MS_HIP(rocprim::segmented_radix_sort_keys(temp, *temp_bytes, in, out, (unsigned int) (rows * n), (unsigned int) rows, begin, begin + 1, 0u, 64u, stream));
        return MS_OK;
    }
    if (!temp) {
        MS_HIP(rocprim::radix_sort_keys(temp, *temp_bytes, in, out, n, 0u, 64u, stream));
        return MS_OK;
    }
    for (size_t i = 0; i < rows; i++) {
        size_t tb = *temp_bytes;
        MS_HIP(rocprim::radix_sort_keys(temp, tb, in + i * n, out + i * n, n, 0u, 64u, stream));
    }
    return MS_OK;
}

int sort_doubles_desc(void *temp, size_t *temp_bytes, const double *in, double *out, size_t n, hipStream_t stream) {
    MS_HIP(rocprim::radix_sort_keys_desc(temp, *temp_bytes, in, out, n, 0u, 64u, stream));
    return MS_OK;
}

int exclusive_sum_u32(void *temp, size_t *temp_bytes, const uint32_t *in, uint64_t *out, size_t n, hipStream_t stream) {
    MS_HIP(rocprim::exclusive_scan(temp, *temp_bytes, in, out, (uint64_t) 0, n, rocprim::plus<uint64_t>(), stream));
    return MS_OK;
}

int inclusive_max_u64(void *temp, size_t *temp_bytes, const uint64_t *in, uint64_t *out, size_t n, hipStream_t stream) {
    MS_HIP(rocprim::inclusive_scan(temp, *temp_bytes, in, out, n, rocprim::maximum<uint64_t>(), stream));
    return MS_OK;
}

int exclusive_sum_i64(void *temp, size_t *temp_bytes, const int64_t *in, int64_t *out, size_t n, hipStream_t stream) {
    MS_HIP(rocprim::exclusive_scan(temp, *temp_bytes, in, out, (int64_t) 0, n, rocprim::plus<int64_t>(), stream));
    return MS_OK;
}

}  // namespace ms
