// at_sort.h -- the library's rocPRIM radix sort (not installed; kept out of at_internal.h because it pulls in rocPRIM).
#pragma once
#include <rocprim/rocprim.hpp>

#include "at_internal.h"

// Onesweep radix sort at every size: below a million items rocPRIM would switch to a merge sort of ~18
// small launches, which is what an iteration of a sharded (N-GPU) run would then mostly consist of;
// the keys of the Lloyd iteration are 13-21 bits wide, two or three onesweep passes.
using at_radix_config = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, 0>;

// Stable sort of n (key, value) pairs by bits [begin_bit, end_bit) of the key, rocPRIM's temporary storage in the
// context's slot `tmp_slot`; the result is in keys.current() / vals.current().  (A template so that a file which only
// wants the configuration does not instantiate the sort's kernels.)
template <typename Key, typename Value>
static inline int at_sort_pairs(at_ctx* ctx, int tmp_slot, rocprim::double_buffer<Key>& keys, rocprim::double_buffer<Value>& vals,
                                size_t n, unsigned begin_bit, unsigned end_bit, hipStream_t stream) {
    size_t tmp_bytes = 0;
    AT_HIP(rocprim::radix_sort_pairs<at_radix_config>(nullptr, tmp_bytes, keys, vals, n, begin_bit, end_bit, stream));
    void* tmp = at_ws(ctx, tmp_slot, tmp_bytes, stream);
    if (!tmp) return AT_E_NOMEM;
    AT_HIP(rocprim::radix_sort_pairs<at_radix_config>(tmp, tmp_bytes, keys, vals, n, begin_bit, end_bit, stream));
    return AT_OK;
}

// The same for keys alone; the result is in keys.current().
template <typename Key>
static inline int at_sort_keys(at_ctx* ctx, int tmp_slot, rocprim::double_buffer<Key>& keys, size_t n, unsigned begin_bit,
                               unsigned end_bit, hipStream_t stream) {
    size_t tmp_bytes = 0;
    AT_HIP(rocprim::radix_sort_keys<at_radix_config>(nullptr, tmp_bytes, keys, n, begin_bit, end_bit, stream));
    void* tmp = at_ws(ctx, tmp_slot, tmp_bytes, stream);
    if (!tmp) return AT_E_NOMEM;
    AT_HIP(rocprim::radix_sort_keys<at_radix_config>(tmp, tmp_bytes, keys, n, begin_bit, end_bit, stream));
    return AT_OK;
}
