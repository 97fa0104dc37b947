// The refusals of msr_match_sets (include/msretr_match.h) as a host function of plain values: no engine, no device, no HIP type,
// so that a program of its own can call it under the host sanitizers (tests/match_args_check.cpp).  msr_engine.hip calls it
// before anything is launched.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "../../include/msretr_match.h"

// MSR_OK, or MSR_ERR_INVALID with the reason in why[0 .. cap) (always terminated when cap > 0).  n_docs: of the bound postings;
// rows_ok: out_bits, row_group_off, group_term_off and row_need are all non-NULL; base_ok: base_bits and row_base are.
inline int msr_match_args_check(int64_t n_docs, int32_t n_rows, bool rows_ok, int64_t out_stride, int32_t n_base, bool base_ok,
                                int64_t base_stride, char* why, size_t cap) {
    const int64_t W = (n_docs + 31) / 32;
    if (cap > 0) why[0] = 0;
    if (n_rows < 0 || n_base < 0) {
        snprintf(why, cap, "msr_match_sets: bad argument (n_rows=%d, n_base=%d)", n_rows, n_base);
        return MSR_ERR_INVALID;
    }
    if (n_rows > 0 && !rows_ok) {
        snprintf(why, cap, "msr_match_sets: bad argument (out_bits, row_group_off, group_term_off or row_need is NULL with n_rows=%d)",
                 n_rows);
        return MSR_ERR_INVALID;
    }
    if (out_stride < W) {
        snprintf(why, cap, "msr_match_sets: bad argument (out_stride=%lld < ceil(n_docs / 32) = %lld)", (long long)out_stride,
                 (long long)W);
        return MSR_ERR_INVALID;
    }
    if (n_base > 0 && !base_ok) {
        snprintf(why, cap, "msr_match_sets: bad argument (base_bits or row_base is NULL with n_base=%d)", n_base);
        return MSR_ERR_INVALID;
    }
    if (n_base > 0 && base_stride < W) {
        snprintf(why, cap, "msr_match_sets: bad argument (base_stride=%lld < ceil(n_docs / 32) = %lld)", (long long)base_stride,
                 (long long)W);
        return MSR_ERR_INVALID;
    }
    return MSR_OK;
}
