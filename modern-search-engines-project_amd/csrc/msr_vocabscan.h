// What the two lookups over the bound vocabulary share (K15 msr_fuzzy.hip, K16 msr_wildcard.hip): both
// give one workgroup MSR_FUZZY_SPAN_TERMS consecutive terms, one lane per term, pass the call's words or patterns through LDS
// MSR_FUZZY_WORD_GROUP at a time, and turn a hit into one 64-bit key; both leave the first `limit` keys of every span in
// caller scratch and merge them per word with msr_sort.h's bitonic network.  Here are the pieces that are the same in both:
// the character-set signature bit, the 64-bit shuffles and wave minimum, the key layout, the first-`limit` extraction of a
// wave, the step in which wave v of a workgroup merges the 16 waves' lists of word v into the span's scratch slot, and the
// whole merge kernel's body (with or without a row of distances).  Every function is inlined into its kernel; none holds
// state.  No atomics anywhere: the same bytes every time.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msretr.h"
#include "msr_sort.h"

namespace msr_vocabscan {

constexpr int VS_SPAN = MSR_FUZZY_SPAN_TERMS;                // terms of one workgroup of a scan, one lane each
constexpr int VS_WAVES = VS_SPAN / 64;
constexpr int VS_G = MSR_FUZZY_WORD_GROUP;                   // words (patterns) staged in LDS at a time
constexpr int VS_LEN = MSR_FUZZY_MAX_LEN;                    // code points of the longest term a lane keeps
constexpr int VS_LIM = MSR_FUZZY_MAX_LIMIT;
constexpr uint64_t VS_NONE = ~0ull;                          // "no candidate": distance 3, which no key has
constexpr int MG_THREADS = 256;
constexpr int MG_CAP = 2048;                                 // keys of one sort of the merge
static_assert(VS_SPAN == 1024, "one lane per term, the largest workgroup");
static_assert(VS_G == VS_WAVES, "wave v of a scan merges word v of the group");
static_assert(VS_LEN == 32 && VS_G * 32 <= VS_SPAN, "32 staging threads per word, a term in 16 registers");
static_assert(VS_LIM <= 64 && VS_WAVES * VS_LIM <= 256, "a wave holds a group's lists in four keys per lane");
static_assert((MG_CAP - VS_LIM) / VS_LIM >= 1, "a round of the merge takes at least one span");

__device__ __forceinline__ uint64_t sig_bit(uint32_t c) { return 1ull << ((c * 0x9E3779B1u) >> 26); }

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
    for (int m = 32; m; m >>= 1) {
        const uint64_t o = shfl_xor_u64(v, m);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }

// A candidate is one 64-bit key -- 2 bits distance (0 where the lookup has none), 31 bits 0x7FFFFFFF - weight, 31 bits term id:
// smaller is better, no two are equal.  key_low: the part a lane knows for the whole kernel (weight below 2^31, term id too).
__device__ __forceinline__ uint64_t key_low(uint32_t weight, int64_t term) {
    return ((uint64_t)(0x7FFFFFFFu - weight) << 31) | (uint64_t)term;
}

// The first `limit` keys of a wave in ascending order, key r in lane r (VS_NONE where there is none).  mine[0 .. N): the
// lane's own keys.  Every lane of the wave calls it.
template <int N>
__device__ __forceinline__ uint64_t wave_first_keys(uint64_t (&mine)[N], int limit, int lane) {
    uint64_t keep = VS_NONE;
    for (int r = 0; r < limit; ++r) {
        uint64_t lo = mine[0];
#pragma unroll
        for (int k = 1; k < N; ++k) lo = mine[k] < lo ? mine[k] : lo;
        const uint64_t mn = wave_min_u64(lo);
        if (mn == VS_NONE) break;                            // (wave-uniform)
        if (lane == r) keep = mn;
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (mine[k] == mn) mine[k] = VS_NONE;            // (keys are unique: exactly one goes)
    }
    return keep;
}

// One wave merges the VS_WAVES lists of `limit` keys and the VS_WAVES counts the workgroup's waves left in LDS for one word
// (s_key [VS_WAVES * limit], s_cnt [VS_WAVES]) and writes the span's slot of the scratch: keys[slot][limit] (absent: all ones)
// and counts[slot].  Every lane of the wave calls it, after the barrier behind the lists.
__device__ __forceinline__ void span_slot_store(const uint64_t* s_key, const int32_t* s_cnt, int limit, int lane, int64_t slot,
                                                uint64_t* keys, int32_t* counts) {
    uint64_t e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = lane + 64 * k;
        e[k] = idx < VS_WAVES * limit ? s_key[idx] : VS_NONE;
    }
    int total = lane < VS_WAVES ? s_cnt[lane] : 0;
    for (int mk = 32; mk; mk >>= 1) total += __shfl_xor(total, mk);
    uint64_t keep = VS_NONE;
    if (total > 0) keep = wave_first_keys<4>(e, limit, lane);
    if (lane < limit) keys[slot * limit + lane] = keep;
    if (lane == 0) counts[slot] = total;
}

// The merge kernel's body: workgroup w (MG_THREADS threads) sums the counts of word w's spans and sorts their keys, MG_CAP at
// a time, the best `limit` so far riding along; a block of spans without any key is not sorted.  It writes the word's row:
// term ids (and, WITH_DIST, distances), -1 behind them, n and the total.
template <bool WITH_DIST>
__device__ __forceinline__ void merge_rows(const uint64_t* keys, const int32_t* counts, int n_spans, int limit, int32_t* out_term,
                                           int32_t* out_dist, int32_t* out_n, int32_t* out_total) {
    __shared__ uint64_t s_hi[MG_CAP];
    __shared__ uint32_t s_lo[MG_CAP];                         // the sort's key extension: unused, all zero
    __shared__ int32_t s_sum[MG_THREADS / 64];
    const int tid = (int)threadIdx.x, w = (int)blockIdx.x;
    const int64_t base = (int64_t)w * n_spans;
    for (int i = tid; i < MG_CAP; i += MG_THREADS) s_lo[i] = 0;
    if (tid < limit) s_hi[tid] = VS_NONE;
    int sum = 0;
    for (int s = tid; s < n_spans; s += MG_THREADS) sum += counts[base + s];
    for (int mk = 32; mk; mk >>= 1) sum += __shfl_xor(sum, mk);
    if ((tid & 63) == 0) s_sum[tid >> 6] = sum;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int k = 0; k < MG_THREADS / 64; ++k) total += s_sum[k];
    if (total > 0) {                                         // (the same in every thread)
        const int per = (MG_CAP - limit) / limit;            // spans of one round: their keys and the best so far fit the sort
        for (int s0 = 0; s0 < n_spans; s0 += per) {
            const int ne = imin(per, n_spans - s0) * limit;
            int P = 2;
            while (P < limit + ne) P <<= 1;
            const uint64_t* src = keys + (base + s0) * limit;                 // the round's keys are contiguous
            int any = 0;
            for (int i = tid; i < P - limit; i += MG_THREADS) {
                const uint64_t k = i < ne ? src[i] : VS_NONE;
                s_hi[limit + i] = k;
                any |= k != VS_NONE;
            }
            if (__syncthreads_or(any)) msr_sort::bitonic_sort<MG_THREADS, false>(s_hi, s_lo, nullptr, P, true);
        }
    }
    __syncthreads();
    if (tid < limit) {
        const uint64_t k = s_hi[tid];
        out_term[(int64_t)w * limit + tid] = k == VS_NONE ? -1 : (int32_t)(k & 0x7FFFFFFFu);
        if (WITH_DIST) out_dist[(int64_t)w * limit + tid] = k == VS_NONE ? -1 : (int32_t)(k >> 62);
    }
    if (tid == 0) { out_total[w] = total; out_n[w] = imin(total, limit); }
}

}  // namespace msr_vocabscan
