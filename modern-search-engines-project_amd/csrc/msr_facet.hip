// K17: facet counts of whole match sets (msr_bind_facet, msr_facet_counts, include/msretr.h).
//
// Row r's match set is  M(r) = base(r)  AND  (OR of D(t) for the row's terms t)  -- K11's base rows and posting lists -- and the
// call returns |M(r)|, the number of matches per facet value, and the values with the most matches.  A facet is one int32 value
// per document; the host (msr_facet_table) turns it into a per-span dictionary: span s of MSR_TERMSET_SPAN_DOCS documents holds
// cnt(s) <= SPAN distinct values, document d carries the position local[d] of its value in its span's list (16 bits), and
// value_pos lists, per value, the slots of the concatenated dictionaries that hold it.
//
// Pass 1, one workgroup per (row, span) with K11's ownership rule (msr_tokscan.h): the row's word of the span in a register,
// the OR of the terms' postings in LDS bits (K11's not-list code), the AND, then one LDS atomicAdd per set bit into a histogram
// of the span's cnt(s) slots, stored as uint16 with plain coalesced stores -- every slot of every (row, span) is written, a
// count is at most SPAN.  Pass 2, one workgroup per row: value v's count is the sum of its slots (value_pos), the first `limit`
// values in (count desc, value asc) order are kept in LDS.  No global atomic, no memset, no float: every output byte is a
// function of the inputs.  The design that was NOT built is one global atomicAdd per matching document into count[row][value]:
// scattered global atomics run at about 1/17 of their contiguous rate, and half the corpus matches a typical row.
//
// LDS layout of the histogram: hist[slot], one dword per slot, slot = local[d].  ds_add_u32 banks by (address / 4) % 32 within a
// 32-lane half; the slots a wave's lanes add to in one instruction are those of 64 documents 32 apart (bit b of 64 consecutive
// words), which a dictionary in value order scatters over the banks.  Known cost, open: when one value dominates a span all
// lanes of a wave add to ONE address and the adds serialise.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/msretr.h"
#include "msr_internal.h"
#include "msr_tokscan.h"

namespace {

using namespace tokscan;
static_assert(SPAN <= 65535, "a slot's count (at most SPAN) is stored in 16 bits, and local ids stay below 0xFFFF");
static_assert(MSR_FACET_MAX_LIMIT <= 64 && MSR_FACET_MAX_LIMIT <= THREADS, "the running top list is merged by one thread per entry");
constexpr uint32_t NO_VALUE = 0xFFFFu;

struct FacetCountArgs {
    const int64_t* term_off;
    const int32_t* post_doc;
    const int32_t* heavy_id;     // nullable
    const uint32_t* tile_off;
    int64_t n_terms, n_docs;
    int32_t n_tiles;
    const int32_t* any_off; const int32_t* any_terms;
    const uint32_t* base_bits; int32_t n_base; int64_t base_stride; const int32_t* row_base;
    const uint16_t* local; const int32_t* span_off;
    uint16_t* part; int64_t part_stride;                 // [n_rows][part_stride] slot counts
    int32_t* hits_part; int32_t n_spans;                 // [n_rows][n_spans] matches per span
    int32_t row0;
};

// the sum of v over the workgroup; red: WAVES words of LDS.  Every thread calls it; a barrier stands at its start and its end.
__device__ __forceinline__ int block_sum(int v, int lane, int wave, int32_t* red) {
    for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    int total = 0;
    for (int i = 0; i < WAVES; ++i) total += red[i];
    return total;
}

__global__ __launch_bounds__(THREADS) void facet_count_kernel(const FacetCountArgs a) {
    __shared__ uint32_t bits[THREADS];
    __shared__ int64_t r_lo[THREADS], r_hi[THREADS];         // the span's postings of up to THREADS terms, found side by side
    __shared__ uint32_t hist[SPAN];
    __shared__ int32_t red[WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = a.row0 + (int)blockIdx.y;
    const int s = (int)blockIdx.x;
    const int64_t d0 = (int64_t)s * SPAN;
    const int64_t W = (a.n_docs + 31) >> 5;
    const int64_t w = (d0 >> 5) + tid;                   // this thread's word of the row
    const int x0 = a.any_off[r], x1 = a.any_off[r + 1];

    // base(r), without the bits at or above n_docs
    uint32_t acc = set_word(a.base_bits, a.n_base, a.base_stride, a.n_base > 0 ? a.row_base[r] : -1, w, W, a.n_docs);
    const int alive = __syncthreads_or(acc != 0);
    if (alive && x0 < x1) {                              // the terms share one OR (an empty list is no condition)
        bits[tid] = 0;
        for (int i0 = x0; i0 < x1; i0 += THREADS) {
            const int cnt = min(THREADS, x1 - i0);
            if (tid < cnt) {
                const int32_t t = a.any_terms[i0 + tid];
                int64_t lo = 0, hi = 0;
                if (t >= 0 && t < a.n_terms) span_postings(a, t, d0, &lo, &hi);
                r_lo[tid] = lo; r_hi[tid] = hi;
            }
            __syncthreads();
            for (int k = 0; k < cnt; ++k) or_postings(a.post_doc, r_lo[k], r_hi[k], d0, bits);
            __syncthreads();
        }
        acc &= bits[tid];
    }

    const int64_t t0 = a.span_off[s];
    const int cnt = min(max(a.span_off[s + 1] - a.span_off[s], 0), SPAN);
    for (int i = tid; i < cnt; i += THREADS) hist[i] = 0;
    const int hits = block_sum(__popc(acc), lane, wave, red);    // (its barriers: the zeroes are in place for every thread)
    if (tid == 0) a.hits_part[(int64_t)r * a.n_spans + s] = hits;

    if (acc) {                                           // a thread's 32 documents are 64 contiguous bytes of `local`
        const int64_t d = d0 + (int64_t)tid * 32;
#pragma unroll
        for (int p = 0; p < 4; ++p) {                    // 16 bytes = 8 documents at a time
            uint32_t m = (acc >> (8 * p)) & 0xFFu;
            if (!m) continue;
            const int64_t dp = d + 8 * p;
            uint32_t q[4];
            if (dp + 8 <= a.n_docs) {
                const uint4 v = *reinterpret_cast<const uint4*>(a.local + dp);
                q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
            } else {                                     // the corpus ends inside the piece: its set bits are all below n_docs
                q[0] = q[1] = q[2] = q[3] = 0xFFFFFFFFu;
                for (int j = 0; j < 8 && dp + j < a.n_docs; ++j) {
                    const uint32_t l = a.local[dp + j];
                    q[j >> 1] = (j & 1) ? (q[j >> 1] & 0x0000FFFFu) | (l << 16) : (q[j >> 1] & 0xFFFF0000u) | l;
                }
            }
            for (; m; m &= m - 1) {
                const int j = __ffs(m) - 1;
                const uint32_t l = (q[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
                if (l < (uint32_t)cnt) atomicAdd(&hist[l], 1u);     // (NO_VALUE and anything a stale table holds stay out of LDS)
            }
        }
    }
    __syncthreads();
    uint16_t* out = a.part + (int64_t)r * a.part_stride + t0;
    for (int i = tid; i < cnt; i += THREADS) out[i] = (uint16_t)hist[i];
}

struct FacetMergeArgs {
    const uint16_t* part; int64_t part_stride;
    const int32_t* hits_part; int32_t n_spans;
    const int32_t* value_off; const int32_t* value_pos; int32_t n_values;
    int32_t limit;
    int32_t* out_hits; int32_t* out_n_values_hit; int32_t* out_top_value; int32_t* out_top_count;
    int32_t* out_counts; int64_t count_stride;
};

// One workgroup per row.  A candidate is the key count << 32 | ~value: larger = earlier in (count desc, value asc); 0 = none.
// top[0 .. limit) holds the running first `limit` keys, descending; a tile of THREADS values joins it only when one of its keys
// beats top[limit - 1], by rank: every key counts the keys above it among top and the tile (keys are distinct).
__global__ __launch_bounds__(THREADS) void facet_merge_kernel(const FacetMergeArgs a) {
    constexpr int L = MSR_FACET_MAX_LIMIT;
    __shared__ uint64_t all[L + THREADS];                // [0, L): top, [L, L + THREADS): the tile's keys
    __shared__ uint64_t nxt[L];
    __shared__ int32_t red[WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = blockIdx.x;
    const uint16_t* part = a.part + r * a.part_stride;
    const int limit = a.limit;
    if (tid < L) all[tid] = 0;
    __syncthreads();
    int nz = 0;
    for (int64_t v0 = 0; v0 < a.n_values; v0 += THREADS) {
        const int64_t v = v0 + tid;
        uint64_t key = 0;
        if (v < a.n_values) {
            uint32_t c = 0;
            for (int32_t i = a.value_off[v]; i < a.value_off[v + 1]; ++i) c += part[a.value_pos[i]];
            if (a.out_counts) a.out_counts[r * a.count_stride + v] = (int32_t)c;
            if (c) {
                ++nz;
                key = ((uint64_t)c << 32) | (uint32_t)~(uint32_t)v;
            }
        }
        if (limit <= 0) continue;
        const uint64_t thr = all[limit - 1];
        if (!__syncthreads_or(key > thr)) continue;
        all[L + tid] = key;
        if (tid < L) nxt[tid] = 0;
        __syncthreads();
        for (int e = tid; e < L + THREADS; e += THREADS) {           // (thread tid: slot tid of the tile part, and of top if tid < L)
            const int slot = e < THREADS ? L + e : e - THREADS;
            const uint64_t k = all[slot];
            if (!k) continue;
            int rank = 0;
            for (int j = 0; j < L + THREADS; ++j) rank += all[j] > k;
            if (rank < limit) nxt[rank] = k;
        }
        __syncthreads();
        if (tid < L) all[tid] = nxt[tid];
        __syncthreads();
    }
    const int n_hit = block_sum(nz, lane, wave, red);
    int h = 0;
    for (int s = tid; s < a.n_spans; s += THREADS) h += a.hits_part[r * a.n_spans + s];
    const int hits = block_sum(h, lane, wave, red);
    if (tid == 0) {
        a.out_hits[r] = hits;
        a.out_n_values_hit[r] = n_hit;
    }
    if (tid < limit) {
        const uint64_t k = all[tid];
        a.out_top_value[r * limit + tid] = k ? (int32_t)~(uint32_t)k : -1;
        a.out_top_count[r * limit + tid] = (int32_t)(k >> 32);
    }
}

// ---- the bind's check (msr_bind_facet): *flag <- max(*flag, code) --------------------------------------------------------------
// The host has read T = span_off[n_spans] (0 <= T <= n_docs) and value_off[n_values] == T; the arrays hold n_docs, n_spans + 1,
// T, n_values + 1 and T elements, which the caller vouches for.  Kernel A reads only by its own index: the offsets and local[].
// 1 span_off does not start at 0 / descends / a span has more than min(SPAN, its documents) entries, 2 a local id at or past
// its span's entry count, 3 value_off does not start at 0 or descends
__global__ void facet_validate_offsets_kernel(const uint16_t* local, const int32_t* span_off, const int32_t* value_off,
                                              int64_t n_docs, int32_t n_spans, int32_t n_values, int32_t* flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    int code = 0;
    if (i == 0 && span_off[0] != 0) code = 1;
    if (i == 0 && value_off[0] != 0) code = 3;
    for (int64_t s = i; s < n_spans; s += step) {
        const int64_t c = (int64_t)span_off[s + 1] - span_off[s];
        if (c < 0 || c > min((int64_t)SPAN, n_docs - s * SPAN)) code = max(code, 1);
    }
    for (int64_t v = i; v < n_values; v += step)
        if (value_off[v + 1] < value_off[v]) code = max(code, 3);
    for (int64_t d = i; d < n_docs; d += step) {
        const int64_t s = d / SPAN;
        const uint32_t l = local[d];
        if (l != NO_VALUE && (int64_t)l >= (int64_t)span_off[s + 1] - span_off[s]) code = max(code, 2);
    }
    if (code) atomicMax(flag, code);
}

// Kernel B follows offsets into span_values and value_pos, so it runs only when kernel A found them sound (monotone from 0 to T:
// every range lies in [0, T)).  4 a span's values are out of range or not strictly ascending, 5 a value's positions are out of
// range, not strictly ascending, or name a slot that holds another value
__global__ void facet_validate_lists_kernel(const int32_t* span_off, const int32_t* span_values, const int32_t* value_off,
                                            const int32_t* value_pos, int32_t n_spans, int32_t n_values, int32_t T, int32_t* flag) {
    if (*flag) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    int code = 0;
    for (int64_t s = i; s < n_spans; s += step)
        for (int32_t p = span_off[s]; p < span_off[s + 1]; ++p) {
            const int32_t v = span_values[p];
            if (v < 0 || v >= n_values || (p > span_off[s] && span_values[p - 1] >= v)) code = max(code, 4);
        }
    for (int64_t v = i; v < n_values; v += step)
        for (int32_t p = value_off[v]; p < value_off[v + 1]; ++p) {
            const int32_t q = value_pos[p];
            if (q < 0 || q >= T || span_values[q] != v || (p > value_off[v] && value_pos[p - 1] >= q)) code = max(code, 5);
        }
    if (code) atomicMax(flag, code);
}

}  // namespace

hipError_t msr_facet_validate(const FacetTable& f, int64_t n_docs, int32_t* flag, hipStream_t stream) {
    const int32_t n_spans = (int32_t)span_count(n_docs);
    const int64_t n = std::max<int64_t>(std::max<int64_t>(n_docs, f.n_values), 1);
    const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(facet_validate_offsets_kernel, dim3(blocks), dim3(256), 0, stream, f.local, f.span_off, f.value_off, n_docs,
                       n_spans, f.n_values, flag);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    const int64_t m = std::max<int64_t>(std::max<int64_t>(n_spans, f.n_values), 1);
    const unsigned blocks_b = (unsigned)std::min<int64_t>((m + 255) / 256, 4096);
    hipLaunchKernelGGL(facet_validate_lists_kernel, dim3(blocks_b), dim3(256), 0, stream, f.span_off, f.span_values, f.value_off,
                       f.value_pos, n_spans, f.n_values, (int32_t)f.n_entries, flag);
    return hipGetLastError();
}

int64_t msr_facet_row_bytes(const FacetTable& f, int64_t n_docs) {
    return (2 * f.n_entries + 15) / 16 * 16 + 4 * span_count(n_docs);
}

hipError_t msr_facet_counts_run(const Bm25Index& ix, const FacetTable& f, int n_rows, const int32_t* any_off,
                                const int32_t* any_terms, const uint32_t* base_bits, int n_base, int64_t base_stride,
                                const int32_t* row_base, int limit, int32_t* out_hits, int32_t* out_n_values_hit,
                                int32_t* out_top_value, int32_t* out_top_count, int32_t* out_counts, int64_t count_stride,
                                void* scratch, hipStream_t stream) {
    const int32_t n_spans = (int32_t)span_count(ix.n_docs);
    const int64_t part_stride = (2 * f.n_entries + 15) / 16 * 8;             // uint16 elements: a row's slots, rounded up to 16 bytes
    uint16_t* part = static_cast<uint16_t*>(scratch);
    int32_t* hits_part = reinterpret_cast<int32_t*>(part + (int64_t)n_rows * part_stride);
    const FacetCountArgs a{ix.term_off, ix.post_doc, ix.heavy_id, ix.tile_off, ix.n_terms, ix.n_docs, ix.n_tiles, any_off, any_terms,
                           base_bits, n_base, base_stride, row_base, f.local, f.span_off, part, part_stride, hits_part, n_spans, 0};
    hipError_t err = launch_rows(facet_count_kernel, n_spans, THREADS, n_rows, a, stream);
    if (err != hipSuccess) return err;
    const FacetMergeArgs m{part, part_stride, hits_part, n_spans, f.value_off, f.value_pos, f.n_values, limit, out_hits,
                           out_n_values_hit, out_top_value, out_top_count, out_counts, count_stride};
    hipLaunchKernelGGL(facet_merge_kernel, dim3((unsigned)n_rows), dim3(THREADS), 0, stream, m);
    return hipGetLastError();
}
