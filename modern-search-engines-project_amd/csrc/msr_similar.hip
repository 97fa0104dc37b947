// K9: "documents like these" -- bound rows back into query images (msr_gather_rows) and the per-group merge of per-row dense
// top-k lists (msr_dense_topk_grouped).  The per-row lists come from msr_dense_topk / msr_dense_topk_within unchanged; this
// file holds the kernels around them.
//
// Merge, one workgroup of 256 threads per group g (rows [r0, r1), exclusions E_g, need = k + |E_g| entries per row):
//   1. tau   = max over the group's rows with at least `need` entries of their need-th score (-inf: none).  Every document
//              of the true top k reaches tau, so entries below max(tau, min_score) and entries past depth
//              `need` of a row are never looked at again.
//   2. count the surviving entries (M); M <= MERGE_CAP: the records live in LDS, else in the group's slice of a global scratch
//      (2 x rows x kk records: the power-of-two padding of M <= rows x need fits).
//   3. records (doc << 32 | ~ord(score), row, chunk) -> sort ascending: per document its best score first, the lowest row
//      among equal scores first.  Keys are distinct (a row lists a document once), so the result does not depend on the order
//      in which the threads placed the records.
//   4. drop all but the first record of a document, and the excluded documents (binary search of each in the sorted records)
//   5. rewrite the kept records as (ord(score) << 32 | ~doc) and sort descending: (score desc, doc asc); the first k are the
//      group's result.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msr_common.h"
#include "msr_internal.h"
#include "msr_sort.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int KSTEPS = MSR_DIM / 16;     // float4 blocks of a 16-row group in the interleaved layout (msr_dense.hip)
constexpr int MT = 256;                  // threads of the merge workgroup
constexpr int MERGE_CAP = 4096;          // records in LDS: 4096 x 16 B = 64 KiB, two workgroups per CU
constexpr uint32_t DROP = 0x80000000u;   // row field flag: record dropped (rows < 2^31)

__global__ __launch_bounds__(256) void check_range_kernel(const int32_t* __restrict__ v, int64_t n, int64_t hi,
                                                          int32_t* __restrict__ flag) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int32_t x = v[i];
        if (x < 0 || x >= hi) *flag = 1;                      // (every writer stores the same value)
    }
}

// one wave per output row: 192 float4 = 3 per lane; layout 1 reads the 16-row interleaved image of msr_interleave_rows
template <int LAYOUT>
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ emb, const int32_t* __restrict__ rows, int n,
                                                          float* __restrict__ out) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    const int64_t r = rows[i];
    const f32x4* src = (const f32x4*)emb;
    f32x4* dst = (f32x4*)(out + (int64_t)i * MSR_DIM);
#pragma unroll
    for (int it = 0; it < 3; ++it) {
        const int v = lane + 64 * it;                         // float4 v of the row: elements 4 v .. 4 v + 3
        int64_t s;
        if (LAYOUT == 0) {
            s = r * (MSR_DIM / 4) + v;
        } else {
            const int t = v >> 2, g = v & 3;                  // elements 16 t + 4 g ..: lane 16 g + (r & 15) of block (group, t)
            s = ((r >> 4) * KSTEPS + t) * 64 + 16 * g + (r & 15);
        }
        dst[v] = src[s];
    }
}

// row_set[r] = g_set[g] for the rows of group g
__global__ __launch_bounds__(256) void row_set_kernel(const int32_t* __restrict__ group_off, const int32_t* __restrict__ g_set,
                                                      int32_t* __restrict__ row_set) {
    const int g = blockIdx.x;
    const int r0 = group_off[g], r1 = group_off[g + 1];
    const int32_t s = g_set[g];
    for (int r = r0 + threadIdx.x; r < r1; r += 256) row_set[r] = s;
}

// bitonic network over GLOBAL records (the overflow path): msr_sort::bitonic_sort's compare-exchanges, a workgroup barrier after
// every stage (its in-wave shortcut orders LDS accesses only)
__device__ void bitonic_sort_global(uint64_t* khi, uint32_t* klo, uint32_t* val, int64_t P, bool ascending) {
    for (int64_t kk = 2; kk <= P; kk <<= 1) {
        for (int64_t j = kk >> 1; j > 0; j >>= 1) {
            for (int64_t idx = threadIdx.x; idx < (P >> 1); idx += MT) {
                const int64_t i = ((idx & ~(j - 1)) << 1) | (idx & (j - 1));
                const int64_t p = i | j;
                const bool want_desc = ((i & kk) == 0) != ascending;
                const uint64_t ah = khi[i], bh = khi[p];
                const uint32_t al = klo[i], bl = klo[p];
                const bool a_lt_b = ah < bh || (ah == bh && al < bl);
                const bool b_lt_a = bh < ah || (bh == ah && bl < al);
                if (want_desc ? a_lt_b : b_lt_a) {
                    khi[i] = bh; klo[i] = bl; khi[p] = ah; klo[p] = al;
                    const uint32_t t = val[i]; val[i] = val[p]; val[p] = t;
                }
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ float block_max(float v, float* red) {
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    return v;
}

__device__ __forceinline__ int block_sum(int v, int* red) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return v;
}

__global__ __launch_bounds__(MT) void grouped_merge_kernel(GroupedMergeArgs a) {
    __shared__ uint64_t s_hi[MERGE_CAP];
    __shared__ uint32_t s_lo[MERGE_CAP];
    __shared__ uint32_t s_val[MERGE_CAP];
    __shared__ float red_f[MT / 64];
    __shared__ int red_i[MT / 64];
    __shared__ int s_cnt;
    const int g = blockIdx.x, tid = threadIdx.x;
    const int r0 = a.group_off[g], r1 = a.group_off[g + 1];
    const int e0 = a.excl_off[g], e1 = a.excl_off[g + 1];
    const int need = a.k + (e1 - e0);
    const int64_t kk = a.kk;

    // 1. the filter threshold
    float tau = -__builtin_inff();
    for (int r = r0 + tid; r < r1; r += MT)
        if (a.l_n[r] >= need) tau = fmaxf(tau, a.l_score[r * kk + need - 1]);
    tau = block_max(tau, red_f);
    const float thr = fmaxf(tau, a.min_score);

    // 2. survivors
    const int64_t total = (int64_t)(r1 - r0) * need;
    int cnt = 0;
    for (int64_t i = tid; i < total; i += MT) {
        const int r = r0 + (int)(i / need), j = (int)(i % need);
        if (j < a.l_n[r] && a.l_score[r * kk + j] >= thr) ++cnt;
    }
    const int M = block_sum(cnt, red_i);
    int64_t P = 2;
    while (P < M) P <<= 1;
    const bool lds = M <= MERGE_CAP;
    uint64_t* hi = lds ? s_hi : a.g_hi + 2 * (int64_t)r0 * kk;
    uint32_t* lo = lds ? s_lo : a.g_lo + 2 * (int64_t)r0 * kk;
    uint32_t* val = lds ? s_val : a.g_val + 2 * (int64_t)r0 * kk;

    // 3. records by (doc asc, score desc, row asc)
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    for (int64_t i = tid; i < total; i += MT) {
        const int r = r0 + (int)(i / need), j = (int)(i % need);
        if (j >= a.l_n[r]) continue;
        const float s = a.l_score[r * kk + j];
        if (!(s >= thr)) continue;
        const int pos = atomicAdd(&s_cnt, 1);
        hi[pos] = ((uint64_t)(uint32_t)a.l_doc[r * kk + j] << 32) | (uint32_t)~msr_ord32(s);
        lo[pos] = (uint32_t)r;
        val[pos] = (uint32_t)a.l_chunk[r * kk + j];
    }
    for (int64_t i = M + tid; i < P; i += MT) { hi[i] = ~0ull; lo[i] = ~0u; val[i] = 0; }
    __syncthreads();
    if (lds) msr_sort::bitonic_sort<MT, true>(hi, lo, val, (int)P, true);
    else bitonic_sort_global(hi, lo, val, P, true);

    // 4. first record of each document; excluded documents out
    for (int i = tid; i < M; i += MT)
        if (i > 0 && (hi[i - 1] >> 32) == (hi[i] >> 32)) lo[i] |= DROP;
    __syncthreads();
    for (int x = e0 + tid; x < e1; x += MT) {
        const uint32_t d = (uint32_t)a.excl_doc[x];
        int lo_i = 0, hi_i = M;                               // first record whose document is >= d
        while (lo_i < hi_i) {
            const int mid = (lo_i + hi_i) >> 1;
            if ((uint32_t)(hi[mid] >> 32) < d) lo_i = mid + 1; else hi_i = mid;
        }
        if (lo_i < M && (uint32_t)(hi[lo_i] >> 32) == d) lo[lo_i] |= DROP;   // (repeated exclusions store the same value)
    }
    __syncthreads();

    // 5. kept records by (score desc, doc asc)
    int kept = 0;
    for (int64_t i = tid; i < P; i += MT) {
        if (i >= M || (lo[i] & DROP)) { hi[i] = 0; lo[i] = 0; continue; }
        const uint32_t doc = (uint32_t)(hi[i] >> 32), ord = ~(uint32_t)hi[i];
        hi[i] = ((uint64_t)ord << 32) | (uint32_t)~doc;
        ++kept;
    }
    kept = block_sum(kept, red_i);                            // (its barriers also end the rewrite)
    if (lds) msr_sort::bitonic_sort<MT, true>(hi, lo, val, (int)P, false);
    else bitonic_sort_global(hi, lo, val, P, false);

    const int n_out = kept < a.k ? kept : a.k;
    const int64_t o = (int64_t)g * a.k;
    for (int j = tid; j < a.k; j += MT) {
        if (j < n_out) {
            a.out_doc[o + j] = (int32_t)~(uint32_t)hi[j];
            a.out_score[o + j] = msr_unord32((uint32_t)(hi[j] >> 32));
            a.out_chunk[o + j] = (int32_t)val[j];
            a.out_src[o + j] = (int32_t)lo[j];
        } else {
            a.out_doc[o + j] = -1;
            a.out_score[o + j] = -__builtin_inff();
            a.out_chunk[o + j] = -1;
            a.out_src[o + j] = -1;
        }
    }
    if (tid == 0) a.out_n[g] = n_out;
}

}  // namespace

hipError_t msr_check_range(const int32_t* v, int64_t n, int64_t hi, int32_t* flag, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const int64_t blocks = (n + 255) / 256;
    check_range_kernel<<<(unsigned)(blocks < 1024 ? blocks : 1024), 256, 0, stream>>>(v, n, hi, flag);
    return hipGetLastError();
}

hipError_t msr_gather_rows_run(const DenseIndex& ix, const int32_t* rows, int n, float* out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((n + 3) / 4);
    if (ix.layout == 1) gather_rows_kernel<1><<<grid, 256, 0, stream>>>(ix.emb, rows, n, out);
    else gather_rows_kernel<0><<<grid, 256, 0, stream>>>(ix.emb, rows, n, out);
    return hipGetLastError();
}

hipError_t msr_group_row_sets(const int32_t* group_off, int n_groups, const int32_t* g_set, int32_t* row_set, hipStream_t stream) {
    if (n_groups <= 0) return hipSuccess;
    row_set_kernel<<<n_groups, 256, 0, stream>>>(group_off, g_set, row_set);
    return hipGetLastError();
}

hipError_t msr_grouped_merge(const GroupedMergeArgs& a, int n_groups, hipStream_t stream) {
    if (n_groups <= 0) return hipSuccess;
    grouped_merge_kernel<<<n_groups, MT, 0, stream>>>(a);
    return hipGetLastError();
}
