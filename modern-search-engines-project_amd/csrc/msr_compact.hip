// Compaction of a CSR-by-term posting table (index update: documents removed from a built index).  The postings of the
// removed documents are dropped and the kept documents are renumbered densely; the order inside every term is kept.
//
// Input: term_off [n_terms + 1] / post_doc / post_tf (documents ascending inside a term) and keep [n_docs] (nonzero = the
// document stays).  The new index of a kept document is the number of kept documents before it, so the renumbering is
// strictly increasing by construction.  Output: out_term_off[t] = the kept postings before
// term_off[t]; out_doc = the renumbered documents of the kept postings, out_tf copied.
//
// The documents are described by 64-document blocks: a 64-bit ballot of keep per block and the kept documents before the
// block, 16 B per 64 documents (250 KB for 10^6 documents, resident in L2 next to the streams; a renumbering table of one
// int32 per document would be 4 MB and compete with them).  Document d is kept iff bit d & 63 of mask[d >> 6] is set, and
// its new index is pre[d >> 6] + popcount(mask[d >> 6] below that bit).  The postings are cut into fixed tiles of TILE,
// independent of how they spread over terms:
//   1. block_kernel     mask[b] = ballot(keep) of the 64 documents of block b, count = its popcount
//      check_kernel     term_off monotone from 0
//   2. count_kernel     one workgroup per tile: its kept count (16-byte loads of post_doc, the mask gathered); a document
//                       index outside [0, n_docs) raises the flag
//   3. exclusive scans  of the tile counts -> tile_off, of the block counts -> pre
//   4. write_kernel     one workgroup per tile: every lane holds a quad of consecutive postings per round; the kept ones
//                       are ranked inside the wave by three 64-bit ballots of the quad's kept count (bit b of the count,
//                       weighted 2^b) with mbcnt, across the waves and rounds of the tile by an LDS prefix of the wave
//                       totals.  The kept postings are packed in LDS in order and leave with 16-byte stores.  The same
//                       prefix gives out_term_off[t] for every term that starts inside the tile (binary search of term_off
//                       for the tile's term range); terms that start at the end (P) get the total.
// Everything the caller controls -- offsets, document indices, capacity -- is checked before anything is written.  No atomics
// on the data path: the output is the same every run.
//
// Offline like msr_build_postings: the entry point allocates its workspace and synchronises.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/msretr.h"
#include "msr_internal.h"

namespace {

constexpr int MT = 256;                  // threads per workgroup (4 waves of 64)
constexpr int ROUNDS = 2;                // quads of postings per thread
constexpr int QUADS = MT * ROUNDS;       // quads per tile
constexpr int TILE = 4 * QUADS;          // postings per workgroup
constexpr int WAVES = MT / 64;

// flag codes (atomicMin: the smallest reported wins; 0x7F7F7F7F = none)
enum { F_OFFSETS = 1, F_DOC = 2 };

__device__ __forceinline__ uint32_t lane_rank(uint64_t mask) {      // set bits of mask below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// first t in [0, n] with off[t] >= p
__device__ __forceinline__ int64_t lower_bound(const int64_t* off, int64_t n, int64_t p) {
    int64_t lo = 0, hi = n + 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] < p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// postings [i, i + 4) of a (-1 past P): one 16-byte load when VEC and the quad is whole
template <bool VEC>
__device__ __forceinline__ int4 load_quad(const int32_t* __restrict__ a, int64_t i, int64_t P) {
    if (VEC && i + 4 <= P) return *reinterpret_cast<const int4*>(a + i);
    return make_int4(i < P ? a[i] : -1, i + 1 < P ? a[i + 1] : -1, i + 2 < P ? a[i + 2] : -1, i + 3 < P ? a[i + 3] : -1);
}

__global__ __launch_bounds__(256) void check_kernel(const int64_t* __restrict__ off, int64_t n_terms, int32_t* __restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t <= n_terms; t += stride)
        if ((t == 0 && off[0] != 0) || (t < n_terms && off[t + 1] < off[t])) atomicMin(flag, F_OFFSETS);
}

// mask[b] = the kept documents of block b as bits, cnt[b] = how many
__global__ __launch_bounds__(256) void block_kernel(const uint8_t* __restrict__ keep, int64_t n_docs, uint64_t* __restrict__ mask,
                                                    int64_t* __restrict__ cnt) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t m = __ballot(d < n_docs && keep[d] != 0);
    if ((threadIdx.x & 63) == 0 && d < n_docs) {
        mask[d >> 6] = m;
        cnt[d >> 6] = __popcll(m);
    }
}

__device__ __forceinline__ bool kept(const uint64_t* __restrict__ mask, int32_t d) { return (mask[d >> 6] >> (d & 63)) & 1; }

// tile_cnt[k] <- kept postings of tile k
template <bool VEC>
__global__ __launch_bounds__(MT) void count_kernel(const int32_t* __restrict__ post_doc, int64_t P, const uint64_t* __restrict__ mask,
                                                   int64_t n_docs, int64_t* __restrict__ tile_cnt, int32_t* __restrict__ flag) {
    __shared__ int s_sum[WAVES];
    const int64_t p0 = (int64_t)blockIdx.x * TILE;
    int c = 0;
    bool bad = false;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const int64_t i = p0 + 4 * ((int64_t)r * MT + threadIdx.x);
        const int4 d = load_quad<VEC>(post_doc, i, P);
        const int32_t dd[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (i + e >= P) continue;
            if (dd[e] < 0 || dd[e] >= n_docs) { bad = true; continue; }
            c += kept(mask, dd[e]);
        }
    }
    if (bad) atomicMin(flag, F_DOC);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t s = 0;
        for (int w = 0; w < WAVES; ++w) s += s_sum[w];
        tile_cnt[blockIdx.x] = s;
    }
}

// the new index of document d, or -1 when d is removed (or d < 0: past P)
__device__ __forceinline__ int32_t renumber(const uint64_t* __restrict__ mask, const int64_t* __restrict__ pre, int32_t d) {
    if (d < 0) return -1;
    const uint64_t m = mask[d >> 6], below = m & ((1ull << (d & 63)) - 1);
    return (m >> (d & 63)) & 1 ? (int32_t)(pre[d >> 6] + __popcll(below)) : -1;
}

__global__ __launch_bounds__(256) void zero_off_kernel(int64_t* __restrict__ out, int64_t n) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) out[t] = 0;
}

template <bool VEC>
__global__ __launch_bounds__(MT) void write_kernel(const int64_t* __restrict__ term_off, int64_t n_terms, const int32_t* __restrict__ post_doc,
                                                   const int32_t* __restrict__ post_tf, int64_t P, const uint64_t* __restrict__ mask,
                                                   const int64_t* __restrict__ pre,
                                                   const int64_t* __restrict__ tile_off, int64_t* __restrict__ out_term_off,
                                                   int32_t* __restrict__ out_doc, int32_t* __restrict__ out_tf) {
    __shared__ __align__(16) int32_t s_doc[TILE + 4];   // the tile's kept postings, at (output position & 3) + rank:
    __shared__ __align__(16) int32_t s_tf[TILE + 4];    // LDS quads line up with the output's 16-byte quads
    __shared__ int32_t s_qpre[QUADS];                   // kept postings of the tile before each quad
    __shared__ uint8_t s_qbits[QUADS];                  // the quad's kept postings as bits
    __shared__ int32_t s_wsum[ROUNDS * WAVES];          // kept postings of each (round, wave)
    __shared__ int64_t s_trange[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t k = blockIdx.x, p0 = k * TILE;
    const int64_t o0 = tile_off[k];
    const int shift = (int)(o0 & 3);
    if (threadIdx.x < 2) {      // terms that start inside this tile: [lb(p0), lb(p0 + TILE)); the last tile also takes those at P
        const bool last = p0 + TILE >= P;
        s_trange[threadIdx.x] = threadIdx.x == 0 ? lower_bound(term_off, n_terms, p0)
                                                 : (last ? n_terms + 1 : lower_bound(term_off, n_terms, p0 + TILE));
    }
    int4 d[ROUNDS], f[ROUNDS];
    uint32_t bits[ROUNDS], rank[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const int64_t i = p0 + 4 * ((int64_t)r * MT + threadIdx.x);
        d[r] = load_quad<VEC>(post_doc, i, P);
        f[r] = load_quad<VEC>(post_tf, i, P);
    }
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        // renumber (past P: doc -1, not kept); bits of the quad, its count c in 0..4, ranked by three ballots
        d[r].x = renumber(mask, pre, d[r].x);
        d[r].y = renumber(mask, pre, d[r].y);
        d[r].z = renumber(mask, pre, d[r].z);
        d[r].w = renumber(mask, pre, d[r].w);
        bits[r] = (d[r].x >= 0) | (d[r].y >= 0) << 1 | (d[r].z >= 0) << 2 | (d[r].w >= 0) << 3;
        const uint32_t c = __popc(bits[r]);
        const uint64_t m0 = __ballot(c & 1), m1 = __ballot(c & 2), m2 = __ballot(c & 4);
        rank[r] = lane_rank(m0) + 2 * lane_rank(m1) + 4 * lane_rank(m2);
        if (lane == 0) s_wsum[r * WAVES + wave] = __popcll(m0) + 2 * __popcll(m1) + 4 * __popcll(m2);
    }
    __syncthreads();
    int tile_kept = 0;
#pragma unroll
    for (int j = 0; j < ROUNDS * WAVES; ++j) tile_kept += s_wsum[j];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        int pre = (int)rank[r];
        for (int j = 0; j < r * WAVES + wave; ++j) pre += s_wsum[j];
        const int q = r * MT + threadIdx.x;
        s_qpre[q] = pre;
        s_qbits[q] = (uint8_t)bits[r];
        int o = shift + pre;
        if (bits[r] & 1) { s_doc[o] = d[r].x; s_tf[o] = f[r].x; ++o; }
        if (bits[r] & 2) { s_doc[o] = d[r].y; s_tf[o] = f[r].y; ++o; }
        if (bits[r] & 4) { s_doc[o] = d[r].z; s_tf[o] = f[r].z; ++o; }
        if (bits[r] & 8) { s_doc[o] = d[r].w; s_tf[o] = f[r].w; }
    }
    __syncthreads();
    // the kept postings -> [o0, o0 + tile_kept): LDS slot i is output position o0 - shift + i
    const int n_slots = shift + tile_kept;
    int32_t* gd = out_doc + (o0 - shift);
    int32_t* gf = out_tf + (o0 - shift);
    for (int i = 4 * threadIdx.x; i < n_slots; i += 4 * MT) {
        if (VEC && i >= shift && i + 4 <= n_slots) {
            *reinterpret_cast<int4*>(gd + i) = *reinterpret_cast<const int4*>(s_doc + i);
            *reinterpret_cast<int4*>(gf + i) = *reinterpret_cast<const int4*>(s_tf + i);
        } else {
            for (int e = i; e < i + 4 && e < n_slots; ++e)
                if (e >= shift) { gd[e] = s_doc[e]; gf[e] = s_tf[e]; }
        }
    }
    // out_term_off of the terms that start inside this tile
    const int64_t t1 = s_trange[1];
    for (int64_t t = s_trange[0] + threadIdx.x; t < t1; t += MT) {
        const int64_t p = term_off[t];
        int64_t v = o0 + tile_kept;
        if (p < P) {
            const int r = (int)(p - p0), q = r >> 2;
            v = o0 + s_qpre[q] + __popc(s_qbits[q] & ((1u << (r & 3)) - 1u));
        }
        out_term_off[t] = v;
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

#define COMPACT_TRY(call)                                                                                    \
    do {                                                                                                     \
        hipError_t _e = (call);                                                                              \
        if (_e != hipSuccess) { rc = msr_fail_global(MSR_ERR_HIP, "%s: %s", #call, hipGetErrorString(_e)); goto done; } \
    } while (0)

extern "C" int msr_compact_postings(const int64_t* term_off, int64_t n_terms, const int32_t* post_doc, const int32_t* post_tf,
                                    const uint8_t* keep, int64_t n_docs, int64_t* out_term_off, int32_t* out_doc, int32_t* out_tf,
                                    int64_t capacity, int64_t* n_postings, void* stream) {
    if (!term_off || !out_term_off || !n_postings || n_terms < 0 || n_docs < 0 || n_docs >= (1ll << 31) || capacity < 0 ||
        (n_docs > 0 && !keep) || (capacity > 0 && (!out_doc || !out_tf)))
        return msr_fail_global(MSR_ERR_INVALID, "msr_compact_postings: bad argument");
    hipStream_t st = (hipStream_t)stream;
    int rc = MSR_OK;
    {   // handle-less entry point: run on the device that holds the caller's arrays
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, term_off) == hipSuccess && attr.type == hipMemoryTypeDevice) (void)hipSetDevice(attr.device);
        else (void)hipGetLastError();
    }
    int32_t* d_flag = nullptr;
    uint64_t* d_mask = nullptr;
    int64_t *d_bcnt = nullptr, *d_bpre = nullptr, *d_tcnt = nullptr, *d_toff = nullptr, *d_tmp = nullptr;
    int64_t P = 0, n_tiles = 0, n_blk = (n_docs + 63) / 64, n_tmp = 0, h_total = 0;
    int32_t h_flag = 0;
    bool vec = false;
    static const char* why[] = {"", "term_off is not a monotone offset array from 0", "a posting's document index is outside [0, n_docs)"};
    COMPACT_TRY(hipMemcpyAsync(&P, term_off + n_terms, 8, hipMemcpyDeviceToHost, st));
    COMPACT_TRY(hipStreamSynchronize(st));
    if (P < 0) { rc = msr_fail_global(MSR_ERR_INVALID, "msr_compact_postings: %s", why[F_OFFSETS]); goto done; }
    if (P > 0 && (!post_doc || !post_tf)) { rc = msr_fail_global(MSR_ERR_INVALID, "msr_compact_postings: null posting array"); goto done; }
    n_tiles = (P + TILE - 1) / TILE;
    n_tmp = exclusive_scan_tmp_words(std::max(n_blk, n_tiles));          // both scans share the scratch
    COMPACT_TRY(hipMalloc((void**)&d_flag, 4));
    COMPACT_TRY(hipMalloc((void**)&d_tmp, (size_t)(n_tmp + 1) * 8));      // + the total
    COMPACT_TRY(hipMalloc((void**)&d_tcnt, (size_t)std::max<int64_t>(n_tiles, 1) * 8));
    COMPACT_TRY(hipMalloc((void**)&d_toff, (size_t)std::max<int64_t>(n_tiles, 1) * 8));
    COMPACT_TRY(hipMalloc((void**)&d_mask, (size_t)std::max<int64_t>(n_blk, 1) * 8));
    COMPACT_TRY(hipMalloc((void**)&d_bcnt, (size_t)std::max<int64_t>(n_blk, 1) * 8));
    COMPACT_TRY(hipMalloc((void**)&d_bpre, (size_t)std::max<int64_t>(n_blk, 1) * 8));
    vec = aligned16(post_doc) && aligned16(post_tf) && aligned16(out_doc) && aligned16(out_tf);
    // ---- checks and counts: before anything is written ----
    COMPACT_TRY(hipMemsetAsync(d_flag, 0x7F, 4, st));
    if (n_docs > 0) {
        block_kernel<<<(unsigned)((n_docs + 255) / 256), 256, 0, st>>>(keep, n_docs, d_mask, d_bcnt);
        COMPACT_TRY(hipGetLastError());
    }
    check_kernel<<<(unsigned)std::min<int64_t>((n_terms + 256) / 256, 1024), 256, 0, st>>>(term_off, n_terms, d_flag);
    COMPACT_TRY(hipGetLastError());
    if (P > 0) {
        if (vec) count_kernel<true><<<(unsigned)n_tiles, MT, 0, st>>>(post_doc, P, d_mask, n_docs, d_tcnt, d_flag);
        else count_kernel<false><<<(unsigned)n_tiles, MT, 0, st>>>(post_doc, P, d_mask, n_docs, d_tcnt, d_flag);
        COMPACT_TRY(hipGetLastError());
    }
    COMPACT_TRY(exclusive_scan(d_tcnt, n_tiles, d_toff, d_tmp, d_tmp + n_tmp, st));
    COMPACT_TRY(hipMemcpyAsync(&h_flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    COMPACT_TRY(hipMemcpyAsync(&h_total, d_tmp + n_tmp, 8, hipMemcpyDeviceToHost, st));
    COMPACT_TRY(hipStreamSynchronize(st));
    if (h_flag >= 1 && h_flag <= 2) { rc = msr_fail_global(MSR_ERR_INVALID, "msr_compact_postings: %s", why[h_flag]); goto done; }
    *n_postings = h_total;
    if (h_total > capacity) {                        // capacity 0: a sizing call; the caller allocates and calls again
        rc = capacity > 0 ? msr_fail_global(MSR_ERR_INVALID, "msr_compact_postings: capacity %lld < %lld postings", (long long)capacity,
                                            (long long)h_total)
                          : MSR_OK;
        goto done;
    }
    // ---- the compaction ----
    if (P == 0) {
        zero_off_kernel<<<(unsigned)((n_terms + 1 + 255) / 256), 256, 0, st>>>(out_term_off, n_terms + 1);
        COMPACT_TRY(hipGetLastError());
    } else {
        COMPACT_TRY(exclusive_scan(d_bcnt, n_blk, d_bpre, d_tmp, nullptr, st));
        if (vec)
            write_kernel<true><<<(unsigned)n_tiles, MT, 0, st>>>(term_off, n_terms, post_doc, post_tf, P, d_mask, d_bpre, d_toff, out_term_off, out_doc, out_tf);
        else
            write_kernel<false><<<(unsigned)n_tiles, MT, 0, st>>>(term_off, n_terms, post_doc, post_tf, P, d_mask, d_bpre, d_toff, out_term_off, out_doc, out_tf);
        COMPACT_TRY(hipGetLastError());
    }
    COMPACT_TRY(hipStreamSynchronize(st));
done:
    (void)hipStreamSynchronize(st);
    for (void* q : {(void*)d_flag, (void*)d_mask, (void*)d_bcnt, (void*)d_bpre, (void*)d_tcnt, (void*)d_toff, (void*)d_tmp})
        if (q) (void)hipFree(q);
    return rc;
}
