// Merge of two CSR-by-term posting tables into one (the incremental half of BM25.build_index, indexer/bm25_indexer.py:252-344:
// the postings of newly indexed documents join those of the built index, both sides renumbered into the merged dense order).
//
// Inputs: A (the built index) and B (the new documents), each term_off [terms + 1] / doc / tf with documents strictly ascending
// inside a term, and a strictly increasing map from each side's dense index to the merged one (A's may be NULL = identity).
// Output: term_off[t] = a_off[min(t, a_terms)] + b_off[min(t, b_terms)]; inside a term the A and B segments merged by mapped
// document; post_doc holds the mapped index, post_tf is copied.
//
// Seen globally, A and B are two sequences sorted by (term, mapped document), and the merged table is their merge: output
// position p takes ia(p) postings of A and p - ia(p) of B, both nondecreasing in p.  So the work is a merge path over the
// whole output range, independent of how the postings spread over terms:
//   1. check_kernel      offsets monotone from 0, maps in range and strictly increasing (before anything is written)
//   2. shared_kernel     for every B document, the A document with the same merged index (-1: none); a B posting can only
//      clash_kernel      clash with A inside its term when its document has one: those postings (none in the common case,
//                        where B holds only new documents) look their A twin up by binary search in the term's A segment
//   3. term_off_kernel   the merged offsets
//   4. partition_kernel  per tile boundary p = k * TILE: its term by binary search of the merged offsets, then the split
//                        ia(p) by a diagonal search on the mapped keys of that term's A and B segments
//   5. merge_kernel      one workgroup per tile of TILE outputs: its A range [ia0, ia1] and B range [ib0, ib1] (+ one
//                        look-ahead posting each) -> mapped keys and tf in LDS (16-byte loads); each thread finds its own split
//                        inside the tile the same way (term search limited to the tile's terms, diagonal search limited to the
//                        tile's ranges: LDS only), merges ITEMS outputs in registers -- crossing term boundaries as it goes --
//                        and writes them with 16-byte stores.  No atomics on the data path: the output is the same every run.
// A posting-level malformation (a document index outside its side, a descent inside a term) is caught inside the merge
// itself: the call then returns MSR_ERR_INVALID after the output was written (its contents unspecified).  Everything the
// caller controls cheaply -- offsets, maps, clashes, capacity -- is rejected before any output is written.
//
// Offline like msr_build_postings: the entry point allocates its workspace and synchronises.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/msretr.h"
#include "msr_internal.h"

namespace {

constexpr int MT = 256;                  // threads per workgroup (4 waves of 64)
constexpr int ITEMS = 8;                 // consecutive outputs per thread
constexpr int TILE = MT * ITEMS;         // outputs per workgroup
constexpr int32_t KEY_NONE = INT32_MAX;  // key of a posting whose document is malformed (never merged as valid)

// flag codes (atomicMin: the smallest reported wins; 0x7F7F7F7F = none)
enum { F_OFFSETS = 1, F_MAP = 2, F_CLASH = 3, F_DOC = 4, F_ORDER = 5 };

struct Side {
    const int64_t* off;
    int64_t terms;
    const int32_t* doc;
    const int32_t* tf;
    const int32_t* map;                  // NULL: identity
    int64_t docs;
    int64_t n_post;                      // off[terms]
};

__device__ __forceinline__ int64_t seg(const Side& s, int64_t t) { return s.off[t < s.terms ? t : s.terms]; }

__device__ __forceinline__ int32_t key_of(const Side& s, int32_t d, int32_t* flag) {
    if (d < 0 || d >= s.docs) {
        atomicMin(flag, F_DOC);
        return KEY_NONE;
    }
    return s.map ? s.map[d] : d;
}

// largest t in [lo, hi) with off[t] <= p (off[lo] <= p)
__device__ __forceinline__ int64_t term_of(const int64_t* off, int64_t lo, int64_t hi, int64_t p) {
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void check_kernel(Side a, Side b, int64_t n_docs, int32_t* __restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t t = g; t <= a.terms; t += stride)
        if ((t == 0 && a.off[0] != 0) || (t < a.terms && a.off[t + 1] < a.off[t])) atomicMin(flag, F_OFFSETS);
    for (int64_t t = g; t <= b.terms; t += stride)
        if ((t == 0 && b.off[0] != 0) || (t < b.terms && b.off[t + 1] < b.off[t])) atomicMin(flag, F_OFFSETS);
    if (a.map)
        for (int64_t d = g; d < a.docs; d += stride) {
            const int32_t m = a.map[d];
            if (m < 0 || m >= n_docs || (d > 0 && a.map[d - 1] >= m)) atomicMin(flag, F_MAP);
        }
    for (int64_t d = g; d < b.docs; d += stride) {
        const int32_t m = b.map[d];
        if (m < 0 || m >= n_docs || (d > 0 && b.map[d - 1] >= m)) atomicMin(flag, F_MAP);
    }
}

// b_in_a[y] = the A document whose merged index is b.map[y], or -1; *any <- 1 when there is one
__global__ __launch_bounds__(256) void shared_kernel(Side a, Side b, int32_t* __restrict__ b_in_a, int32_t* __restrict__ any) {
    const int64_t y = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (y >= b.docs) return;
    const int32_t m = b.map[y];
    int64_t x = -1;
    if (!a.map) {
        x = m < a.docs ? m : -1;
    } else {
        int64_t lo = 0, hi = a.docs;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.map[mid] < m) lo = mid + 1; else hi = mid;
        }
        if (lo < a.docs && a.map[lo] == m) x = lo;
    }
    b_in_a[y] = (int32_t)x;
    if (x >= 0) *any = 1;                       // (every writer stores the same value)
}

__global__ __launch_bounds__(256) void clash_kernel(Side a, Side b, const int32_t* __restrict__ b_in_a, int32_t* __restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < b.n_post; p += stride) {
        const int32_t y = b.doc[p];
        if (y < 0 || y >= b.docs) continue;     // (reported by the merge)
        const int32_t x = b_in_a[y];
        if (x < 0) continue;
        const int64_t t = term_of(b.off, 0, b.terms, p);
        if (t >= a.terms) continue;
        int64_t lo = a.off[t], hi = a.off[t + 1];
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.doc[mid] < x) lo = mid + 1; else hi = mid;
        }
        if (lo < a.off[t + 1] && a.doc[lo] == x) atomicMin(flag, F_CLASH);
    }
}

__global__ __launch_bounds__(256) void term_off_kernel(Side a, Side b, int64_t n_terms, int64_t* __restrict__ term_off) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t <= n_terms) term_off[t] = seg(a, t) + seg(b, t);
}

// tile boundary k (p = min(k * TILE, P)): tile_ia[k] = postings of A among the first p outputs, tile_t[k] = term of output p
// (of output P - 1 at the end)
__global__ __launch_bounds__(256) void partition_kernel(Side a, Side b, const int64_t* __restrict__ term_off, int64_t n_terms,
                                                        int64_t n_tiles, int64_t* __restrict__ tile_ia, int64_t* __restrict__ tile_t,
                                                        int32_t* __restrict__ flag) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > n_tiles) return;
    const int64_t P = a.n_post + b.n_post;
    const int64_t p = std::min<int64_t>(k * TILE, P);
    if (p == P) {
        tile_ia[k] = a.n_post;
        tile_t[k] = term_of(term_off, 0, n_terms, P - 1);
        return;
    }
    const int64_t t = term_of(term_off, 0, n_terms, p);
    const int64_t r = p - term_off[t];
    const int64_t as = seg(a, t), na = seg(a, t + 1) - as, bs = seg(b, t), nb = seg(b, t + 1) - bs;
    int64_t lo = std::max<int64_t>(0, r - nb), hi = std::min(r, na);
    while (lo < hi) {                             // merge path: ties go to A
        const int64_t mid = (lo + hi) >> 1;
        if (key_of(a, a.doc[as + mid], flag) <= key_of(b, b.doc[bs + r - 1 - mid], flag)) lo = mid + 1; else hi = mid;
    }
    tile_ia[k] = as + lo;
    tile_t[k] = t;
}

// [start, start + len) of one side -> mapped keys / tf at s_key[dst ..] / s_tf[dst ..]
template <bool VEC>
__device__ __forceinline__ void load_range(const Side& s, int64_t start, int64_t len, int dst, int32_t* s_key, int32_t* s_tf,
                                           int32_t* flag) {
    if (VEC) {                                    // 16-byte loads from the aligned quad at or below start
        for (int64_t j = (start & ~(int64_t)3) + 4 * (int64_t)threadIdx.x; j < start + len; j += 4 * MT) {
            if (j >= start && j + 4 <= start + len) {
                const int4 d = *reinterpret_cast<const int4*>(s.doc + j);
                const int4 f = *reinterpret_cast<const int4*>(s.tf + j);
                const int o = dst + (int)(j - start);
                s_key[o] = key_of(s, d.x, flag); s_key[o + 1] = key_of(s, d.y, flag);
                s_key[o + 2] = key_of(s, d.z, flag); s_key[o + 3] = key_of(s, d.w, flag);
                s_tf[o] = f.x; s_tf[o + 1] = f.y; s_tf[o + 2] = f.z; s_tf[o + 3] = f.w;
            } else {
                for (int e = 0; e < 4; ++e)
                    if (j + e >= start && j + e < start + len) {
                        const int o = dst + (int)(j + e - start);
                        s_key[o] = key_of(s, s.doc[j + e], flag);
                        s_tf[o] = s.tf[j + e];
                    }
            }
        }
    } else {
        for (int64_t j = threadIdx.x; j < len; j += MT) {
            s_key[dst + j] = key_of(s, s.doc[start + j], flag);
            s_tf[dst + j] = s.tf[start + j];
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(MT) void merge_kernel(Side a, Side b, const int64_t* __restrict__ term_off,
                                                   const int64_t* __restrict__ tile_ia, const int64_t* __restrict__ tile_t,
                                                   int32_t* __restrict__ post_doc, int32_t* __restrict__ post_tf,
                                                   int32_t* __restrict__ flag) {
    __shared__ int32_t s_key[TILE + 2];
    __shared__ int32_t s_tf[TILE + 2];
    const int64_t P = a.n_post + b.n_post;
    const int64_t p0 = (int64_t)blockIdx.x * TILE, p1 = std::min<int64_t>(P, p0 + TILE);
    const int64_t ia0 = tile_ia[blockIdx.x], ia1 = tile_ia[blockIdx.x + 1];
    const int64_t ib0 = p0 - ia0, ib1 = p1 - ia1;
    const int64_t t0 = tile_t[blockIdx.x], t1 = tile_t[blockIdx.x + 1];
    // splits that are not monotone come only from postings out of order (the partition's searches assume the order): the
    // LDS ranges below would not fit
    if (ia0 < 0 || ib0 < 0 || ia1 < ia0 || ib1 < ib0 || ia1 > a.n_post || ib1 > b.n_post) {
        if (threadIdx.x == 0) atomicMin(flag, F_ORDER);
        return;
    }
    // the tile's postings of each side plus one look-ahead posting (order and clash checks at the tile's end)
    const int la = (int)(std::min(ia1 + 1, a.n_post) - ia0), lb = (int)(std::min(ib1 + 1, b.n_post) - ib0);
    load_range<VEC>(a, ia0, la, 0, s_key, s_tf, flag);
    load_range<VEC>(b, ib0, lb, la, s_key, s_tf, flag);
    __syncthreads();
    // LDS slot of A posting i / B posting j; -1 outside the loaded ranges (only reachable with malformed input)
    auto slot_a = [&](int64_t i) { return i >= ia0 && i < ia0 + la ? (int)(i - ia0) : -1; };
    auto slot_b = [&](int64_t j) { return j >= ib0 && j < ib0 + lb ? la + (int)(j - ib0) : -1; };
    auto key_at = [&](int s) {
        if (s < 0) { atomicMin(flag, F_ORDER); return KEY_NONE; }
        return s_key[s];
    };
    const int64_t p = p0 + (int64_t)threadIdx.x * ITEMS;
    if (p >= p1) return;
    int64_t t = term_of(term_off, t0, t1 + 1, p);
    int64_t ae = seg(a, t + 1), be = seg(b, t + 1), tn = term_off[t + 1];
    int64_t ia, ib;
    {   // this thread's split: diagonal search inside the term, limited to the tile's ranges
        const int64_t r = p - term_off[t], as = seg(a, t), bs = seg(b, t);
        int64_t lo = std::max(std::max<int64_t>(0, r - (be - bs)), std::max(ia0 - as, r - (ib1 - bs)));
        int64_t hi = std::min(std::min(r, ae - as), std::min(ia1 - as, r - (ib0 - bs)));
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (key_at(slot_a(as + mid)) <= key_at(slot_b(bs + r - 1 - mid))) lo = mid + 1; else hi = mid;
        }
        ia = as + lo;
        ib = bs + (r - lo);
    }
    int32_t od[ITEMS], of[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const int64_t q = p + it;
        od[it] = of[it] = 0;
        if (q >= p1) continue;
        if (q >= tn) {                            // next (non-empty) term
            do { ++t; tn = term_off[t + 1]; } while (tn <= q);
            ae = seg(a, t + 1);
            be = seg(b, t + 1);
        }
        const bool ha = ia < ae, hb = ib < be;
        const int sa = ha ? slot_a(ia) : -1, sb = hb ? slot_b(ib) : -1;
        const int32_t ka = ha ? key_at(sa) : KEY_NONE, kb = hb ? key_at(sb) : KEY_NONE;
        if (ha && hb && ka == kb) atomicMin(flag, F_CLASH);
        if (ha && (!hb || ka <= kb)) {
            od[it] = ka; of[it] = s_tf[sa < 0 ? 0 : sa];
            if (ia + 1 < ae && key_at(slot_a(ia + 1)) <= ka) atomicMin(flag, F_ORDER);
            ++ia;
        } else {
            od[it] = kb; of[it] = s_tf[sb < 0 ? 0 : sb];
            if (ib + 1 < be && key_at(slot_b(ib + 1)) <= kb) atomicMin(flag, F_ORDER);
            ++ib;
        }
    }
    if (VEC && p + ITEMS <= p1) {
        int4* d4 = reinterpret_cast<int4*>(post_doc + p);
        int4* f4 = reinterpret_cast<int4*>(post_tf + p);
        d4[0] = make_int4(od[0], od[1], od[2], od[3]); d4[1] = make_int4(od[4], od[5], od[6], od[7]);
        f4[0] = make_int4(of[0], of[1], of[2], of[3]); f4[1] = make_int4(of[4], of[5], of[6], of[7]);
    } else {
#pragma unroll
        for (int it = 0; it < ITEMS; ++it)
            if (p + it < p1) { post_doc[p + it] = od[it]; post_tf[p + it] = of[it]; }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

#define MERGE_TRY(call)                                                                                      \
    do {                                                                                                     \
        hipError_t _e = (call);                                                                              \
        if (_e != hipSuccess) { rc = msr_fail_global(MSR_ERR_HIP, "%s: %s", #call, hipGetErrorString(_e)); goto done; } \
    } while (0)

extern "C" int msr_merge_postings(const int64_t* a_term_off, int64_t a_terms, const int32_t* a_doc, const int32_t* a_tf,
                                  const int32_t* a_map, int64_t a_docs, const int64_t* b_term_off, int64_t b_terms,
                                  const int32_t* b_doc, const int32_t* b_tf, const int32_t* b_map, int64_t b_docs,
                                  int64_t n_terms, int64_t n_docs, int64_t* term_off, int32_t* post_doc, int32_t* post_tf,
                                  int64_t capacity, void* stream) {
    if (!a_term_off || !b_term_off || !term_off || a_terms < 0 || b_terms < 0 || a_docs < 0 || b_docs < 0 || capacity < 0 ||
        n_terms < std::max(a_terms, b_terms) || n_docs < 0 || n_docs >= (1ll << 31) || (b_docs > 0 && !b_map) ||
        (!a_map && a_docs > n_docs))
        return msr_fail_global(MSR_ERR_INVALID, "msr_merge_postings: bad argument");
    hipStream_t st = (hipStream_t)stream;
    int rc = MSR_OK;
    {   // handle-less entry point: run on the device that holds the caller's arrays
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, term_off) == hipSuccess && attr.type == hipMemoryTypeDevice) (void)hipSetDevice(attr.device);
        else (void)hipGetLastError();
    }
    int32_t* d_flag = nullptr;                     // [0] flag, [1] any shared document, [2 ..] b_in_a
    int64_t *d_tile_ia = nullptr, *d_tile_t = nullptr;
    int64_t Pa = 0, Pb = 0, P = 0, n_tiles = 0;
    int32_t h_flag[2] = {0, 0};
    Side A{a_term_off, a_terms, a_doc, a_tf, a_map, a_docs, 0}, B{b_term_off, b_terms, b_doc, b_tf, b_map, b_docs, 0};
    static const char* why[] = {"", "a term_off is not a monotone offset array from 0", "a map is out of [0, n_docs) or not strictly increasing",
                                "the same merged document has postings of one term on both sides",
                                "a posting's document index is outside its side's documents",
                                "documents are not strictly ascending inside a posting list"};
    MERGE_TRY(hipMemcpyAsync(&Pa, a_term_off + a_terms, 8, hipMemcpyDeviceToHost, st));
    MERGE_TRY(hipMemcpyAsync(&Pb, b_term_off + b_terms, 8, hipMemcpyDeviceToHost, st));
    MERGE_TRY(hipStreamSynchronize(st));
    if (Pa < 0 || Pb < 0) { rc = msr_fail_global(MSR_ERR_INVALID, "msr_merge_postings: %s", why[F_OFFSETS]); goto done; }
    P = Pa + Pb;
    if (P > capacity) {
        rc = msr_fail_global(MSR_ERR_INVALID, "msr_merge_postings: capacity %lld < %lld postings", (long long)capacity, (long long)P);
        goto done;
    }
    if ((Pa > 0 && (!a_doc || !a_tf)) || (Pb > 0 && (!b_doc || !b_tf)) || (P > 0 && (!post_doc || !post_tf))) {
        rc = msr_fail_global(MSR_ERR_INVALID, "msr_merge_postings: null posting array");
        goto done;
    }
    A.n_post = Pa;
    B.n_post = Pb;
    n_tiles = (P + TILE - 1) / TILE;
    MERGE_TRY(hipMalloc((void**)&d_flag, (size_t)(2 + b_docs) * 4));
    MERGE_TRY(hipMalloc((void**)&d_tile_ia, (size_t)(n_tiles + 1) * 8));
    MERGE_TRY(hipMalloc((void**)&d_tile_t, (size_t)(n_tiles + 1) * 8));
    // ---- checks that need no posting: before anything is written ----
    MERGE_TRY(hipMemsetAsync(d_flag, 0x7F, 4, st));
    MERGE_TRY(hipMemsetAsync(d_flag + 1, 0, 4, st));
    check_kernel<<<1024, 256, 0, st>>>(A, B, n_docs, d_flag);
    MERGE_TRY(hipGetLastError());
    MERGE_TRY(hipMemcpyAsync(h_flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    MERGE_TRY(hipStreamSynchronize(st));
    if (h_flag[0] >= 1 && h_flag[0] <= 5) { rc = msr_fail_global(MSR_ERR_INVALID, "msr_merge_postings: %s", why[h_flag[0]]); goto done; }
    if (b_docs > 0) {
        shared_kernel<<<(unsigned)((b_docs + 255) / 256), 256, 0, st>>>(A, B, d_flag + 2, d_flag + 1);
        MERGE_TRY(hipGetLastError());
        MERGE_TRY(hipMemcpyAsync(h_flag, d_flag, 8, hipMemcpyDeviceToHost, st));
        MERGE_TRY(hipStreamSynchronize(st));
        if (h_flag[1] && Pb > 0 && Pa > 0) {       // documents on both sides: their postings must not share a term
            clash_kernel<<<(unsigned)std::min<int64_t>((Pb + 255) / 256, 4096), 256, 0, st>>>(A, B, d_flag + 2, d_flag);
            MERGE_TRY(hipGetLastError());
            MERGE_TRY(hipMemcpyAsync(h_flag, d_flag, 4, hipMemcpyDeviceToHost, st));
            MERGE_TRY(hipStreamSynchronize(st));
            if (h_flag[0] >= 1 && h_flag[0] <= 5) { rc = msr_fail_global(MSR_ERR_INVALID, "msr_merge_postings: %s", why[h_flag[0]]); goto done; }
        }
    }
    // ---- the merge ----
    term_off_kernel<<<(unsigned)((n_terms + 1 + 255) / 256), 256, 0, st>>>(A, B, n_terms, term_off);
    MERGE_TRY(hipGetLastError());
    if (P > 0) {
        partition_kernel<<<(unsigned)((n_tiles + 1 + 255) / 256), 256, 0, st>>>(A, B, term_off, n_terms, n_tiles, d_tile_ia, d_tile_t, d_flag);
        MERGE_TRY(hipGetLastError());
        if (aligned16(a_doc) && aligned16(a_tf) && aligned16(b_doc) && aligned16(b_tf) && aligned16(post_doc) && aligned16(post_tf))
            merge_kernel<true><<<(unsigned)n_tiles, MT, 0, st>>>(A, B, term_off, d_tile_ia, d_tile_t, post_doc, post_tf, d_flag);
        else
            merge_kernel<false><<<(unsigned)n_tiles, MT, 0, st>>>(A, B, term_off, d_tile_ia, d_tile_t, post_doc, post_tf, d_flag);
        MERGE_TRY(hipGetLastError());
    }
    MERGE_TRY(hipMemcpyAsync(h_flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    MERGE_TRY(hipStreamSynchronize(st));
    if (h_flag[0] >= 1 && h_flag[0] <= 5) rc = msr_fail_global(MSR_ERR_INVALID, "msr_merge_postings: malformed postings: %s", why[h_flag[0]]);
done:
    (void)hipStreamSynchronize(st);
    for (void* q : {(void*)d_flag, (void*)d_tile_ia, (void*)d_tile_t})
        if (q) (void)hipFree(q);
    return rc;
}
