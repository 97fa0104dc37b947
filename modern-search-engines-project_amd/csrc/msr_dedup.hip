// K18: near-duplicate collapse (msr_doc_signatures, msr_bind_signatures, msr_collapse_duplicates, include/msretr.h; DESIGN.md
// section 3, K18).  All of it is uint32 arithmetic mod 2^32: every output byte is a function of the inputs.
//
// Signatures.  A document's shingles are the windows of L = min(w, n) tokens of its indexed stream; shingle a hashes to h(a)
// (FNV-style over token + 1, then murmur3's finaliser), and word k of the signature is the minimum over a of A[k] h(a) + B[k].
// One wave per document, lane k owns word k.  Per chunk of 64 tokens: one coalesced load (lane l = position b0 + l, bounded
// by the document's end as tokscan::load_token bounds it), each lane hashes the shingle that starts at its own position --
// the L - 1 following tokens come from the neighbouring lanes and from the next chunk, whose load is already in flight --
// then a wave-uniform loop over the chunk's valid starts: broadcast h (readlane, uniform index), one multiply-add, one
// minimum.  No dependent load.
// A long page must not hold the launch up behind one wave, so a workgroup is SIG_WAVES waves over SIG_WAVES consecutive
// documents, and only a workgroup that holds a document of more than SIG_SEG shingle starts takes the shared path: the
// segments of SIG_SEG starts of its documents are dealt round over its waves, each wave keeps a partial minimum per document
// in LDS, and after ONE barrier wave i joins document i's partials.  Minimum is associative: the bytes are the same.  Every
// other workgroup meets no barrier and touches no LDS.
//
// Collapse of a query's fused list (slots in fused order).  Step a, one workgroup per (query, tile of 64 slots i, tile of 64
// slots j <= i): both tiles' signatures in LDS (rows 65 words apart: lane j reads its row at bank (j + k) % 64), wave per
// row i, lane per j; a pair stops counting once its mismatches exceed 64 - min_matches -- exact -- and the wave stops when
// every lane has; the ballot of dup(i, j) is the two words of row i the tile owns, stored whole with plain stores.  A slot
// that is passive (document outside the table, EMPTY signature, rejected by the bound domain table) has a zero row AND a
// zero column, so step b needs no flag for it.  Step b, one workgroup per query: wave 0 walks the slots in order with the
// kept set as a bit vector across its lanes (lane l = slots 32 l ..), rows loaded a batch ahead; row i AND kept, a ballot and
// two find-firsts give the leader, the smallest kept duplicate slot; running counts give each slot its place.  Then all
// waves move the rows, recount the matches of each dropped row against its leader, and pad.  No global atomic, no memset:
// step b reads exactly the words step a wrote.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msretr.h"
#include "msr_internal.h"

namespace {

constexpr int K = MSR_SIG_WORDS;
static_assert(K == 64, "lane k of a wave owns word k of a signature");
static_assert(MSR_SIG_MAX_SHINGLE >= 1 && MSR_SIG_MAX_SHINGLE <= 64, "a shingle spans at most the current chunk and the next");
static_assert(MSR_COLLAPSE_MAX_CAND <= 1024, "the kept set is one 32-bit word in each of 32 lanes; a leader fits 16 bits");
constexpr uint32_t EMPTY_WORD = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t fmix(uint32_t x) {
    x ^= x >> 16; x *= 0x85EBCA6Bu;
    x ^= x >> 13; x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

// ---- signatures -----------------------------------------------------------------------------------------------------------------
constexpr int SIG_WAVES = 8;                 // waves, and documents, per workgroup
constexpr int SIG_THREADS = SIG_WAVES * 64;
constexpr int SIG_SEG = 4096;                // shingle starts per segment of a long document (64 chunks)
static_assert(SIG_SEG % 64 == 0, "a segment is whole chunks");

// lane l's 64-bit value as a wave-uniform one (l uniform): the loop bounds made of it stay in scalar registers
__device__ __forceinline__ int64_t lane_value(int64_t v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), l);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ int32_t sig_token(const int32_t* tok_ids, int64_t pos, int64_t e) {
    return pos < e ? tok_ids[pos] : -1;      // THE BOUND OF EVERY READ IS THE DOCUMENT'S END (msr_tokscan.h load_token)
}

// m <- min(m, A h(a) + B) over the starts a in [a0, a1) of document [s, e), 0 <= a0 < a1 <= n - L + 1: every shingle read
// ends at s + a1 - 1 + L <= e.  Every lane of the wave calls this with the same arguments but lane / A / B / m.
__device__ __forceinline__ uint32_t sig_starts(const int32_t* __restrict__ tok_ids, int64_t s, int64_t e, int L, int64_t a0,
                                               int64_t a1, int lane, uint32_t A, uint32_t B, uint32_t m) {
    const int64_t end = s + a1;
    int64_t pos = s + a0 + lane;
    int32_t t_cur = sig_token(tok_ids, pos, e);
    pos += 64;
    int32_t t_nxt = sig_token(tok_ids, pos, e);
    for (int64_t b0 = s + a0; b0 < end; b0 += 64) {
        pos += 64;
        const int32_t t_far = sig_token(tok_ids, pos, e);            // in flight while this chunk is hashed
        uint32_t x = ((uint32_t)t_cur + 1u) * 0x01000193u;           // j = 0: (0 ^ (token + 1)) * prime
        for (int j = 1; j < L; ++j) {                                // the token j places on: a neighbour's, or the next chunk's
            const int src = (lane + j) & 63;
            const int32_t a = __shfl(t_cur, src), b = __shfl(t_nxt, src);
            const uint32_t t = (uint32_t)(lane + j < 64 ? a : b);
            x = (x ^ (t + 1u)) * 0x01000193u;
        }
        const uint32_t h = fmix(x ^ (uint32_t)L);
        const int cnt = (int)(end - b0 < 64 ? end - b0 : 64);        // wave-uniform: the chunk's starts that are the document's
        for (int i = 0; i < cnt; ++i) {
            const uint32_t v = A * (uint32_t)__builtin_amdgcn_readlane((int)h, i) + B;
            m = v < m ? v : m;
        }
        t_cur = t_nxt;
        t_nxt = t_far;
    }
    return m;
}

__global__ __launch_bounds__(SIG_THREADS) void doc_signatures_kernel(const int64_t* __restrict__ tok_off,
                                                                     const int32_t* __restrict__ tok_ids, int64_t d0, int64_t d1,
                                                                     int shingle, uint32_t* __restrict__ out) {
    __shared__ uint32_t part[SIG_WAVES][SIG_WAVES][K];               // [document][wave][word]; the shared path only
    const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int64_t base = d0 + (int64_t)blockIdx.x * SIG_WAVES;       // < d1 (the grid is ceil((d1 - d0) / SIG_WAVES))
    // the offsets of the workgroup's documents, clamped to d1 (<= n_docs): a document past the range has length 0
    const int64_t off = tok_off[min(base + min(lane, SIG_WAVES), d1)];
    const uint32_t A = fmix(2u * (uint32_t)lane + 1u) | 1u, B = fmix(2u * (uint32_t)lane + 2u);
    bool any_long = false;                                           // the same in every wave of the workgroup
    for (int i = 0; i < SIG_WAVES; ++i) {
        const int64_t n = lane_value(off, i + 1) - lane_value(off, i);
        any_long |= n - min((int64_t)shingle, n) + 1 > SIG_SEG;
    }
    if (!any_long) {
        const int64_t d = base + wave;
        if (d >= d1) return;
        const int64_t s = lane_value(off, wave), e = lane_value(off, wave + 1), n = e - s;
        uint32_t m = EMPTY_WORD;
        if (n > 0) {
            const int L = (int)min((int64_t)shingle, n);
            m = sig_starts(tok_ids, s, e, L, 0, n - L + 1, lane, A, B, m);
        }
        out[(d - d0) * K + lane] = m;
        return;
    }
    for (int i = 0; i < SIG_WAVES; ++i) {                            // segment g of document i goes to wave (i + g) % SIG_WAVES
        const int64_t s = lane_value(off, i), e = lane_value(off, i + 1), n = e - s;
        uint32_t m = EMPTY_WORD;
        if (n > 0) {
            const int L = (int)min((int64_t)shingle, n);
            const int64_t starts = n - L + 1;
            for (int64_t a0 = (int64_t)((wave - i + SIG_WAVES) % SIG_WAVES) * SIG_SEG; a0 < starts; a0 += (int64_t)SIG_WAVES * SIG_SEG)
                m = sig_starts(tok_ids, s, e, L, a0, min(a0 + SIG_SEG, starts), lane, A, B, m);
        }
        part[i][wave][lane] = m;
    }
    __syncthreads();
    const int64_t d = base + wave;
    if (d >= d1) return;
    uint32_t m = EMPTY_WORD;
    for (int w = 0; w < SIG_WAVES; ++w) m = min(m, part[wave][w][lane]);
    out[(d - d0) * K + lane] = m;
}

// ---- collapse, step a: the dup bit matrix ---------------------------------------------------------------------------------------
constexpr int TILE = 64;                     // slots per tile: a row's bits of one tile are two words
constexpr int ROW = K + 1;                   // LDS words between two signatures of a tile
constexpr int DUP_THREADS = 256, DUP_WAVES = DUP_THREADS / 64;

struct CollapseArgs {
    const uint32_t* sig; int64_t n_sig;                  // the bound signature table
    const int32_t* doc_domain; int64_t n_domain;         // nullable: the bound domain table
    const int32_t* f_doc; const double* f_score; const double* f_orig; const int32_t* f_chunk; const int32_t* f_n;
    int32_t max_cand, min_matches, wpr;                  // wpr = ceil(max_cand / 32): words per row of the matrix
    uint32_t* bits;                                      // [n_queries][max_cand][wpr]
    int32_t* out_doc; double* out_score; double* out_orig; int32_t* out_chunk; int32_t* out_n;
    int32_t* drop_doc; int32_t* drop_leader; int32_t* drop_matches; int32_t* drop_n;
};

__device__ __forceinline__ int clamp_n(int n, int max_cand) { return n < 0 ? 0 : n > max_cand ? max_cand : n; }

// the signature of slot `slot` of query row `row` into dst[0 .. K) (lane = word); -> the slot takes part in comparisons (it is
// below n and not passive).  Wave-uniform result; a slot that does not take part leaves dst as it is (never compared).
__device__ __forceinline__ bool load_slot(const CollapseArgs& a, int64_t row, int slot, int n, int lane, uint32_t* dst) {
    if (slot >= n) return false;
    const int64_t d = a.f_doc[row + slot];
    if (d < 0 || d >= a.n_sig) return false;
    if (a.doc_domain && (d >= a.n_domain || a.doc_domain[d] < 0)) return false;
    const uint32_t w = a.sig[d * K + lane];
    dst[lane] = w;
    return __ballot(w != EMPTY_WORD) != 0;
}

__global__ __launch_bounds__(DUP_THREADS) void dup_matrix_kernel(const CollapseArgs a) {
    __shared__ uint32_t Si[TILE * ROW], Sj[TILE * ROW];
    __shared__ uint32_t act_i[TILE], act_j[TILE];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int q = (int)blockIdx.y;
    int ti = 0;                                          // blockIdx.x = ti (ti + 1) / 2 + tj, tj <= ti
    while ((ti + 1) * (ti + 2) / 2 <= (int)blockIdx.x) ++ti;
    const int tj = (int)blockIdx.x - ti * (ti + 1) / 2;
    const int n = clamp_n(a.f_n[q], a.max_cand);
    if (ti * TILE >= n) return;                          // step b reads no row at or past n
    const int64_t row = (int64_t)q * a.max_cand;
    for (int r = wave; r < TILE; r += DUP_WAVES) {
        const bool ok = load_slot(a, row, ti * TILE + r, n, lane, Si + r * ROW);
        if (lane == 0) act_i[r] = ok;
        if (tj != ti) {
            const bool okj = load_slot(a, row, tj * TILE + r, n, lane, Sj + r * ROW);
            if (lane == 0) act_j[r] = okj;
        }
    }
    __syncthreads();
    const uint32_t* S2 = tj == ti ? Si : Sj;
    const uint32_t* act2 = tj == ti ? act_i : act_j;
    const int max_miss = K - a.min_matches;              // a pair with more mismatches is no duplicate
    const int j = tj * TILE + lane;
    const bool j_ok = act2[lane] != 0;
    for (int r = wave; r < TILE; r += DUP_WAVES) {
        const int i = ti * TILE + r;
        if (i >= n) break;
        bool live = j_ok && j < i && act_i[r] != 0;      // this lane's pair is still undecided
        int miss = 0;
        if (__ballot(live)) {
            const uint32_t* si = Si + r * ROW;
            const uint32_t* sj = S2 + lane * ROW;
            for (int k = 0; k < K; ++k) {
                if (live) {
                    miss += si[k] != sj[k];
                    live = miss <= max_miss;
                }
                if (!__ballot(live)) break;
            }
        }
        const uint64_t dup = __ballot(live);             // what is still live after K words has at most max_miss mismatches
        uint32_t* out = a.bits + (row + i) * a.wpr + tj * 2;
        if (lane == 0) out[0] = (uint32_t)dup;
        if (lane == 1 && tj * 2 + 1 < a.wpr) out[1] = (uint32_t)(dup >> 32);
    }
}

// ---- collapse, step b: the greedy order, the move, the padding ------------------------------------------------------------------
constexpr int RES_THREADS = 256, RES_WAVES = RES_THREADS / 64;
constexpr int BATCH = 16;                    // matrix rows wave 0 loads ahead of the ones it resolves

__global__ __launch_bounds__(RES_THREADS) void collapse_resolve_kernel(const CollapseArgs a) {
    __shared__ int16_t leader[MSR_COLLAPSE_MAX_CAND];    // the slot that swallowed slot i, -1 = kept
    __shared__ int16_t place[MSR_COLLAPSE_MAX_CAND];     // the slot's position among the kept / among the dropped
    __shared__ int32_t counts[2];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = (int)blockIdx.x;
    const int n = clamp_n(a.f_n[q], a.max_cand);
    const int64_t row = (int64_t)q * a.max_cand;
    if (wave == 0) {
        const uint32_t* bits = a.bits + row * a.wpr;
        uint32_t kept = 0;                               // lane l: slots 32 l .. 32 l + 31
        int n_kept = 0, n_drop = 0;
        uint32_t cur[BATCH], nxt[BATCH];
        // row i holds words 0 .. i >> 5 (step a wrote exactly those, and more): lane l reads word l of it, or nothing
#pragma unroll
        for (int u = 0; u < BATCH; ++u) cur[u] = (u < n && lane <= (u >> 5)) ? bits[(int64_t)u * a.wpr + lane] : 0u;
        for (int i0 = 0; i0 < n; i0 += BATCH) {
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int i = i0 + BATCH + u;
                nxt[u] = (i < n && lane <= (i >> 5)) ? bits[(int64_t)i * a.wpr + lane] : 0u;
            }
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int i = i0 + u;
                if (i < n) {                             // (wave-uniform)
                    const uint32_t x = cur[u] & kept;
                    const uint64_t hit = __ballot(x != 0);
                    int lead = -1;
                    if (hit) {
                        const int l = __ffsll((unsigned long long)hit) - 1;
                        lead = l * 32 + __ffs(__builtin_amdgcn_readlane((int)x, l)) - 1;
                    } else if (lane == (i >> 5)) {
                        kept |= 1u << (i & 31);
                    }
                    if (lane == 0) {
                        leader[i] = (int16_t)lead;
                        place[i] = (int16_t)(lead < 0 ? n_kept : n_drop);
                    }
                    if (lead < 0) ++n_kept; else ++n_drop;
                }
            }
#pragma unroll
            for (int u = 0; u < BATCH; ++u) cur[u] = nxt[u];
        }
        if (lane == 0) { counts[0] = n_kept; counts[1] = n_drop; }
    }
    __syncthreads();
    const int n_kept = counts[0], n_drop = counts[1];
    for (int i = tid; i < n; i += RES_THREADS) {
        const int lead = leader[i], p = place[i];
        const int32_t d = a.f_doc[row + i];
        if (lead < 0) {
            a.out_doc[row + p] = d; a.out_score[row + p] = a.f_score[row + i];
            a.out_orig[row + p] = a.f_orig[row + i]; a.out_chunk[row + p] = a.f_chunk[row + i];
        } else {
            a.drop_doc[row + p] = d; a.drop_leader[row + p] = a.f_doc[row + lead];
        }
    }
    for (int i = wave; i < n; i += RES_WAVES) {          // matches(dropped row, its leader): both are documents of the table
        const int lead = leader[i];
        if (lead < 0) continue;
        const int64_t d = a.f_doc[row + i], dl = a.f_doc[row + lead];
        const uint64_t eq = __ballot(a.sig[d * K + lane] == a.sig[dl * K + lane]);
        if (lane == 0) a.drop_matches[row + place[i]] = __popcll((unsigned long long)eq);
    }
    for (int p = n_kept + tid; p < a.max_cand; p += RES_THREADS) {
        a.out_doc[row + p] = -1; a.out_score[row + p] = -__builtin_inf(); a.out_orig[row + p] = 0.0; a.out_chunk[row + p] = -1;
    }
    for (int p = n_drop + tid; p < a.max_cand; p += RES_THREADS) {
        a.drop_doc[row + p] = -1; a.drop_leader[row + p] = -1; a.drop_matches[row + p] = 0;
    }
    if (tid == 0) { a.out_n[q] = n_kept; a.drop_n[q] = n_drop; }
}

}  // namespace

hipError_t msr_doc_signatures_run(const int64_t* tok_off, const int32_t* tok_ids, int64_t d0, int64_t d1, int shingle,
                                  uint32_t* out, hipStream_t stream) {
    if (d1 <= d0) return hipSuccess;
    const int64_t blocks = (d1 - d0 + SIG_WAVES - 1) / SIG_WAVES;
    if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(doc_signatures_kernel, dim3((unsigned)blocks), dim3(SIG_THREADS), 0, stream, tok_off, tok_ids, d0, d1, shingle,
                       out);
    return hipGetLastError();
}

int64_t msr_collapse_bytes(int n_queries, int max_cand) {
    const int64_t wpr = (max_cand + 31) / 32;
    return ((int64_t)n_queries * max_cand * wpr * 4 + 15) / 16 * 16;
}

hipError_t msr_collapse_run(const uint32_t* sig, int64_t n_sig, const int32_t* doc_domain, int64_t n_domain, int n_queries,
                            const int32_t* f_doc, const double* f_score, const double* f_orig, const int32_t* f_chunk,
                            const int32_t* f_n, int max_cand, int min_matches, int32_t* out_doc, double* out_score,
                            double* out_orig, int32_t* out_chunk, int32_t* out_n, int32_t* drop_doc, int32_t* drop_leader,
                            int32_t* drop_matches, int32_t* drop_n, void* scratch, hipStream_t stream) {
    if (n_queries <= 0) return hipSuccess;
    if (max_cand < 1 || max_cand > MSR_COLLAPSE_MAX_CAND || min_matches < 1 || min_matches > K) return hipErrorInvalidValue;
    const CollapseArgs a{sig, n_sig, doc_domain, doc_domain ? n_domain : 0, f_doc, f_score, f_orig, f_chunk, f_n, max_cand,
                         min_matches, (max_cand + 31) / 32, static_cast<uint32_t*>(scratch), out_doc, out_score, out_orig,
                         out_chunk, out_n, drop_doc, drop_leader, drop_matches, drop_n};
    const int T = (max_cand + TILE - 1) / TILE;
    for (int q0 = 0; q0 < n_queries; q0 += 32768) {      // (the grid's y extent is 16 bits)
        CollapseArgs s = a;
        const int nq = n_queries - q0 < 32768 ? n_queries - q0 : 32768;
        const int64_t r0 = (int64_t)q0 * max_cand;
        s.f_doc += r0; s.f_n += q0; s.bits += r0 * a.wpr;
        hipLaunchKernelGGL(dup_matrix_kernel, dim3((unsigned)(T * (T + 1) / 2), (unsigned)nq), dim3(DUP_THREADS), 0, stream, s);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    hipLaunchKernelGGL(collapse_resolve_kernel, dim3((unsigned)n_queries), dim3(RES_THREADS), 0, stream, a);
    return hipGetLastError();
}
