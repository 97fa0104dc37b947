// K16: prefix and wildcard lookup (msr_wildcard_terms; include/msretr.h).
//
// For every pattern of a call -- `*` any run of code points, `?` exactly one, anything else itself, anchored at both ends --
// the vocabulary terms it matches, ordered by (weight descending, term id), the first `limit` of them and the number of all.
// K15's shape and K15's pieces (msr_vocabscan.h): two kernels, no atomics, the same bytes every time.
//
// SCAN.  One workgroup owns WC_SPAN consecutive terms, one lane per term.  The lane keeps its term twice for the whole kernel,
// two code points per register: left-aligned (code point i in slot i) and right-aligned (the last code point in slot 31), with
// its length, its key and its 64-bit character-set signature; the workgroup also leaves the span's terms in LDS, one column
// per lane (s_term[i][lane]: lanes of a wave read neighbouring half-words, whatever their i).  The call's patterns come through
// LDS WC_G at a time.  32 threads stage one pattern and derive, with one ballot and a shuffle-or,
//   n, the symbol count;  n_lit, the symbols that are not `*`;  whether there is a star;
//   sig_lit, the signature of the literal code points (neither `?` nor `*`);
//   the HEAD (the symbols before the first `*`; the whole pattern when it has none), left-aligned like a term, and the TAIL
//   (the symbols behind the last `*`), right-aligned like the term's second image, each with a mask that is 0 where the symbol
//   is `?` and outside the head / tail;
//   whether the MIDDLE -- first to last star -- holds anything but stars.
// Per pattern a lane applies, all lossless,
//   the length tests   L >= n_lit, without a star L == n_lit, with one |head| + |tail| <= L, and
//   the signature test sig_lit & ~sig_t == 0 (every literal code point occurs in the term; hashing only merges characters),
// then head and tail as anchored compares of packed registers, (term ^ pattern) & mask over static indices, as many registers as
// the head / tail is long (wave-uniform).  That decides `head*`, `*tail`, `head*tail` and a pattern without a star.  Only a
// pattern whose middle holds a segment (`a*b*c`, `*a*`) runs the general matcher, on the middle of the term, [|head|, L -
// |tail|): greedy leftmost placement of each segment, written as the one-star-back loop (on a mismatch return to the last
// star and let it take one code point more), which is exact for globs; reaching the last star ends it.  The matcher reads the
// pattern's symbols and the term's code points from LDS: no dynamically indexed register array, no private memory.
// A match is one key (distance bits 0).  Each wave leaves its first `limit` keys (repeated wave minimum: `limit` rounds where
// a wave holds that many matches, which `a*` over 64 neighbouring terms does) and its count in LDS; wave v then merges pattern
// v of the group into the span's slot of the scratch (span_slot_store), exactly as K15.
//
// MERGE.  msr_vocabscan.h's merge_rows without the row of distances: one workgroup per pattern.  A pattern of 0 or more than
// 32 symbols matches nothing in SCAN and gets an empty row here: no host round trip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msretr.h"
#include "msr_internal.h"
#include "msr_sort.h"
#include "msr_vocabscan.h"

namespace {

using namespace msr_vocabscan;

constexpr int WC_SPAN = VS_SPAN;
constexpr int WC_WAVES = VS_WAVES;
constexpr int WC_G = VS_G;
constexpr int WC_LEN = MSR_WILD_MAX_LEN;
constexpr uint32_t WC_STAR = 0x2Au, WC_ANY = 0x3Fu;
static_assert(WC_LEN == VS_LEN && MSR_WILD_MAX_LIMIT == VS_LIM && MSR_WILD_MAX_PATTERNS == MSR_FUZZY_MAX_WORDS,
              "K16 rides on K15's span, group, key and scratch layout");

struct WildArgs {
    const int64_t* char_off; const uint16_t* chars; const uint32_t* weight; const uint64_t* sig;
    int64_t n_terms; int32_t n_spans;
    int32_t n_pat; const int32_t* pat_off; const uint16_t* pat_chars; int32_t limit;
    uint64_t* keys; int32_t* counts;                         // the scratch: [n_pat][n_spans][limit], [n_pat][n_spans]
    int32_t* out_term; int32_t* out_n; int32_t* out_total;
};

struct PatInfo {                                             // what staging derives of one pattern (n == 0: matches nothing)
    int32_t n, n_lit, head, tail, star, general;
};

__global__ __launch_bounds__(WC_SPAN) void wildcard_scan_kernel(const WildArgs a) {
    __shared__ uint16_t s_term[WC_LEN][WC_SPAN];             // the span's terms, one column per lane (64 KB)
    __shared__ uint16_t s_pch[WC_G][WC_LEN];                 // the group's patterns as typed (the general matcher reads them)
    __shared__ uint32_t s_ph[WC_G][WC_LEN / 2], s_phm[WC_G][WC_LEN / 2];     // head, left-aligned, and its mask
    __shared__ uint32_t s_pt[WC_G][WC_LEN / 2], s_ptm[WC_G][WC_LEN / 2];     // tail, right-aligned, and its mask
    __shared__ PatInfo s_pi[WC_G];
    __shared__ uint64_t s_psig[WC_G];
    __shared__ uint64_t s_key[WC_G][WC_WAVES * VS_LIM];
    __shared__ int32_t s_cnt[WC_G][WC_WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int span = (int)blockIdx.x, limit = a.limit;
    const int64_t t = (int64_t)span * WC_SPAN + tid;

    // the lane's term; a lane without one (past n_terms, weight 0, too long) stays to the end: it takes part in every barrier
    bool term_ok = false;
    int L = 0;
    uint32_t tc[WC_LEN / 2], tr[WC_LEN / 2];                 // left-aligned, right-aligned
#pragma unroll
    for (int k = 0; k < WC_LEN / 2; ++k) tc[k] = tr[k] = 0;
    uint64_t st = 0, key = 0;
    if (t < a.n_terms) {
        const uint32_t wt = a.weight[t];
        const int64_t o0 = a.char_off[t], len = a.char_off[t + 1] - o0;
        if (wt > 0 && wt < 0x80000000u && len >= 0 && len <= WC_LEN) {
            term_ok = true;
            L = (int)len;
            st = a.sig[t];
            key = key_low(wt, t);
#pragma unroll
            for (int i = 0; i < WC_LEN; ++i) {
                const uint32_t c = i < L ? a.chars[o0 + i] : 0u;
                const int j = i - (WC_LEN - L);              // the code point that stands in slot i of the right-aligned image
                const uint32_t r = j >= 0 ? a.chars[o0 + j] : 0u;
                tc[i >> 1] |= c << ((i & 1) * 16);
                tr[i >> 1] |= r << ((i & 1) * 16);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < WC_LEN; ++i) s_term[i][tid] = (uint16_t)((tc[i >> 1] >> ((i & 1) * 16)) & 0xFFFFu);
    // (the barrier behind the first staging stands between these writes and the matcher's reads)

    for (int g0 = 0; g0 < a.n_pat; g0 += WC_G) {
        const int ng = imin(WC_G, a.n_pat - g0);
        if (tid < WC_G * 32) {                               // 32 threads stage one pattern: whole waves, two patterns each
            const int g = tid >> 5, c = tid & 31;
            int n = 0, o = 0;
            bool ok = false;
            if (g < ng) {
                o = a.pat_off[g0 + g];
                n = a.pat_off[g0 + g + 1] - o;
                ok = n >= 1 && n <= WC_LEN;
            }
            if (!ok) n = 0;
            const bool have = c < n;
            const uint32_t ch = have ? a.pat_chars[o + c] : 0u;
            const int sh = tid & 32;                         // this pattern's half of the wave's ballots
            const uint32_t stars = (uint32_t)(__ballot(have && ch == WC_STAR) >> sh);
            const bool lit = have && ch != WC_STAR && ch != WC_ANY;
            uint64_t sb = lit ? sig_bit(ch) : 0ull;
            for (int m = 16; m; m >>= 1) sb |= shfl_xor_u64(sb, m);          // (stays inside the 32 lanes of the pattern)
            const bool star = stars != 0;
            const int first = star ? __ffs((int)stars) - 1 : n, last = star ? 31 - __clz((int)stars) : n;
            const int head = first, tail = star ? n - 1 - last : 0;
            // head: slot c holds symbol c; tail: slot c holds symbol c - (32 - n)
            const bool in_head = c < head;
            const int j = c - (WC_LEN - n);
            const bool in_tail = star && j > last;           // (j <= n - 1 always)
            const uint32_t tch = in_tail ? a.pat_chars[o + j] : 0u;
            s_pch[g][c] = (uint16_t)ch;
            ((uint16_t*)&s_ph[g][0])[c] = (uint16_t)(in_head ? ch : 0u);
            ((uint16_t*)&s_phm[g][0])[c] = (uint16_t)(in_head && ch != WC_ANY ? 0xFFFFu : 0u);
            ((uint16_t*)&s_pt[g][0])[c] = (uint16_t)tch;
            ((uint16_t*)&s_ptm[g][0])[c] = (uint16_t)(in_tail && tch != WC_ANY ? 0xFFFFu : 0u);
            if (c == 0) {
                const int n_star = __popc(stars);
                s_pi[g] = PatInfo{n, n - n_star, head, tail, star ? 1 : 0, star && n_star != last - first + 1 ? 1 : 0};
                s_psig[g] = sb;
            }
        }
        __syncthreads();
        for (int g = 0; g < ng; ++g) {
            PatInfo p = s_pi[g];                             // the same in every lane: kept in scalar registers
            p.n = __builtin_amdgcn_readfirstlane(p.n); p.n_lit = __builtin_amdgcn_readfirstlane(p.n_lit);
            p.head = __builtin_amdgcn_readfirstlane(p.head); p.tail = __builtin_amdgcn_readfirstlane(p.tail);
            p.star = __builtin_amdgcn_readfirstlane(p.star); p.general = __builtin_amdgcn_readfirstlane(p.general);
            const uint64_t sp = s_psig[g];
            const bool len_ok = p.star ? (L >= p.n_lit && p.head + p.tail <= L) : L == p.n_lit;
            const bool pass = term_ok && p.n > 0 && len_ok && (sp & ~st) == 0;
            bool hit = false;
            if (__ballot(pass)) {                            // (wave-uniform; the compares are static and cost every lane the same)
                uint32_t diff = 0;
#pragma unroll
                for (int k = 0; k < WC_LEN / 2; ++k)         // (p is the same in every lane: a scalar branch per register)
                    if (2 * k < p.head) diff |= (tc[k] ^ s_ph[g][k]) & s_phm[g][k];
#pragma unroll
                for (int k = 0; k < WC_LEN / 2; ++k)         // register k holds slots 2k and 2k + 1; the tail fills [32 - tail, 32)
                    if (2 * k + 1 >= WC_LEN - p.tail) diff |= (tr[k] ^ s_pt[g][k]) & s_ptm[g][k];
                hit = pass && diff == 0;
                if (hit && p.general) {
                    // the middle of the pattern, [head, n - tail), starts and ends with a star; the middle of the term is
                    // [head, L - tail).  pi == pe is reached only through the last star, which takes whatever is left.
                    int ti = p.head, pi = p.head, back = p.head, mark = p.head;
                    const int te = L - p.tail, pe = p.n - p.tail;
                    bool ok = true;
                    while (pi < pe) {
                        const uint32_t pc = s_pch[g][pi];
                        if (pc == WC_STAR) { back = pi; mark = ti; ++pi; continue; }
                        if (ti < te) {
                            const uint32_t c = s_term[ti][tid];
                            if (pc == WC_ANY || pc == c) { ++ti; ++pi; continue; }
                            ti = ++mark;                     // the last star takes one code point more
                            pi = back + 1;
                            if (ti < te) continue;
                        }
                        ok = false;                          // the term's middle is used up in front of a symbol
                        break;
                    }
                    hit = ok;
                }
            }
            uint64_t mine[1] = {hit ? key : VS_NONE};
            const uint64_t found = __ballot(hit);
            uint64_t keep = VS_NONE;
            if (found) keep = wave_first_keys<1>(mine, limit, lane);
            if (lane < limit) s_key[g][wave * limit + lane] = keep;
            if (lane == 0) s_cnt[g][wave] = __popcll(found);
        }
        __syncthreads();
        if (wave < ng) {                                     // wave v merges pattern v of the group
            const int g = wave;
            span_slot_store(&s_key[g][0], &s_cnt[g][0], limit, lane, (int64_t)(g0 + g) * a.n_spans + span, a.keys, a.counts);
        }
        // (no barrier: the next group's staging writes what this merge does not read, and the barrier behind the staging
        // stands between this merge and the next group's lists)
    }
}

__global__ __launch_bounds__(MG_THREADS) void wildcard_merge_kernel(const WildArgs a) {
    merge_rows<false>(a.keys, a.counts, a.n_spans, a.limit, a.out_term, nullptr, a.out_n, a.out_total);
}

}  // namespace

hipError_t msr_wildcard_terms_run(const int64_t* char_off, const uint16_t* chars, const uint32_t* weight, const uint64_t* sig,
                                  int64_t n_terms, int n_patterns, const int32_t* pat_off, const uint16_t* pat_chars, int limit,
                                  int32_t* out_term, int32_t* out_n, int32_t* out_total, void* scratch, hipStream_t stream) {
    if (n_patterns <= 0) return hipSuccess;
    const int64_t n_spans = msr_fuzzy_spans(n_terms);
    uint64_t* keys = (uint64_t*)scratch;
    int32_t* counts = (int32_t*)(keys + (int64_t)n_patterns * n_spans * limit);
    const WildArgs a{char_off, chars, weight, sig, n_terms, (int32_t)n_spans, n_patterns, pat_off, pat_chars, limit,
                     keys, counts, out_term, out_n, out_total};
    if (n_spans > 0) {
        hipLaunchKernelGGL(wildcard_scan_kernel, dim3((unsigned)n_spans), dim3(WC_SPAN), 0, stream, a);
        hipError_t err = hipGetLastError();
        if (err != hipSuccess) return err;
    }
    hipLaunchKernelGGL(wildcard_merge_kernel, dim3((unsigned)n_patterns), dim3(MG_THREADS), 0, stream, a);
    return hipGetLastError();
}
