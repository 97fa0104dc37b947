// The streaming pass over the f32 rows (msr_gemm_f32.hip): what a binding allocates for it, and for a call how wide a pass
// is, how many query groups share a launch, which rows the launches read, which kernel instance serves a launch and where the
// emit pass is cut -- the one place that decides.  Host-only and free of HIP and engine types
// (tests/stream_plan_check.cpp enumerates it on the CPU).  The engine (msr_engine.hip) sizes the binding from stream_caps;
// msr_gemm_f32_pass plans a call with stream_plan / pass_shape and its launcher switches on stream_kernel.  Which calls
// the pass takes at all: dense_stream_ok and the predicates beside it (msr_dense_plan.h).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "msr_dense_plan.h"

constexpr int STREAM_WAVES = 8;          // waves per workgroup of both kernels = emission buffers per workgroup

// ---- capacities of a binding, from msr_config.max_queries -------------------------------------------------------------------
struct StreamCaps {
    int groups;        // groups of 128 queries one call may hold (bounded by the select scratch: max(max_queries, 128) rows)
    int max_nt;        // groups of 256 queries that may share the rows of one launch of the 256-query kernel
    int wv_cap;        // emitted entries per wave and call: ~600 per 128 queries at 5 M rows (150 x sample stride per query)
    int tmax_row;      // queries per tile row of tmax_t: the most one launch serves
    bool want_copy;    // the fragment-order copy of the rows: read by launches of the 256-query kernel
    bool want_image;   // the f16 image of the rows: read by launches of several groups
    int call_cap;      // queries per call: beyond 128 they run in groups of 256, so an odd last group of 128 is not usable
    int width;         // queries per pass that msr_scan_width reports
};
constexpr StreamCaps stream_caps(int max_queries) {
    const int groups = std::min(8, std::max(max_queries, 128) / 128);
    const int max_nt = std::max(1, std::min(4, groups / 2));
    return StreamCaps{groups, max_nt, 4096 * std::max(1, groups / 2), groups >= 2 ? 256 * max_nt : 128, groups >= 2,
                      max_nt >= 2, groups >= 2 ? (groups & ~1) * 128 : 128, groups >= 2 ? 256 : 128};
}

// ---- the plan of a call -----------------------------------------------------------------------------------------------------
enum StreamQimg { STREAM_QIMG_128, STREAM_QIMG_256, STREAM_QIMG_256_IMAGE16 };   // build_qimg1_kernel / build_qimg2_kernel's forms
struct StreamPlan {
    bool valid;        // 1 <= nq and the call's groups fit the binding
    int W, G;          // queries per pass (128 or 256; a last group that is not full is padded), passes per segment
    int NT;            // groups per launch: up to max_nt groups walk the same tiles on CUs of one XCD and share the rows in its L2
    bool image16;      // the launches read the f16 image: several groups per launch are bound by the matrix pipes, not by HBM
    bool tiled;        // ... the fragment-order copy of the f32 rows (else: the caller's row-major matrix)
    bool nt_loads;     // on the copy, a launch of ONE group loads the rows non-temporally (stream_kernel)
    int tmax_parts;    // rows of tmax_t per tile: one per wave, or one where the kernel joins the waves' maxima in LDS
    bool entry_tmax;   // the emit launches store no tile maxima: they are recovered from the emitted entries
    StreamQimg qimg;
};
constexpr StreamPlan stream_plan(StreamCaps c, int n_cus, int nq, bool has_copy, bool has_image) {
    const int W = nq > 128 ? 256 : 128, G = (nq + W - 1) / W;
    const int NT = W == 256 && n_cus % 8 == 0 ? std::min(std::min(G, c.max_nt), n_cus / 8) : 1;
    const bool image16 = W == 256 && NT > 1 && has_image, tiled = W == 256 && has_copy && !image16;
    return StreamPlan{nq >= 1 && G * W <= 128 * c.groups, W, G, NT, image16, tiled, tiled, image16 ? 1 : STREAM_WAVES,
                      W == 256 && !image16, image16 ? STREAM_QIMG_256_IMAGE16 : W == 256 ? STREAM_QIMG_256 : STREAM_QIMG_128};
}

// The kernel instance of one launch of nt groups (the template instances of msr_gemm_f32.hip).
enum StreamKernel {
    STREAM_IMAGE16,    // gemm_stream256_kernel over the f16 image
    STREAM_128,        // gemm_stream_kernel
    STREAM_COPY_NT,    // gemm_stream256_kernel over the fragment-order copy, rows loaded with the non-temporal policy
    STREAM_COPY,       // gemm_stream256_kernel over the fragment-order copy
    STREAM_ROWS,       // gemm_stream256_kernel over the row-major rows
};
// One group per launch reads every row exactly once, by one wave: loaded non-temporally, the 15 GB stream does not displace the
// 384 KB query image (re-read by every workgroup for every tile) from the L2s -- 3.07 -> 2.94 ms per pass
// (profiles/r04_stream256_experiments.md).  Several groups per launch share the rows through the L2: the default policy.
constexpr StreamKernel stream_kernel(StreamPlan p, int nt) {
    return p.image16 ? STREAM_IMAGE16 : p.W == 128 ? STREAM_128 : p.tiled && p.nt_loads && nt == 1 ? STREAM_COPY_NT
         : p.tiled ? STREAM_COPY : STREAM_ROWS;
}
constexpr int stream_case(StreamKernel kernel, bool emit) { return (int)kernel * 2 + (emit ? 1 : 0); }   // switch label

// ---- which tiles the sample pass visits, where the emit pass is cut ---------------------------------------------------------
// Sample: every ss-th tile (ss / 2, ss / 2 + ss, ...: n_s of them) bounds the k-th score from below; >= per_k k sampled tiles,
// ss <= cap (the weaker the bound, the more entries the emit pass writes: ~150 ss per query).  The f32 pass samples with
// (3, 64), the bf16 candidate pass (msr_gemm.hip) with (8, 16).
struct StreamSample { int ss, n_s; };
constexpr StreamSample stream_sample(int T, int k, int per_k, int cap) {
    const int ss = std::max(1, std::min(cap, T / (per_k * k)));
    return StreamSample{ss, (T - ss / 2 + ss - 1) / ss};
}
// Segments: tile maxima are by-products of the emit pass itself, and ANY set of >= k distinct tiles bounds the k-th
// document score from below (documents never straddle tiles).  So the pass emits over the first T1 tiles with the sample's
// threshold, takes the k-th largest of THOSE T1 maxima (gemm_kth_kernel, raise mode: thr = max(thr, k-th - margin)) and
// emits over the rest with the raised threshold.  With entries ~ c (T1 / n_s + (T - T1) / T1) the optimum is
// T1 = sqrt(T n_s); T1 is the multiple of the grid nearest to that, so that both segments run whole rounds of the persistent
// grid, and the cut is made only where T1 >= max(grid, 2 k) and T - T1 >= grid: smaller corpora keep the one-launch pass.
// thr(sample) <= thr(first T1) <= thr2(all tiles) -- subsets of the same maxima, the same margin --, so what the bucket
// keeps (score >= thr2) is the same set of entries either way: results do not move, the wave buffers only get fewer entries.
// (Other cuts and three segments were measured and not kept: profiles/dense_emit_segments.md.  Restated in numpy and
// compared case by case by tests/test_dense_segments_host.py.)
struct PassShape {
    int ss, n_s;       // the sample (stream_sample)
    int n_seg;         // emit launches per group: 1 or 2
    int bound[3];      // segment s covers tiles [bound[s], bound[s + 1])
};
inline PassShape pass_shape(int T, int k, int grid, bool single) {
    const StreamSample sm = stream_sample(T, k, 3, 64);
    const int64_t t1 = (int64_t)std::floor(std::sqrt((double)T * (double)sm.n_s) / grid + 0.5) * grid;
    if (!single && t1 >= std::max(grid, 2 * k) && T - t1 >= grid) return PassShape{sm.ss, sm.n_s, 2, {0, (int)t1, T}};
    return PassShape{sm.ss, sm.n_s, 1, {0, T, T}};
}
