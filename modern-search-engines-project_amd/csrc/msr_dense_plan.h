// Which dense sweep kernel serves a slice of queries, how wide a slice is, and how many query rows the kernel reads: the one
// place that decides.  Host-only and free of HIP and engine types (tests/dense_plan_check.cpp enumerates it on the CPU).  The
// engine (msr_engine.hip) takes slice widths, query padding and the predicates from here; the launchers (msr_dense.hip,
// msr_dense_ks.hip) call the same plan function and switch on its result, so the two cannot disagree.
#pragma once

// The resolved scan kind of a binding: the values of msr_config.scan_variant (msr_bind_chunks resolves AUTO).
constexpr int MSR_SCAN_AUTO = 0;         // msr_config only: K-split f16x2, else f16x2, else exact, by row norms and layout
constexpr int MSR_SCAN_EXACT = 2;        // exact f32 MFMA products: wave streaming up to 32 queries, K-split above
constexpr int MSR_SCAN_F16X2 = 7;        // f16-split products, wave streaming
constexpr int MSR_SCAN_KSPLIT = 14;      // f16-split products, K-split kernel preferred; the only kind the streaming pass serves
constexpr int MSR_SCAN_PRESPLIT = 15;    // A/B: K-split kernel over a pre-split f16 hi/lo copy of the rows

constexpr bool dense_variant_known(int v) {
    return v == MSR_SCAN_EXACT || v == MSR_SCAN_F16X2 || v == MSR_SCAN_KSPLIT || v == MSR_SCAN_PRESPLIT;
}
constexpr bool dense_variant_f16x2(int v) { return v != MSR_SCAN_EXACT; }       // the products' arithmetic (msr_scan_arith)

// What the plan needs from a binding (DenseIndex: msr_internal.h dense_binding).
struct DenseBinding {
    int variant;     // resolved: EXACT, F16X2, KSPLIT or PRESPLIT
    int layout;      // 0 row-major, 1 interleaved
    int wide_ok;     // the K-split kernels' ring of 128 documents never wraps onto live slots (chunk_layout)
    int wide_ok64;   // the same for a ring of 64 documents (implies wide_ok)
};

enum DenseKernel {
    DENSE_NARROW_EXACT,      // dense_scan_v2_kernel, f32 rows, exact f32 products
    DENSE_NARROW_F16X2,      // dense_scan_v2_kernel, f32 rows, f16-split products
    DENSE_KSPLIT_F16X2,      // dense_ksplit_kernel, f32 rows split on the fly
    DENSE_KSPLIT_PRESPLIT,   // dense_ksplit_kernel, the pre-split copy of the rows
    DENSE_KSPLIT_EXACT,      // dense_ksplit_kernel, exact f32 products
    DENSE_BF16_NARROW,       // dense_scan_v2_kernel, bf16 rows
    DENSE_BF16_KSPLIT,       // dense_ksplit_kernel, bf16 rows
};
// qb: 16-query blocks of the template instance that runs -- it reads 16 * qb rows of qn.  0: nq lies outside [1, slice].
struct DensePlan {
    DenseKernel kernel;
    int qb;
};
constexpr int dense_case(DenseKernel kernel, int qb) { return (int)kernel * 16 + qb; }     // switch label of an instance
constexpr int dense_case(DensePlan p) { return dense_case(p.kernel, p.qb); }

// ---- sweeps over the f32 rows ---------------------------------------------------------------------------------------------
// The K-split kernels need row-major rows, the ring precondition and no per-document row limit; F16X2 never asks for them.
constexpr bool dense_ksplit_ok(DenseBinding b, int max_chunks) {
    return (b.variant == MSR_SCAN_EXACT || b.variant == MSR_SCAN_KSPLIT || b.variant == MSR_SCAN_PRESPLIT) && b.layout == 0 &&
           b.wide_ok && max_chunks == 0;
}
// Queries per pass over the matrix.
constexpr int dense_slice(DenseBinding b, int max_chunks) { return dense_ksplit_ok(b, max_chunks) ? 64 : 32; }
constexpr DensePlan dense_plan(DenseBinding b, int nq, int max_chunks) {
    const bool ks = dense_ksplit_ok(b, max_chunks);
    const int qb = nq < 1 || nq > dense_slice(b, max_chunks) ? 0 : nq <= 16 ? 1 : nq <= 32 ? 2 : 4;
    if (ks && b.variant == MSR_SCAN_KSPLIT) return DensePlan{DENSE_KSPLIT_F16X2, qb == 1 ? 2 : qb};
    if (ks && b.variant == MSR_SCAN_PRESPLIT) return DensePlan{DENSE_KSPLIT_PRESPLIT, qb == 1 ? 2 : qb};
    // exact products: the K-split kernel pays off above 32 queries only (matrix-core bound: 4.5 ms per 64 queries against
    // 2 x 2.8 ms on the narrow kernel; at <= 32 queries the narrow kernel is faster)
    if (ks && qb == 4) return DensePlan{DENSE_KSPLIT_EXACT, qb};
    return DensePlan{b.variant == MSR_SCAN_EXACT ? DENSE_NARROW_EXACT : DENSE_NARROW_F16X2, qb};
}

// ---- sweeps over the bf16 image (the batched path's candidate generator) --------------------------------------------------
constexpr bool dense_bf16_ksplit_ok(DenseBinding b, int max_chunks) { return b.wide_ok && max_chunks == 0; }
constexpr int dense_bf16_slice(DenseBinding b, int max_chunks) {
    return dense_bf16_ksplit_ok(b, max_chunks) && b.wide_ok64 ? 128 : 64;
}
constexpr DensePlan dense_bf16_plan(DenseBinding b, int nq, int max_chunks) {
    if (nq < 1 || nq > dense_bf16_slice(b, max_chunks)) return DensePlan{DENSE_BF16_NARROW, 0};
    if (dense_bf16_ksplit_ok(b, max_chunks) && nq > 32) return DensePlan{DENSE_BF16_KSPLIT, nq > 64 ? 8 : 4};
    return DensePlan{DENSE_BF16_NARROW, (nq + 15) / 16};
}

// ---- the streaming pass over the f32 rows (msr_gemm_f32.hip) and the gated sweeps behind it ---------------------------------
constexpr bool dense_stream_variant(DenseBinding b) { return b.variant == MSR_SCAN_KSPLIT; }
// msr_bind_chunks builds the pass' tables: every document inside one row tile, enough tiles to sample
constexpr bool dense_stream_bindable(DenseBinding b, bool tiles_ok, int n_tiles) {
    return tiles_ok && dense_stream_variant(b) && n_tiles >= 64;
}
// the pass serves the binding (gf_ok: its tables were built): its gated sweeps are the 64-query K-split f16x2 instance
constexpr bool dense_stream_bound(DenseBinding b, bool gf_ok) {
    return dense_ksplit_ok(b, 0) && gf_ok && dense_stream_variant(b);
}
// ... and takes a call of more than one slice of queries asking for k documents
constexpr bool dense_stream_ok(DenseBinding b, int max_chunks, bool gf_ok, int n_tiles, int k) {
    return max_chunks == 0 && dense_stream_bound(b, gf_ok) && n_tiles >= 2 * k;
}
// The gated fallback (msr_dense_scan_slices) sweeps all queries of a call as slices of 64 with one gate word each: the
// 64-query K-split instance, its queries zero-padded to whole slices.
constexpr int MSR_DENSE_FALLBACK_SLICE = 64;
constexpr int dense_fallback_slices(int nq) { return (nq + MSR_DENSE_FALLBACK_SLICE - 1) / MSR_DENSE_FALLBACK_SLICE; }
constexpr int dense_fallback_pad(int nq) { return dense_fallback_slices(nq) * MSR_DENSE_FALLBACK_SLICE; }
