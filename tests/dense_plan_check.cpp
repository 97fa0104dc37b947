// Stand-alone check of csrc/msr_dense_plan.h on the CPU: the whole input space of the dense sweep plan against a table
// written out here.  Built and run by tests/test_dense_plan.py (with the host sanitizers); exit status 0 = pass.
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

#include "msr_dense_plan.h"

#define CHECK(cond)                                                                                                   \
    do {                                                                                                              \
        if (!(cond)) {                                                                                                \
            printf("%s:%d: CHECK(%s) failed at variant=%d layout=%d wide_ok=%d wide_ok64=%d max_chunks=%d nq=%d\n",   \
                   __FILE__, __LINE__, #cond, b.variant, b.layout, b.wide_ok, b.wide_ok64, mc, nq);                   \
            exit(1);                                                                                                  \
        }                                                                                                             \
    } while (0)

struct Want { int slice; DenseKernel kernel; int qb; };

// The f32-row table, a row per case.
static Want want_f32(int variant, int layout, int wide_ok, int max_chunks, int nq) {
    const bool ksplit = layout == 0 && wide_ok == 1 && max_chunks == 0;
    const int narrow_qb = nq <= 16 ? 1 : 2;
    switch (variant) {
    case 14:
        if (ksplit) return Want{64, DENSE_KSPLIT_F16X2, nq <= 32 ? 2 : 4};
        return Want{32, DENSE_NARROW_F16X2, narrow_qb};       // (an explicit 14 on an interleaved layout lands here)
    case 15:
        if (ksplit) return Want{64, DENSE_KSPLIT_PRESPLIT, nq <= 32 ? 2 : 4};
        return Want{32, DENSE_NARROW_F16X2, narrow_qb};
    case 2:
        if (ksplit && nq > 32) return Want{64, DENSE_KSPLIT_EXACT, 4};
        return Want{ksplit ? 64 : 32, DENSE_NARROW_EXACT, narrow_qb};
    default:                                                   // 7
        return Want{32, DENSE_NARROW_F16X2, narrow_qb};
    }
}

// The bf16 table.
static Want want_bf16(int wide_ok, int wide_ok64, int max_chunks, int nq) {
    const bool wide_able = wide_ok == 1 && max_chunks == 0;
    const int slice = wide_able && wide_ok64 == 1 ? 128 : 64;
    if (wide_able && nq > 32) return Want{slice, DENSE_BF16_KSPLIT, nq > 64 ? 8 : 4};
    return Want{slice, DENSE_BF16_NARROW, nq <= 16 ? 1 : nq <= 32 ? 2 : nq <= 48 ? 3 : 4};
}

// Query blocks of the largest instance of each kernel (the template instances of msr_dense.hip / msr_dense_ks.hip): the
// wave-streaming kernel holds 2 blocks of f32-row queries in LDS or 4 of bf16; the K-split kernel 4, or 8 over bf16 rows with
// the ring of 64 documents.
static int largest_qb(DenseKernel kernel, int wide_ok64) {
    switch (kernel) {
    case DENSE_NARROW_EXACT: case DENSE_NARROW_F16X2: return 2;
    case DENSE_KSPLIT_F16X2: case DENSE_KSPLIT_PRESPLIT: case DENSE_KSPLIT_EXACT: return 4;
    case DENSE_BF16_NARROW: return 4;
    case DENSE_BF16_KSPLIT: return wide_ok64 ? 8 : 4;
    }
    return 0;
}

int main() {
    static_assert(MSR_SCAN_EXACT == 2 && MSR_SCAN_F16X2 == 7 && MSR_SCAN_KSPLIT == 14 && MSR_SCAN_PRESPLIT == 15 &&
                  MSR_SCAN_AUTO == 0, "the values of msr_config.scan_variant");
    static_assert(MSR_DENSE_FALLBACK_SLICE == 64 && dense_fallback_slices(64) == 1 && dense_fallback_slices(65) == 2 &&
                  dense_fallback_pad(1) == 64 && dense_fallback_pad(129) == 192, "the gated fallback's slices");
    const int variants[4] = {2, 7, 14, 15};
    long cases = 0;
    for (int variant : variants)
    for (int layout = 0; layout < 2; ++layout)
    for (int wide_ok = 0; wide_ok < 2; ++wide_ok)
    for (int wide_ok64 = 0; wide_ok64 <= wide_ok; ++wide_ok64)             // wide_ok64 implies wide_ok
    for (int mc : {0, 3}) {
        const DenseBinding b{variant, layout, wide_ok, wide_ok64};
        int nq = 0;                                                        // (for CHECK's message)
        CHECK(dense_variant_known(variant) && dense_variant_f16x2(variant) == (variant == 7 || variant == 14 || variant == 15));
        // 4. what msr_scan_width (sweeps) and msr_batch_width report: the slices of a call without a row limit
        {
            const bool wide = (variant == 2 || variant == 14 || variant == 15) && layout == 0 && wide_ok;
            CHECK(dense_slice(b, 0) == (wide ? 64 : 32));
            CHECK(dense_bf16_slice(b, 0) == (wide_ok && wide_ok64 ? 128 : 64));
            // the streaming pass: resolved 14 exactly, on the K-split kernel's preconditions
            CHECK(dense_stream_variant(b) == (variant == 14));
            CHECK(dense_stream_bound(b, true) == (wide && variant == 14) && !dense_stream_bound(b, false));
            CHECK(dense_stream_ok(b, mc, true, 200, 100) == (wide && variant == 14 && mc == 0));
            CHECK(!dense_stream_ok(b, mc, true, 199, 100) && !dense_stream_ok(b, mc, false, 200, 100));
            CHECK(dense_stream_bindable(b, true, 64) == (variant == 14));
            CHECK(!dense_stream_bindable(b, false, 64) && !dense_stream_bindable(b, true, 63));
        }
        for (int bf16 = 0; bf16 < 2; ++bf16) {
            const int slice = bf16 ? dense_bf16_slice(b, mc) : dense_slice(b, mc);
            for (nq = 1; nq <= 128; ++nq) {
                const DensePlan p = bf16 ? dense_bf16_plan(b, nq, mc) : dense_plan(b, nq, mc);
                const Want w = bf16 ? want_bf16(wide_ok, wide_ok64, mc, nq) : want_f32(variant, layout, wide_ok, mc, nq);
                ++cases;
                // 1. the table
                CHECK(slice == w.slice);
                if (nq > slice) { CHECK(p.qb == 0); continue; }            // outside the plan's domain: no instance
                CHECK(p.kernel == w.kernel && p.qb == w.qb);
                CHECK(dense_case(p) == dense_case(w.kernel, w.qb));
                // 2. the instance holds the slice's queries
                CHECK(16 * p.qb >= nq && nq <= slice);
                // 3. a full slice fills the largest instance of the kernel that serves it
                if (nq == slice) CHECK(slice == 16 * largest_qb(p.kernel, wide_ok64) && p.qb == largest_qb(p.kernel, wide_ok64));
                CHECK(p.qb <= largest_qb(p.kernel, wide_ok64));
            }
            nq = 0;
            CHECK((bf16 ? dense_bf16_plan(b, 0, mc) : dense_plan(b, 0, mc)).qb == 0);
        }
    }
    printf("dense plan ok (%ld cases)\n", cases);
    return 0;
}
