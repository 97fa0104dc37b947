// The refusals of msr_match_sets (csrc/msr_match_args.h) as a program of its own: built with the host compiler under its
// address / undefined-behaviour sanitizers by tests/test_match_cases.py.  No GPU, no ROCm runtime.
#include <stdio.h>
#include <string.h>

#include "msr_match_args.h"

static int failures = 0;

static void expect(bool ok, const char* what) {
    if (!ok) {
        printf("FAILED: %s\n", what);
        ++failures;
    }
}

int main() {
    char why[192];
    const int64_t N = 20013, W = (N + 31) / 32;
    // what is accepted
    expect(msr_match_args_check(N, 4, true, W, 0, false, 0, why, sizeof why) == MSR_OK && why[0] == 0, "no bases");
    expect(msr_match_args_check(N, 4, true, W + 3, 2, true, W, why, sizeof why) == MSR_OK, "bases, a wider output row");
    expect(msr_match_args_check(N, 0, false, W, 0, false, 0, why, sizeof why) == MSR_OK, "n_rows == 0 needs no pointer");
    expect(msr_match_args_check(0, 1, true, 0, 0, false, 0, why, sizeof why) == MSR_OK, "an index without documents");
    expect(msr_match_args_check(N, 4, true, W, 0, false, -5, why, sizeof why) == MSR_OK, "base_stride is not read without bases");
    // every refusal, with its reason
    struct Bad { int32_t n_rows; bool rows_ok; int64_t out_stride; int32_t n_base; bool base_ok; int64_t base_stride; const char* says; };
    const Bad bad[] = {
        {-1, true, W, 0, false, 0, "n_rows=-1"},
        {4, true, W, -1, true, W, "n_base=-1"},
        {4, false, W, 0, false, 0, "is NULL with n_rows=4"},
        {4, true, W - 1, 0, false, 0, "out_stride="},
        {0, true, W - 1, 0, false, 0, "out_stride="},
        {4, true, W, 3, false, W, "is NULL with n_base=3"},
        {4, true, W, 3, true, W - 1, "base_stride="},
    };
    for (const Bad& b : bad) {
        memset(why, 'x', sizeof why);
        const int rc = msr_match_args_check(N, b.n_rows, b.rows_ok, b.out_stride, b.n_base, b.base_ok, b.base_stride, why, sizeof why);
        expect(rc == MSR_ERR_INVALID, b.says);
        expect(strstr(why, "msr_match_sets") && strstr(why, b.says), b.says);
    }
    // a short buffer is terminated and not overrun; none at all is not written
    char tiny[8];
    memset(tiny, 'x', sizeof tiny);
    expect(msr_match_args_check(N, -1, true, W, 0, false, 0, tiny, 4) == MSR_ERR_INVALID && strlen(tiny) == 3 && tiny[4] == 'x',
           "a short reason buffer");
    expect(msr_match_args_check(N, -1, true, W, 0, false, 0, nullptr, 0) == MSR_ERR_INVALID, "no reason buffer");
    // the largest index a row of int64 words can describe
    expect(msr_match_args_check(INT64_MAX - 31, 1, true, (INT64_MAX - 31 + 31) / 32, 0, false, 0, why, sizeof why) == MSR_OK,
           "n_docs near the top of int64");
    if (failures) return 1;
    printf("match args ok\n");
    return 0;
}
