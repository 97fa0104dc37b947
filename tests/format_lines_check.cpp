// msr_format_lines (csrc/msr_format.cpp) on scores of 1e12 and above, infinities and NaNs, as a program of its own: built with
// the host compiler under its address / undefined-behaviour sanitizers, together with msr_format.cpp, by
// tests/test_host_logic.py.  No GPU, no ROCm runtime.  Every call gets a heap buffer of EXACTLY the bytes the sizing call asked
// for, filled with a sentinel: a write past it is the sanitizer's to report, a byte count that differs from the bytes written
// is this program's.  The lines go to stdout; the test compares them with Python's own formatting.
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "msretr.h"

static int failures = 0;

static void expect(bool ok, const char* what, int at) {
    if (!ok) {
        printf("FAILED: %s (case %d)\n", what, at);
        ++failures;
    }
}

static const char URLS[] = "https://a.de/xhttp://b.org/a/long/path?q=1";      // documents 0, 1 (no URL), 2
static const int64_t URL_OFF[] = {0, 14, 14, 42};
static const char SENTINEL = 0x7F;

// one sizing call, one formatting call into exactly `need` bytes; prints the lines
static int64_t run(int at, int32_t Q, int32_t stride, const std::vector<int32_t>& doc, const std::vector<double>& score,
                const std::vector<int32_t>& n, const char* qblob, const std::vector<int64_t>& qoff, int64_t max_url) {
    const int64_t need = -msr_format_lines(qblob, qoff.data(), Q, doc.data(), score.data(), n.data(), stride, URLS, URL_OFF, 3, max_url,
                                           nullptr, 0);
    expect(need > 0, "the sizing call returns -need", at);
    if (need <= 0) return 0;
    char* out = (char*)malloc((size_t)need);
    memset(out, SENTINEL, (size_t)need);
    const int64_t got = msr_format_lines(qblob, qoff.data(), Q, doc.data(), score.data(), n.data(), stride, URLS, URL_OFF, 3, max_url,
                                         out, need);
    expect(got > 0 && got <= need, "0 < bytes written <= need", at);
    if (got > 0 && got <= need) {
        bool clean = out[got - 1] == '\n';
        for (int64_t i = 0; i < got; ++i) clean = clean && out[i] != 0 && out[i] != SENTINEL;
        expect(clean, "the returned count covers written text only: no NUL, no untouched byte, a newline last", at);
        bool rest = true;
        for (int64_t i = got; i < need; ++i) rest = rest && out[i] == SENTINEL;
        expect(rest, "nothing is written behind the returned count", at);
        fwrite(out, 1, (size_t)got, stdout);
    }
    free(out);
    return need;
}

int main() {
    uint64_t neg_nan_bits = 0xFFF8000000000000ull;
    double neg_nan;
    memcpy(&neg_nan, &neg_nan_bits, 8);
    const double vals[] = {1e12, -1e12, 1e12 - 0.0005, 1e36, 1e308, -1e308, DBL_MAX, -DBL_MAX, INFINITY, -INFINITY, NAN, neg_nan,
                           999999999999.9994, 4503599627370496.5, 9007199254740993.0};
    const int NV = (int)(sizeof vals / sizeof vals[0]);
    const char qblob[] = "7Q-otto42";                                         // query numbers "7", "Q-otto", "42"
    const std::vector<int64_t> qoff = {0, 1, 7, 9};
    for (int v = 0; v < NV; ++v) {
        uint64_t bits;
        memcpy(&bits, &vals[v], 8);
        printf("# %016llx\n", (unsigned long long)bits);
        // three queries of three results; the value first and last in the first and the last query
        std::vector<int32_t> doc = {0, 1, 2, 2, -1, 0, 1, 3, 0}, n = {3, 2, 3};
        std::vector<double> score(9, 0.5);
        score[0] = score[2] = score[6] = score[8] = vals[v];
        score[5] = vals[v];                                                   // behind the second query's count: not formatted
        run(v, 3, 3, doc, score, n, qblob, qoff, v % 2 ? 0 : 28);             // (max_url_len given, and worked out by the call)
    }
    // every value in one list, three times over, and a sizing call that must not need the URL table
    printf("# all\n");
    std::vector<int32_t> doc(3 * NV), n = {3 * NV};
    std::vector<double> score(3 * NV);
    for (int i = 0; i < 3 * NV; ++i) { doc[i] = i % 4 - 1; score[i] = vals[i % NV]; }
    const int64_t sized = run(NV, 1, 3 * NV, doc, score, n, qblob, qoff, 28);
    const int64_t need = msr_format_lines(qblob, qoff.data(), 1, doc.data(), score.data(), n.data(), 3 * NV, nullptr, (const int64_t*)8, 3,
                                          28, nullptr, 0);
    expect(need == -sized, "pass 1 reads neither the URL bytes nor the offsets", NV);
    if (failures) return 1;
    printf("format lines ok\n");
    return 0;
}
