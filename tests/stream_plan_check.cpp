// Stand-alone check of csrc/msr_stream_plan.h on the CPU: the capacities of a binding, the plan of a call and the kernel
// instance of every launch against a table written out here, the sample rule against both of its written-out forms.  Built
// and run by tests/test_stream_plan.py (with the host sanitizers); exit status 0 = pass.  With the argument "shapes" it
// prints pass_shape over a fixed enumeration instead, a line per case, for tests/test_dense_segments_host.py to compare with
// its numpy restatement.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>

#include "msr_stream_plan.h"

#define CHECK(cond)                                                                                                   \
    do {                                                                                                              \
        if (!(cond)) {                                                                                                \
            printf("%s:%d: CHECK(%s) failed at max_queries=%d n_cus=%d copy=%d image=%d nq=%d nt=%d\n", __FILE__,     \
                   __LINE__, #cond, mq, n_cus, copy, image, nq, nt);                                                  \
            exit(1);                                                                                                  \
        }                                                                                                             \
    } while (0)

// The capacities, a row per max_queries.
struct WantCaps { int groups, max_nt, wv_cap, tmax_row, want_copy, want_image, call_cap, width; };
static WantCaps want_caps(int mq) {
    const int groups = std::min(8, std::max(mq, 128) / 128);
    const int max_nt = std::max(1, std::min(4, groups / 2));
    WantCaps w;
    w.groups = groups;
    w.max_nt = max_nt;
    w.wv_cap = 4096 * std::max(1, groups / 2);
    w.tmax_row = groups >= 2 ? 256 * max_nt : 128;
    w.want_copy = groups >= 2;
    w.want_image = max_nt >= 2;
    w.call_cap = groups >= 2 ? (groups & ~1) * 128 : 128;
    w.width = groups >= 2 ? 256 : 128;
    return w;
}

// The plan of a call.
struct WantPlan { int valid, W, G, NT, image16, tiled, tmax_parts, entry_tmax; StreamQimg qimg; };
static WantPlan want_plan(const WantCaps& c, int n_cus, int nq, int copy, int image) {
    WantPlan w;
    w.W = nq > 128 ? 256 : 128;
    w.G = (nq + w.W - 1) / w.W;
    w.valid = nq >= 1 && w.G * w.W <= 128 * c.groups;
    w.NT = w.W == 256 && n_cus % 8 == 0 ? std::min(std::min(w.G, c.max_nt), n_cus / 8) : 1;
    w.image16 = w.W == 256 && w.NT > 1 && image;
    w.tiled = w.W == 256 && copy && !w.image16;
    w.tmax_parts = w.image16 ? 1 : 8;
    w.entry_tmax = w.W == 256 && !w.image16;
    w.qimg = w.image16 ? STREAM_QIMG_256_IMAGE16 : w.W == 256 ? STREAM_QIMG_256 : STREAM_QIMG_128;
    return w;
}
static StreamKernel want_kernel(const WantPlan& w, int nt) {
    if (w.image16) return STREAM_IMAGE16;
    if (w.W == 128) return STREAM_128;
    if (w.tiled && nt == 1) return STREAM_COPY_NT;
    if (w.tiled) return STREAM_COPY;
    return STREAM_ROWS;
}

static const int KS[7] = {1, 3, 10, 25, 100, 250, 1000};
static int shape_T(int i) { const int big[4] = {5000, 20100, 40000, 200000}; return i < 1200 ? i + 1 : big[i - 1200]; }

static int print_shapes() {
    for (int i = 0; i < 1204; ++i)
    for (int k : KS)
    for (int grid : {8, 64, 250, 256, 304})
    for (int single = 0; single < 2; ++single) {
        const int T = shape_T(i);
        if (T < 2 * k) continue;
        const PassShape p = pass_shape(T, k, grid, single != 0);
        if (p.n_seg < 1 || p.n_seg > 2 || p.bound[0] != 0 || p.bound[p.n_seg] != T) return 1;
        printf("%d %d %d %d : %d %d %d %d\n", T, k, grid, single, p.ss, p.n_s, p.n_seg, p.n_seg == 2 ? p.bound[1] : 0);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "shapes")) return print_shapes();
    static_assert(STREAM_WAVES == 8, "both kernels run 8 waves per workgroup");
    static_assert(stream_case(STREAM_IMAGE16, false) != stream_case(STREAM_128, true), "switch labels are distinct");
    long cases = 0;
    int n_cus = 0, copy = 0, image = 0, nq = 0, nt = 0;                    // (for CHECK's message)
    for (int mq : {1, 32, 128, 255, 256, 384, 512, 640, 768, 1024, 4096}) {
        const WantCaps wc = want_caps(mq);
        const StreamCaps c = stream_caps(mq);
        CHECK(c.groups == wc.groups && c.max_nt == wc.max_nt && c.wv_cap == wc.wv_cap && c.tmax_row == wc.tmax_row);
        CHECK(c.want_copy == (wc.want_copy != 0) && c.want_image == (wc.want_image != 0));
        CHECK(c.call_cap == wc.call_cap && c.width == wc.width);
        // the call capacity fits the per-query arrays and is whole groups of the width it runs at
        CHECK(c.call_cap <= 128 * c.groups && c.groups <= 8 && (c.width == 128 || c.call_cap % 256 == 0));
        for (int n_cus_ : {8, 60, 64, 250, 256, 304})
        for (copy = 0; copy < 2; ++copy)
        for (image = 0; image < 2; ++image)
        for (nq = 1; nq <= c.call_cap + 1; ++nq) {
            n_cus = n_cus_; nt = 0;
            const WantPlan w = want_plan(wc, n_cus, nq, copy, image);
            const StreamPlan p = stream_plan(c, n_cus, nq, copy != 0, image != 0);
            ++cases;
            // 1. the table
            CHECK(p.valid == (w.valid != 0) && p.W == w.W && p.G == w.G && p.NT == w.NT);
            CHECK(p.image16 == (w.image16 != 0) && p.tiled == (w.tiled != 0) && p.tmax_parts == w.tmax_parts);
            CHECK(p.entry_tmax == (w.entry_tmax != 0) && p.qimg == w.qimg && p.nt_loads == p.tiled);
            // 2. every call up to the capacity is served, the first one beyond it is not when it needs another group
            if (nq <= c.call_cap) CHECK(p.valid);
            else CHECK(p.valid == (p.G * p.W <= 128 * c.groups));
            if (!p.valid) continue;
            // 3. the groups hold the queries; the launches fit the binding and the grid
            CHECK(p.G * p.W >= nq && p.NT >= 1 && p.NT <= p.G);
            if (p.NT > 1) CHECK(p.NT <= c.max_nt && p.NT * 8 <= n_cus);
            CHECK(c.tmax_row >= p.W * p.NT);
            CHECK(!(p.image16 && p.tiled));
            CHECK(!p.image16 || c.want_image);
            // a binding never limits the groups of a launch below those of a call it admits (G <= max_nt): on a grid of whole
            // rounds of 8 with a round per group, a call is ONE launch per segment
            if (n_cus % 8 == 0) CHECK(p.NT == std::min(p.G, n_cus / 8));
            if (n_cus % 8 == 0 && n_cus >= 8 * p.G) CHECK(p.NT == p.G);
            // 4. the instance of every launch
            for (nt = 1; nt <= p.NT; ++nt) {
                const StreamKernel kn = stream_kernel(p, nt);
                CHECK(kn == want_kernel(w, nt));
                CHECK((kn == STREAM_COPY_NT) == (nt == 1 && p.tiled));
                CHECK((kn == STREAM_COPY || kn == STREAM_COPY_NT) == p.tiled && (kn == STREAM_IMAGE16) == p.image16);
                CHECK((kn == STREAM_128) == (p.W == 128));
                CHECK(stream_case(kn, true) == stream_case(kn, false) + 1 && stream_case(kn, false) == 2 * (int)kn);
            }
        }
    }
    // the sample rule against both written-out forms, and pass_shape's sample against it
    long samples = 0;
    for (int i = 0; i < 1204; ++i)
    for (int k : KS) {
        const int T = shape_T(i);
        if (T < 2 * k) continue;
        int mq = 0; n_cus = T; nq = k;                                      // (CHECK's message: n_cus = T, nq = k)
        int ss = T / (3 * k);
        ss = ss < 1 ? 1 : (ss > 64 ? 64 : ss);
        const StreamSample f = stream_sample(T, k, 3, 64);
        CHECK(f.ss == ss && f.n_s == (T - ss / 2 + ss - 1) / ss);
        CHECK(f.n_s >= k && f.ss / 2 + (f.n_s - 1) * f.ss < T && f.ss / 2 + f.n_s * f.ss >= T);
        int sb = T / (8 * k);
        sb = sb < 1 ? 1 : (sb > 16 ? 16 : sb);
        const StreamSample b = stream_sample(T, k, 8, 16);
        CHECK(b.ss == sb && b.n_s == (T - sb / 2 + sb - 1) / sb);
        const PassShape p = pass_shape(T, k, 256, false);
        CHECK(p.ss == f.ss && p.n_s == f.n_s);
        ++samples;
    }
    printf("stream plan ok (%ld calls, %ld samples)\n", cases, samples);
    return 0;
}
