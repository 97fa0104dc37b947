// Stand-alone check of csrc/msr_devmem.h on the CPU: the lifetime groups over a counting host allocator whose n-th
// allocation can be made to fail.  Built and run by tests/test_devmem.py (with the host sanitizers); exit status 0 = pass.
#include <stdio.h>
#include <stdlib.h>

#include "msr_devmem.h"

static int g_live = 0;        // allocations not yet freed
static int g_calls = 0;       // alloc calls so far
static int g_fail_at = 0;     // the g_fail_at-th alloc call fails (0: none)

struct HostMem {
    static int alloc(void** p, size_t bytes) {
        if (++g_calls == g_fail_at) { *p = (void*)0x1; return 2; }     // a failing allocator may leave rubbish behind
        *p = malloc(bytes ? bytes : 1);
        ++g_live;
        return 0;
    }
    static void free(void* p) { ::free(p); --g_live; }
};
using Group = DevGroup<HostMem>;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) { printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

struct Slots { float* a = nullptr; void* b = nullptr; int* c = nullptr; };

// scoped temporaries on an early return: `fail` makes the second allocation fail
static int with_temporaries(bool fail) {
    DevTemp<HostMem, double> t0;
    DevTemp<HostMem, int> t1;
    if (t0.alloc(64) != 0) return -1;
    t0.p[7] = 1.0;
    if (fail) g_fail_at = g_calls + 1;
    if (t1.alloc(32) != 0) return t1.p ? -3 : -2;           // early return: t0 must not leak
    t1.p[7] = 1;
    return 0;
}

int main() {
    Slots s;
    {
        Group g;
        // alloc fills the slot and bytes() adds up
        CHECK(g.alloc(&s.a, 100) == 0 && s.a && g.bytes() == 100 && g_live == 1);
        CHECK(g.alloc(&s.b, 28) == 0 && s.b && g.bytes() == 128 && g_live == 2);
        s.a[24] = 1.0f;                                     // (the memory is usable: the sanitizer watches)
        // a failing alloc leaves the slot null and bytes() unchanged
        g_fail_at = g_calls + 1;
        s.c = (int*)&s;
        CHECK(g.alloc(&s.c, 40) == 2 && s.c == nullptr && g.bytes() == 128 && g_live == 2);
        CHECK(g.alloc(&s.c, 40) == 0 && s.c && g.bytes() == 168 && g_live == 3);
        // free_one nulls its slot only; a slot without an allocation is left alone
        g.free_one(&s.b);
        CHECK(s.b == nullptr && s.a && s.c && g.bytes() == 140 && g_live == 2);
        g.free_one(&s.b);
        CHECK(g.bytes() == 140 && g_live == 2);
        // grow: free_one, then alloc into the same slot
        g.free_one(&s.a);
        CHECK(g.alloc(&s.a, 1000) == 0 && s.a && g.bytes() == 1040 && g_live == 2);
        // release() nulls every slot, brings the counter and bytes() to zero, and is harmless twice
        g.release();
        CHECK(!s.a && !s.b && !s.c && g.bytes() == 0 && g_live == 0);
        g.release();
        CHECK(g.bytes() == 0 && g_live == 0);
        // a group may be used again after release
        CHECK(g.alloc(&s.b, 16) == 0 && s.b && g.bytes() == 16 && g_live == 1);
        CHECK(g.alloc(&s.c, 8) == 0 && s.c && g.bytes() == 24 && g_live == 2);
    }
    // the destructor released (and nulled the slots, which outlive the group here)
    CHECK(g_live == 0 && !s.b && !s.c);
    // the scoped temporary frees on the normal path and on an early return
    CHECK(with_temporaries(false) == 0 && g_live == 0);
    CHECK(with_temporaries(true) == -2 && g_live == 0);
    // two groups over the same struct of slots are independent
    {
        Group g1, g2;
        CHECK(g1.alloc(&s.a, 4) == 0 && g2.alloc(&s.b, 8) == 0 && g_live == 2);
        g1.release();
        CHECK(!s.a && s.b && g1.bytes() == 0 && g2.bytes() == 8 && g_live == 1);
    }
    CHECK(g_live == 0 && !s.b);
    printf("devmem ok\n");
    return 0;
}
