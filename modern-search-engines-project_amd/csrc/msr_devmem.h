// Device allocations owned by lifetime (host-only, used by msr_engine.hip).  A DevGroup frees together what dies together:
// every allocation goes into exactly one group, and releasing the group nulls every pointer it handed out, so there is no
// free list to keep in step with the allocation sites.
//
// The allocator A is a policy with two static functions, `status alloc(void** p, size_t bytes)` and `void free(void* p)`;
// success is the zero value of its status type (hipSuccess).  The engine uses hipMalloc / hipFree, tests/devmem_check.cpp a
// counting host allocator.
#pragma once
#include <stddef.h>

#include <vector>

template <class A>
class DevGroup {
    struct Rec { void** slot; void* p; size_t bytes; };
    std::vector<Rec> recs_;

  public:
    DevGroup() = default;
    DevGroup(const DevGroup&) = delete;
    DevGroup& operator=(const DevGroup&) = delete;
    ~DevGroup() { release(); }

    // *slot <- a new allocation of `bytes`.  The group keeps the slot's ADDRESS to null it on release, so a slot must neither
    // move nor die while the group holds its allocation: the engine's slots are members of the heap-allocated msr_engine,
    // which never moves and outlives its groups' contents.  On failure *slot is null, nothing is recorded and the allocator's
    // status comes back.  A slot that still holds an allocation is given to free_one() first.
    template <class T>
    auto alloc(T** slot, size_t bytes) {
        void* p = nullptr;
        auto err = A::alloc(&p, bytes);
        if (err != decltype(err)()) p = nullptr;
        *slot = (T*)p;
        if (p) recs_.push_back(Rec{(void**)slot, p, bytes});
        return err;
    }
    // frees the allocation that `slot` holds (none: nothing happens) and nulls that slot only
    template <class T>
    void free_one(T** slot) {
        for (size_t i = 0; i < recs_.size(); ++i)
            if (recs_[i].slot == (void**)slot) {
                A::free(recs_[i].p);
                *slot = nullptr;
                recs_.erase(recs_.begin() + i);
                return;
            }
    }
    // frees every allocation and nulls every slot; the group can be used again
    void release() {
        for (const Rec& r : recs_) {
            A::free(r.p);
            *r.slot = nullptr;
        }
        recs_.clear();
    }
    size_t bytes() const {
        size_t total = 0;
        for (const Rec& r : recs_) total += r.bytes;
        return total;
    }
};

// A scoped temporary: one allocation that is freed at the end of the scope, on every path out of it.
template <class A, class T>
struct DevTemp {
    T* p = nullptr;                    // (declared before the group: it outlives it)
    DevGroup<A> group;
    auto alloc(size_t bytes) { return group.alloc(&p, bytes); }
};
