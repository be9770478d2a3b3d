// TEST INFRASTRUCTURE: the owning buffer and handle types of sentinel_amd/csrc/devmem.h over counting stub
// allocators (host memory, no GPU). Stand-alone program; tests/test_devmem.py builds it with ASan + UBSan and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "../../sentinel_amd/csrc/devmem.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// Counts every allocation and free, knows the live set (a double free or a free of a foreign pointer is an error),
// and fails on request.
struct Counting {
    static inline int allocs = 0, frees = 0, bad_frees = 0;
    static inline bool fail_next = false;
    static inline std::set<void*> live;
    static bool alloc(void** p, size_t bytes) {
        if (fail_next) {
            fail_next = false;
            return false;
        }
        *p = std::malloc(bytes ? bytes : 1);
        if (!*p) return false;
        ++allocs;
        live.insert(*p);
        return true;
    }
    static void free(void* p) {
        if (!live.erase(p)) {
            ++bad_frees;
            return;
        }
        ++frees;
        std::free(p);
    }
    static void reset_counts() {
        allocs = frees = bad_frees = 0;
        fail_next = false;
    }
};
struct CountingPinned : Counting {};  // a second instantiation, as DevBuf / PinnedBuf are

template <class T>
using Dev = sg::OwnedBuf<T, Counting>;
template <class T>
using Pinned = sg::OwnedBuf<T, CountingPinned>;

int handle_destroys = 0;
int destroy_handle(int* h) {
    ++handle_destroys;
    delete h;
    return 0;
}
using Handle = sg::UniqueHandle<int*, int, destroy_handle>;

template <template <class> class Buf>
void buffer_checks() {
    Counting::reset_counts();
    {
        Buf<uint64_t> a;
        CHECK(a.get() == nullptr && a.size() == 0 && !a);
        CHECK(a.alloc(100));
        CHECK(a.get() != nullptr && a.size() == 100);
        a[99] = 7;  // the whole allocation is writable (ASan checks the bound)
        uint64_t* raw = a;
        CHECK(raw == a.get());

        // move construction and move assignment leave the source empty
        Buf<uint64_t> b(std::move(a));
        CHECK(a.get() == nullptr && a.size() == 0);
        CHECK(b.get() == raw && b.size() == 100 && b[99] == 7);
        Buf<uint64_t> c;
        CHECK(c.alloc(5));
        c = std::move(b);  // frees c's own allocation
        CHECK(b.get() == nullptr && b.size() == 0);
        CHECK(c.get() == raw && c.size() == 100);
        CHECK(Counting::allocs == 2 && Counting::frees == 1);
        Buf<uint64_t>& self = c;
        c = std::move(self);  // self-move keeps the allocation
        CHECK(c.get() == raw && c.size() == 100);

        // reserve within the size does not reallocate; beyond it, it does, and the old allocation is freed
        CHECK(c.reserve(100) && c.get() == raw && Counting::allocs == 2);
        CHECK(c.reserve(1) && c.get() == raw && c.size() == 100 && Counting::allocs == 2);
        CHECK(c.reserve(101) && c.size() == 101 && Counting::allocs == 3 && Counting::frees == 2);

        // a failed reserve / alloc leaves nullptr and 0: pointer and capacity cannot disagree
        Counting::fail_next = true;
        CHECK(!c.reserve(1000));
        CHECK(c.get() == nullptr && c.size() == 0);
        CHECK(Counting::frees == 3);
        CHECK(c.reserve(10) && c.size() == 10);  // the next smaller request allocates
        Counting::fail_next = true;
        CHECK(!c.alloc(10));
        CHECK(c.get() == nullptr && c.size() == 0);

        // sizes in bytes: whole elements
        Buf<uint32_t> d;
        CHECK(d.alloc_bytes(4 * 5 + 8 * 3) && d.size() == 11);
        d.reset();
        CHECK(d.get() == nullptr && d.size() == 0);
        d.reset();  // idempotent

        // containers of buffers (the node's per-shard vectors)
        std::vector<Buf<uint8_t>> v(3);
        for (auto& x : v) CHECK(x.alloc(16));
        v.resize(8);
        v.clear();

        Buf<uint64_t> e;
        CHECK(e.alloc(3));  // freed at scope exit
    }
    CHECK(Counting::allocs == Counting::frees);
    CHECK(Counting::bad_frees == 0);
    CHECK(Counting::live.empty());
}

void handle_checks() {
    handle_destroys = 0;
    {
        Handle a;
        CHECK(a.get() == nullptr);
        *a.put() = new int(1);
        int* raw = a;
        Handle b(std::move(a));
        CHECK(a.get() == nullptr && b.get() == raw);
        Handle c;
        *c.put() = new int(2);
        c = std::move(b);
        CHECK(handle_destroys == 1 && b.get() == nullptr && c.get() == raw);
        *c.put() = new int(3);  // put() on a live handle destroys it first
        CHECK(handle_destroys == 2);
    }
    CHECK(handle_destroys == 3);
}

}  // namespace

int main() {
    buffer_checks<Dev>();
    buffer_checks<Pinned>();
    handle_checks();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::puts("OK");
    return 0;
}
