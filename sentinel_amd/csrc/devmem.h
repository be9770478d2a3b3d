// devmem.h — owning types for device and pinned host memory. Plain host C++: the allocator is a template parameter
// (two static functions), so the HIP calls sit behind DevAlloc / PinnedAlloc (defined in api.cpp) and the host tests
// instantiate the same code over counting stubs (tests/cpp/test_devmem_host.cpp).
#pragma once

#include <cstddef>

namespace sg {

// One allocation of T from allocator A (bool A::alloc(void**, size_t bytes), void A::free(void*)). Move-only; frees
// in its destructor, under whatever device is current then (the owner of a buffer makes its device current before
// its members destruct). Pointer and size change together: a failed alloc / reserve leaves nullptr and 0.
template <class T, class A>
class OwnedBuf {
public:
    OwnedBuf() = default;
    OwnedBuf(const OwnedBuf&) = delete;
    OwnedBuf& operator=(const OwnedBuf&) = delete;
    OwnedBuf(OwnedBuf&& o) noexcept : p_(o.p_), n_(o.n_) {
        o.p_ = nullptr;
        o.n_ = 0;
    }
    OwnedBuf& operator=(OwnedBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_;
            n_ = o.n_;
            o.p_ = nullptr;
            o.n_ = 0;
        }
        return *this;
    }
    ~OwnedBuf() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t size() const { return n_; }  // elements

    void reset() {
        if (p_) A::free(p_);
        p_ = nullptr;
        n_ = 0;
    }
    // A fresh allocation of n elements (the old one is freed first, its contents are not kept).
    bool alloc(size_t n) { return alloc_bytes(n * sizeof(T)); }
    // The same for a size in bytes (tables of mixed layout); size() is the whole elements that fit.
    bool alloc_bytes(size_t bytes) {
        reset();
        void* p = nullptr;
        if (!A::alloc(&p, bytes)) return false;
        p_ = static_cast<T*>(p);
        n_ = p_ ? bytes / sizeof(T) : 0;
        return true;
    }
    // At least n elements, contents not kept; no new allocation when n <= size().
    bool reserve(size_t n) { return n <= n_ || alloc(n); }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

struct DevAlloc {     // hipMalloc / hipFree
    static bool alloc(void** p, size_t bytes);
    static void free(void* p);
};
struct PinnedAlloc {  // hipHostMalloc / hipHostFree
    static bool alloc(void** p, size_t bytes);
    static void free(void* p);
};

template <class T>
using DevBuf = OwnedBuf<T, DevAlloc>;
template <class T>
using PinnedBuf = OwnedBuf<T, PinnedAlloc>;

// A stream or event handle H destroyed by D (hipStreamDestroy / hipEventDestroy). put() is the out-parameter of the
// create call.
template <class H, class R, R (*D)(H)>
class UniqueHandle {
public:
    UniqueHandle() = default;
    UniqueHandle(const UniqueHandle&) = delete;
    UniqueHandle& operator=(const UniqueHandle&) = delete;
    UniqueHandle(UniqueHandle&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    UniqueHandle& operator=(UniqueHandle&& o) noexcept {
        if (this != &o) {
            reset();
            h_ = o.h_;
            o.h_ = nullptr;
        }
        return *this;
    }
    ~UniqueHandle() { reset(); }
    operator H() const { return h_; }
    H get() const { return h_; }
    H* put() {
        reset();
        return &h_;
    }
    void reset() {
        if (h_) (void)D(h_);
        h_ = nullptr;
    }

private:
    H h_ = nullptr;
};

}  // namespace sg
