#pragma once
// vrt_devbuf.h — the owner of one device allocation: a pointer and its capacity in elements of T, freed by the destructor.
// A is the allocator: A::alloc(void **, size_t bytes) returns an error whose value-initialised state means success, A::free(void *)
// gives the memory back (vrt_ctx.h: hipMalloc / hipFree; tools/sanitize_devbuf.cpp: a counting one).  No HIP header is needed here.
// One operation per way the backend allocates; a failed allocation leaves the buffer empty (null, capacity 0) and hands the
// allocator's error to the caller.  Contents never survive a reallocation.
#include <cstddef>

namespace vrt {

template <typename T, typename A>
class DevBuf {
  public:
    using Err = decltype(A::alloc((void **)nullptr, (size_t)0));

    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            release();
            p_ = o.p_; cap_ = o.cap_;
            o.p_ = nullptr; o.cap_ = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }

    operator T *() const { return p_; }   // kernel parameters and launchers take the raw pointer
    T *get() const { return p_; }
    size_t cap() const { return cap_; }   // elements

    // grow-only, contents dropped: nothing if n elements fit
    Err grow(size_t n) { return n <= cap_ ? Err{} : fresh(n); }
    // allocate once: nothing if there is an allocation
    Err once(size_t n) { return p_ ? Err{} : fresh(n); }
    // exactly this size: nothing if there is an allocation of n elements
    Err exactly(size_t n) { return p_ && cap_ == n ? Err{} : fresh(n); }
    // release to empty
    void release() {
        if (p_) A::free(p_);
        p_ = nullptr;
        cap_ = 0;
    }

  private:
    Err fresh(size_t n) {   // free, be empty, allocate
        release();
        void *q = nullptr;
        const Err e = A::alloc(&q, n * sizeof(T));
        if (e == Err{}) { p_ = static_cast<T *>(q); cap_ = n; }
        return e;
    }
    T *p_ = nullptr;
    size_t cap_ = 0;
};

}  // namespace vrt
