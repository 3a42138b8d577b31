#pragma once
// vrt_handle.h — the owner of one runtime handle (an event, a stream, a pinned allocation): null by default, destroyed by the
// destructor.  P is the policy: P::T the raw handle (a pointer type), P::create(T *, args...) returns an error whose
// value-initialised state means success, P::destroy(T) gives the handle back (vrt_ctx.h: the HIP runtime's;
// tools/sanitize_handle.cpp: a counting one).  No HIP header is needed here.  One operation makes a handle — ensure(): what is
// made on first use is made where it is first used — and a failed creation leaves the owner null and hands the policy's error to
// the caller.  Not shared, not counted: whoever is handed the raw handle borrows it.
#include <utility>

namespace vrt {

template <typename P>
class Handle {
  public:
    using T = typename P::T;

    Handle() = default;
    Handle(const Handle &) = delete;
    Handle &operator=(const Handle &) = delete;
    Handle(Handle &&o) noexcept : h_(o.h_) { o.h_ = T{}; }
    Handle &operator=(Handle &&o) noexcept {
        if (this != &o) {
            reset();
            h_ = o.h_;
            o.h_ = T{};
        }
        return *this;
    }
    ~Handle() { reset(); }

    operator T() const { return h_; }   // launchers and the runtime's calls take the raw handle
    T get() const { return h_; }

    // create if null: nothing, not a call of the policy, if there is a handle
    template <typename... Args>
    auto ensure(Args &&...args) -> decltype(P::create((T *)nullptr, std::forward<Args>(args)...)) {
        using Err = decltype(P::create((T *)nullptr, std::forward<Args>(args)...));
        if (h_) return Err{};
        T h{};
        const Err e = P::create(&h, std::forward<Args>(args)...);
        if (e == Err{}) h_ = h;
        return e;
    }
    // destroy to null
    void reset() {
        if (h_) P::destroy(h_);
        h_ = T{};
    }

  private:
    T h_{};
};

}  // namespace vrt
