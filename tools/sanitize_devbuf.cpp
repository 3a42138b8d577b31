// tools/sanitize_devbuf.cpp — vrt::DevBuf (voxelraytracing_amd/csrc/vrt_devbuf.h, the owner of the context's device buffers)
// under AddressSanitizer + UBSan, as a program of its own: over a counting allocator (malloc underneath, so a double free or a
// leak is the sanitizer's to report as well) that can be told to fail its k-th allocation.  For every operation, from an empty
// buffer and from one of 8 elements, with a growing, an equal and a shrinking request and the failure at each allocation in
// turn: every allocation freed exactly once by the end, a request that has nothing to do allocates and frees nothing, the
// buffer empty after a failure, a moved-from buffer frees nothing, the bytes asked for n * sizeof(T).
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
//       -o /tmp/sanitize_devbuf tools/sanitize_devbuf.cpp && /tmp/sanitize_devbuf
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

#include "../voxelraytracing_amd/csrc/vrt_devbuf.h"

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); std::exit(1); } } while (0)

struct Counting {
    static inline int allocs = 0, frees = 0, failed = 0, fail_at = 0;   // fail_at: the allocation (1-based, since reset) that fails; 0: none
    static inline size_t last_bytes = 0;
    static inline std::set<void *> live;
    static void reset(int fail) { CHECK(live.empty()); allocs = frees = failed = 0; fail_at = fail; last_bytes = 0; }
    static int alloc(void **p, size_t bytes) {
        allocs++;
        last_bytes = bytes;
        if (allocs == fail_at) { failed++; return 2; }   // (the caller's out-of-memory)
        *p = std::malloc(bytes ? bytes : 1);
        CHECK(*p && live.insert(*p).second);
        return 0;
    }
    static void free(void *p) {
        frees++;
        CHECK(live.erase(p) == 1);   // freed once, and only what was allocated
        std::free(p);
    }
};

struct Rec { uint64_t a, b, c; };   // 24 bytes: the byte counts are not the element counts
using Buf = vrt::DevBuf<Rec, Counting>;
enum Op { kGrow, kOnce, kExactly, kRelease, kOps };

static int apply(Buf &b, int op, size_t n) {
    switch (op) {
    case kGrow: return b.grow(n);
    case kOnce: return b.once(n);
    case kExactly: return b.exactly(n);
    default: b.release(); return 0;
    }
}
// whether the operation has to allocate, from a buffer of `have` elements (0: empty)
static bool allocates(int op, size_t have, size_t n) {
    if (op == kGrow) return n > have;
    if (op == kOnce) return have == 0;
    if (op == kExactly) return have == 0 || n != have;
    return false;
}

static long g_cases = 0;

// fail: 0 none, else the case's fail-th allocation.  From 8 elements: 1 the set-up's, 2 the operation's; from empty: 1 the operation's
static void one(int op, size_t have, size_t n, int fail) {
    Counting::reset(fail);
    {
        Buf b;
        CHECK(!b.get() && b.cap() == 0 && static_cast<Rec *>(b) == nullptr);
        if (have) {
            const int e = b.once(have);
            CHECK(Counting::allocs == 1 && Counting::last_bytes == have * sizeof(Rec));
            if (fail == 1) { CHECK(e == 2 && !b.get() && b.cap() == 0 && Counting::frees == 0); have = 0; }
            else CHECK(e == 0 && b.get() && b.cap() == have);
        }
        Rec *const before = b.get();
        const int a0 = Counting::allocs, f0 = Counting::frees;
        const bool will = allocates(op, have, n), fails = will && Counting::fail_at == a0 + 1;
        const int e = apply(b, op, n);
        Counting::fail_at = 0;   // (the moves below allocate for themselves)
        if (op == kRelease) {
            CHECK(!b.get() && b.cap() == 0 && Counting::allocs == a0 && Counting::frees == f0 + (have ? 1 : 0));
        } else if (!will) {   // nothing to do: no allocator call at all, the same memory
            CHECK(e == 0 && Counting::allocs == a0 && Counting::frees == f0 && b.get() == before && b.cap() == have);
        } else {
            CHECK(Counting::allocs == a0 + 1 && Counting::last_bytes == n * sizeof(Rec));
            CHECK(Counting::frees == f0 + (have ? 1 : 0));   // the old allocation went first
            if (fails) CHECK(e == 2 && !b.get() && b.cap() == 0);
            else CHECK(e == 0 && b.get() && b.cap() == n);
        }
        if (b.cap()) { b.get()[0].a = 1; b.get()[b.cap() - 1].c = 2; }   // the whole capacity is the buffer's to write
        // moves: the source is left empty and frees nothing, the target's old allocation goes
        Rec *const p = b.get();
        const size_t cap = b.cap();
        Buf m(std::move(b));
        CHECK(!b.get() && b.cap() == 0 && m.get() == p && m.cap() == cap);
        const int f1 = Counting::frees;
        b.release();
        CHECK(Counting::frees == f1);
        Buf t;
        CHECK(t.once(3) == 0);
        t = std::move(m);
        CHECK(Counting::frees == f1 + 1 && !m.get() && m.cap() == 0 && t.get() == p && t.cap() == cap);
        Buf &self = t;
        t = std::move(self);   // (self-assignment keeps it)
        CHECK(t.get() == p && Counting::frees == f1 + 1);
    }
    CHECK(Counting::live.empty());
    CHECK(Counting::frees == Counting::allocs - Counting::failed);   // each successful allocation freed once
    g_cases++;
}

int main() {
    const size_t requests[] = {12, 8, 5, 1, 0};   // against 8: growing, equal, shrinking, one element, none
    for (int op = 0; op < kOps; op++)
        for (size_t have : {(size_t)0, (size_t)8})
            for (size_t n : requests)
                for (int fail = 0; fail <= (have ? 2 : 1); fail++) one(op, have, n, fail);
    // a sequence, as a table buffer lives: grow, grow less, grow more, exactly the same, exactly less, release twice
    Counting::reset(0);
    {
        Buf b;
        CHECK(b.grow(4) == 0 && b.grow(2) == 0 && Counting::allocs == 1);
        CHECK(b.grow(9) == 0 && b.cap() == 9 && Counting::allocs == 2 && Counting::frees == 1);
        CHECK(b.exactly(9) == 0 && Counting::allocs == 2);
        CHECK(b.exactly(3) == 0 && b.cap() == 3 && Counting::allocs == 3 && Counting::frees == 2);
        b.release();
        b.release();
        CHECK(Counting::frees == 3);
        CHECK(b.once(2) == 0);
    }   // (the destructor frees the last one)
    CHECK(Counting::live.empty() && Counting::allocs == 4 && Counting::frees == 4);
    std::printf("sanitize_devbuf: ok (%ld cases)\n", g_cases);
    return 0;
}
