// tools/sanitize_handle.cpp — vrt::Handle (voxelraytracing_amd/csrc/vrt_handle.h, the owner of the context's events, streams and
// pinned ring) under AddressSanitizer + UBSan, as a program of its own: over a counting policy (malloc underneath, so a double
// destroy or a leak is the sanitizer's to report as well) that can be told to fail its k-th creation.  Every created handle
// destroyed exactly once by the end; ensure() on a live handle calls nothing; a failed ensure() leaves the owner null and
// destroys nothing; a moved-from owner destroys nothing, move-assignment destroys the target's old handle, self-move keeps it;
// reset() twice destroys once; a vector of arrays of four owners (vrt_ctx::ev_pool) grows by reallocation; and the two error
// paths of the backend with the failure at each creation in turn: two local owners (ensure_accel_world's timing pair) and four
// events that join the pool whole or not at all (next_events).
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
//       -o /tmp/sanitize_handle tools/sanitize_handle.cpp && /tmp/sanitize_handle
#include <array>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <type_traits>
#include <utility>
#include <vector>

#include "../voxelraytracing_amd/csrc/vrt_handle.h"

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); std::exit(1); } } while (0)

struct Counting {
    using T = int *;
    static inline int creates = 0, destroys = 0, failed = 0, fail_at = 0;   // fail_at: the creation (1-based, since reset) that fails; 0: none
    static inline unsigned last_flags = 0;
    static inline std::set<T> live;
    static void reset(int fail) { CHECK(live.empty()); creates = destroys = failed = 0; fail_at = fail; last_flags = 0; }
    static int calls() { return creates + destroys; }
    static int create(T *h, unsigned flags = 2u) {   // (a default argument, as the event policy's untimed flag)
        creates++;
        last_flags = flags;
        if (creates == fail_at) { failed++; return 2; }
        *h = static_cast<T>(std::malloc(sizeof(int)));
        CHECK(*h && live.insert(*h).second);
        return 0;
    }
    static void destroy(T h) {
        destroys++;
        CHECK(live.erase(h) == 1);   // destroyed once, and only what was created
        std::free(h);
    }
};
using H = vrt::Handle<Counting>;
using Four = std::array<H, 4>;
static_assert(!std::is_copy_constructible<H>::value && !std::is_copy_assignable<H>::value, "move-only");
static_assert(std::is_nothrow_move_constructible<Four>::value, "a vector of them moves its elements when it grows");

static long g_cases = 0;
static void done() {   // the end of a case: nothing alive, each successful creation destroyed once
    CHECK(Counting::live.empty());
    CHECK(Counting::destroys == Counting::creates - Counting::failed);
    g_cases++;
}

static void one_owner(int fail) {   // fail: 0 none, 1 the first creation
    Counting::reset(fail);
    {
        H h;
        CHECK(!h && h.get() == nullptr && static_cast<int *>(h) == nullptr && Counting::calls() == 0);
        const int e = h.ensure();
        CHECK(Counting::creates == 1 && Counting::last_flags == 2u);
        if (fail == 1) {
            CHECK(e == 2 && !h && Counting::destroys == 0);   // null, and nothing destroyed
            CHECK(h.ensure(5u) == 0 && Counting::creates == 2 && Counting::last_flags == 5u);   // (the next attempt creates, with its flags)
        } else {
            CHECK(e == 0 && h);
        }
        int *const p = h;
        *p = 7;   // the handle is the policy's, alive
        const int n0 = Counting::calls();
        CHECK(h.ensure() == 0 && h.ensure(9u) == 0 && Counting::calls() == n0 && h.get() == p);   // live: no policy call at all
        // moves: the source is left null and destroys nothing, the target's old handle goes
        H m(std::move(h));
        CHECK(!h && m.get() == p && Counting::calls() == n0);
        h.reset();
        CHECK(Counting::calls() == n0);
        H t;
        CHECK(t.ensure() == 0);
        const int d0 = Counting::destroys;
        t = std::move(m);
        CHECK(Counting::destroys == d0 + 1 && !m && t.get() == p);
        H &self = t;
        t = std::move(self);   // (self-move keeps it)
        CHECK(t.get() == p && Counting::destroys == d0 + 1);
        t.reset();
        t.reset();
        CHECK(!t && Counting::destroys == d0 + 2);
        CHECK(t.ensure() == 0 && t);   // (and lives again; the destructor takes this one)
    }
    done();
}

// std::vector<std::array<Handle, 4>> as vrt_ctx::ev_pool lives: grown one quadruple at a time through many reallocations
static void pool_grows() {
    Counting::reset(0);
    {
        std::vector<Four> pool;
        std::vector<int *> raw;
        size_t reallocations = 0;
        for (int i = 0; i < 64; i++) {
            Four t;
            for (auto &e : t) CHECK(e.ensure() == 0);
            for (auto &e : t) raw.push_back(e);
            const size_t cap = pool.capacity();
            pool.push_back(std::move(t));
            reallocations += pool.capacity() != cap;
            CHECK(Counting::destroys == 0);   // neither the moved-from locals nor the vector's old storage destroy anything
        }
        CHECK(reallocations > 3 && Counting::creates == 256);
        for (size_t i = 0; i < pool.size(); i++)
            for (size_t k = 0; k < 4; k++) CHECK(pool[i][k].get() == raw[4 * i + k]);
    }
    CHECK(Counting::destroys == 256);
    done();
}

// ensure_accel_world's shape: two local owners, an early return when either creation fails
static int two_locals() {
    H e0, e1;
    if (const int e = e0.ensure(0u)) return e;
    if (const int e = e1.ensure(0u)) return e;
    CHECK(e0 && e1 && e0.get() != e1.get());
    return 0;
}

// next_events' shape: four events made as locals join the pool whole or not at all
static int next_quadruple(std::vector<Four> &pool) {
    Four t;
    for (auto &e : t)
        if (const int err = e.ensure(0u)) return err;
    pool.push_back(std::move(t));
    return 0;
}

int main() {
    one_owner(0);
    one_owner(1);
    pool_grows();
    for (int fail = 0; fail <= 2; fail++) {
        Counting::reset(fail);
        CHECK(two_locals() == (fail ? 2 : 0));
        CHECK(Counting::creates == (fail ? fail : 2) && Counting::live.empty());   // (fail = 2: the first event does not leak)
        done();
    }
    for (int fail = 0; fail <= 4; fail++) {
        Counting::reset(0);
        {
            std::vector<Four> pool;
            CHECK(next_quadruple(pool) == 0 && pool.size() == 1);
            Counting::fail_at = fail ? Counting::creates + fail : 0;
            CHECK(next_quadruple(pool) == (fail ? 2 : 0));
            CHECK(pool.size() == (fail ? 1u : 2u));
            CHECK(Counting::live.size() == 4u * pool.size());   // what a failed quadruple had made is gone already
            for (auto &t : pool)
                for (auto &e : t) CHECK(e);
        }
        done();
    }
    std::printf("sanitize_handle: ok (%ld cases)\n", g_cases);
    return 0;
}
