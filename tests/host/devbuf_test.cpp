// Stand-alone test of DevBuf<T> (circom_amd/csrc/cw_devbuf.h) over a counting malloc / free: every allocation is freed
// exactly once, whatever the sequence of alloc / grow / reset / moves.  tests/test_devbuf.py builds it with
// -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

typedef int hipError_t;
static const hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2;

static long n_alloc = 0, n_free = 0;
static bool fail_next = false;
static hipError_t count_malloc(void **p, size_t n) {
    if (fail_next) {
        fail_next = false;
        return hipErrorOutOfMemory;
    }
    *p = malloc(n ? n : 1);
    n_alloc++;
    return hipSuccess;
}
static hipError_t count_free(void *p) {
    free(p);
    n_free++;
    return hipSuccess;
}
#define CW_DEVBUF_MALLOC count_malloc
#define CW_DEVBUF_FREE count_free
#include "../../circom_amd/csrc/cw_devbuf.h"

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
            return 1;                                                   \
        }                                                               \
    } while (0)

static int run() {
    {
        DevBuf<unsigned> empty;                        // destruction of an empty holder
        CHECK(!empty && empty.get() == nullptr);
    }
    CHECK(n_alloc == 0 && n_free == 0);
    {
        DevBuf<unsigned> a;
        CHECK(a.alloc(64) == hipSuccess && a);
        unsigned *p = a;                               // implicit conversion; the memory is usable
        memset(p, 0xAB, 64);
        CHECK(a[15] == 0xABABABABu && a + 1 == p + 1);
        CHECK(n_alloc == 1 && n_free == 0);
        CHECK(a.alloc(128) == hipSuccess);             // alloc over a held buffer frees it
        CHECK(n_alloc == 2 && n_free == 1);
        memset(a, 0, 128);
        p = a;
        CHECK(a.grow(16) == hipSuccess && a == p);     // smaller: kept
        CHECK(a.grow(128) == hipSuccess && a == p);    // equal: kept
        CHECK(n_alloc == 2 && n_free == 1);
        CHECK(a.grow(129) == hipSuccess);              // larger: freed and allocated anew
        CHECK(n_alloc == 3 && n_free == 2);
        memset(a, 0, 129);
        CHECK(a.grow(128) == hipSuccess);              // the capacity is the new one
        CHECK(n_alloc == 3 && n_free == 2);
        a.reset();
        CHECK(!a && n_free == 3);
        a.reset();                                     // twice
        CHECK(!a && n_free == 3);
        CHECK(a.grow(8) == hipSuccess && a);           // grow of an empty holder allocates
        CHECK(n_alloc == 4);
    }
    CHECK(n_alloc == 4 && n_free == 4);                // the destructor freed the last one
    {
        DevBuf<unsigned> a;
        CHECK(a.alloc(32) == hipSuccess);
        unsigned *p = a;
        DevBuf<unsigned> b(std::move(a));              // move construction
        CHECK(!a && b == p && n_alloc == 5 && n_free == 4);
        CHECK(b.grow(32) == hipSuccess && b == p);     // the capacity moved with the pointer
        DevBuf<unsigned> c;
        c = std::move(b);                              // move assignment onto an empty holder
        CHECK(!b && c == p && n_free == 4);
        DevBuf<unsigned> d;
        CHECK(d.alloc(16) == hipSuccess);
        d = std::move(c);                              // ... onto one that owns memory: that memory is freed
        CHECK(!c && d == p && n_alloc == 6 && n_free == 5);
        DevBuf<unsigned> &self = d;
        d = std::move(self);                           // ... onto itself: nothing happens
        CHECK(d == p && n_free == 5);
        CHECK(a.grow(4) == hipSuccess);                // a moved-from holder is an empty one
        CHECK(n_alloc == 7);
    }
    CHECK(n_alloc == 7 && n_free == 7);
    {
        DevBuf<unsigned> a;
        fail_next = true;
        CHECK(a.alloc(64) == hipErrorOutOfMemory && !a);           // the error comes back, the holder stays empty
        CHECK(a.alloc(64) == hipSuccess);
        fail_next = true;
        CHECK(a.alloc(64) == hipErrorOutOfMemory && !a);           // over a held buffer: that one is gone, nothing is held
        CHECK(n_alloc == 8 && n_free == 8);
        CHECK(a.alloc(64) == hipSuccess);
        fail_next = true;
        CHECK(a.grow(65) == hipErrorOutOfMemory && !a);
        CHECK(a.grow(1) == hipSuccess && a);                       // the capacity was forgotten with the pointer
        CHECK(n_alloc == 10 && n_free == 9);
    }
    CHECK(n_alloc == 10 && n_free == 10);
    {
        DevBuf<void> v;                                // T = void
        CHECK(v.alloc(40) == hipSuccess);
        void *p = v;
        memset(p, 1, 40);
        CHECK(v.grow(40) == hipSuccess && v == p);
        DevBuf<void> w(std::move(v));
        CHECK(!v && w.get() == p);
        const void *cp = w;                            // T* -> const void*, as the kernel wrappers take it
        CHECK(cp == p);
    }
    CHECK(n_alloc == 11 && n_free == 11);
    return 0;
}

int main() {
    int rc = run();
    if (rc == 0 && n_alloc != n_free) {
        fprintf(stderr, "%ld allocations, %ld frees\n", n_alloc, n_free);
        rc = 1;
    }
    if (rc == 0) printf("devbuf ok: %ld allocations, %ld frees\n", n_alloc, n_free);
    return rc;
}
