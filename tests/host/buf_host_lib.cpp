// Host build of the library's owning buffer type (coloc_amd/csrc/clc_buf.h: Buf<Traits>) over counting traits whose k-th allocation can be
// told to fail, as a tiny shared library for tests/test_buf_host.py.  Each exported scenario returns 0 or the number of the first check
// that failed.  Test infrastructure only.
#define CLC_BUF_NO_HIP
#include "../../coloc_amd/csrc/clc_buf.h"

#include <cstdlib>
#include <utility>

namespace {

struct Fake {
    using Err = int;
    static long calls, allocs, frees, fail_at;      // fail_at: the alloc call (1-based, counted from the last reset) that fails; 0 = none
    static Err alloc(void** p, size_t n)
    {
        if (++calls == fail_at) { *p = (void*)0x1; return 2; }      // (a failing allocator may leave rubbish in *p)
        *p = malloc(n ? n : 1);
        if (!*p) return 2;
        ++allocs;
        return 0;
    }
    static Err free(void* p) { ++frees; ::free(p); return 0; }
    static long live() { return allocs - frees; }
    static void reset(long fail) { calls = allocs = frees = 0; fail_at = fail; }
};
long Fake::calls = 0, Fake::allocs = 0, Fake::frees = 0, Fake::fail_at = 0;
using FBuf = clc::Buf<Fake>;

#define CHECK(cond) do { ++step; if (!(cond)) return step; } while (0)

} // namespace

// alloc, grow, move-construct, move-assign, reset and scope exit: live == allocations - frees throughout, 0 at the end
extern "C" int buf_host_lifetime(void)
{
    int step = 0;
    Fake::reset(0);
    {
        FBuf a;
        CHECK(!a && a.ptr == nullptr && a.bytes == 0 && Fake::live() == 0);
        CHECK(a.reset() == 0 && Fake::frees == 0);                    // an empty buffer frees nothing
        CHECK(a.alloc(100) == 0 && a.ptr && a.bytes == 100 && Fake::live() == 1);
        void* const pa = a.ptr;
        FBuf b(std::move(a));                                        // move-construct
        CHECK(b.ptr == pa && b.bytes == 100 && !a.ptr && a.bytes == 0 && Fake::live() == 1 && Fake::frees == 0);
        CHECK(a.reset() == 0 && Fake::frees == 0);                    // the moved-from buffer is empty and frees nothing
        FBuf c;
        CHECK(c.alloc(7) == 0 && Fake::live() == 2);
        c = std::move(b);                                            // move-assign over a full buffer: its block is freed
        CHECK(c.ptr == pa && c.bytes == 100 && !b.ptr && b.bytes == 0 && Fake::live() == 1 && Fake::frees == 1);
        c = std::move(c);                                            // onto itself: nothing happens
        CHECK(c.ptr == pa && c.bytes == 100 && Fake::live() == 1);
        CHECK(c.grow(101, 0, 1) == 0 && c.bytes == 101 && Fake::live() == 1 && Fake::allocs == 3 && Fake::frees == 2);
        {
            FBuf d;
            CHECK(d.alloc(1) == 0 && Fake::live() == 2);
        }                                                            // scope exit
        CHECK(Fake::live() == 1);
        CHECK(c.as<char>() == (char*)c.ptr);
        CHECK(c.reset() == 0 && !c.ptr && c.bytes == 0 && Fake::live() == 0);
        CHECK(c.alloc(5) == 0 && Fake::live() == 1);                 // (left to the destructor)
    }
    CHECK(Fake::live() == 0 && Fake::allocs == Fake::frees && Fake::allocs == 5);
    return 0;
}

// a failed allocation, first in alloc and then inside grow: the buffer is left empty, nothing leaks, nothing is freed twice
extern "C" int buf_host_failure(void)
{
    int step = 0;
    Fake::reset(1);
    {
        FBuf a;
        CHECK(a.alloc(64) != 0 && a.ptr == nullptr && a.bytes == 0 && Fake::live() == 0);
        CHECK(a.alloc(64) == 0 && a.bytes == 64 && Fake::live() == 1);          // and it is usable afterwards
    }
    CHECK(Fake::live() == 0 && Fake::frees == 1);
    Fake::reset(2);
    {
        FBuf a;
        CHECK(a.alloc(64) == 0);
        CHECK(a.grow(65, 1, 2) != 0 && a.ptr == nullptr && a.bytes == 0 && Fake::live() == 0 && Fake::frees == 1);   // old block gone, no new one
        CHECK(a.grow(10, 1, 2) == 0 && a.bytes == 15 && Fake::live() == 1);
    }
    CHECK(Fake::live() == 0 && Fake::frees == 2);
    return 0;
}

// the capacity after grow(need, num, den) on a buffer that held `have` bytes, and (through *reallocated) whether it allocated
extern "C" size_t buf_host_grow(size_t have, size_t need, size_t num, size_t den, int* reallocated, long* live_after)
{
    Fake::reset(0);
    size_t bytes;
    {
        FBuf a;
        if (have) (void)a.alloc(have);
        const long before = Fake::allocs;
        (void)a.grow(need, num, den);
        *reallocated = (int)(Fake::allocs - before);
        bytes = a.bytes;
    }
    *live_after = Fake::live();
    return bytes;
}
