// clc_buf.h -- the owners of the library's device memory, pinned memory and events (not installed).  Whoever holds one as a member or a
// local frees it by going out of scope: there is no list of buffers to keep anywhere.
#ifndef CLC_BUF_H
#define CLC_BUF_H

#include <cstddef>
#ifndef CLC_BUF_NO_HIP      // (tests/host/buf_host_lib.cpp builds Buf over counting traits with the host compiler alone)
#include <hip/hip_runtime.h>
#endif

namespace clc {

// One block of memory of Traits' kind and its size.  Traits: Err (a status type whose value-initialised state is success),
// static Err alloc(void**, size_t), static Err free(void*).  Move-only; a moved-from buffer is empty.
template <class Traits> struct Buf {
    using Err = typename Traits::Err;
    void* ptr = nullptr;
    size_t bytes = 0;          // capacity (0 while empty)
    Buf() = default;
    Buf(Buf&& o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr; o.bytes = 0; }
    Buf& operator=(Buf&& o) noexcept { if (this != &o) { (void)reset(); ptr = o.ptr; bytes = o.bytes; o.ptr = nullptr; o.bytes = 0; } return *this; }
    ~Buf() { (void)reset(); }
    Err reset() { const Err e = ptr ? Traits::free(ptr) : Err(); ptr = nullptr; bytes = 0; return e; }
    // on an empty buffer; a failure leaves it empty
    Err alloc(size_t n) { const Err e = Traits::alloc(&ptr, n); if (e == Err()) bytes = n; else ptr = nullptr; return e; }
    // Room for `need` bytes: a buffer that has it stays as it is; any other is freed and allocated anew with need + need * num / den
    // bytes, so its contents do not survive.  (clc::grow, clc_ctx.h, puts the context's stream synchronisation and error text round it.)
    Err grow(size_t need, size_t num, size_t den)
    {
        if (need <= bytes) return Err();
        const Err e = reset();
        return e == Err() ? alloc(need + need * num / den) : e;
    }
    template <class T> T* as() const { return (T*)ptr; }
    explicit operator bool() const { return ptr != nullptr; }
};


#ifndef CLC_BUF_NO_HIP
struct DevTraits {
    using Err = hipError_t;
    static Err alloc(void** p, size_t n) { return hipMalloc(p, n); }
    static Err free(void* p) { return hipFree(p); }
};
struct PinTraits {
    using Err = hipError_t;
    static Err alloc(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
    static Err free(void* p) { return hipHostFree(p); }
};
using DevBuf = Buf<DevTraits>;
using PinBuf = Buf<PinTraits>;

// An event, created on first use.  Move-only.
struct Event {
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : ev(o.ev) { o.ev = nullptr; }
    Event& operator=(Event&& o) noexcept { if (this != &o) { (void)reset(); ev = o.ev; o.ev = nullptr; } return *this; }
    ~Event() { (void)reset(); }
    hipError_t reset() { const hipError_t e = ev ? hipEventDestroy(ev) : hipSuccess; ev = nullptr; return e; }
    hipError_t create(unsigned flags) { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, flags); }
    operator hipEvent_t() const { return ev; }
};
#endif

} // namespace clc
#endif
