// clc_carve.h -- the cursor every workspace block is laid out with (not installed; no HIP).  A layout is ONE function that takes arrays
// from a cursor in order (clc_layout.h); it is run on a cursor without a base to measure the block and on the allocation to place it
// (carve_block, clc_ctx.h), so a block's size and its pointers cannot disagree.
#ifndef CLC_CARVE_H
#define CLC_CARVE_H

#include <stddef.h>
#include <stdint.h>

namespace clc {

// A base address (0: measuring -- every pointer handed out is null and only bytes() is of use) and a running offset.  Offsets are
// integers relative to the base, which the allocators align to 256 bytes or more; `align` is a power of two.
struct Carve {
    uintptr_t base = 0;
    size_t off = 0;
    Carve() = default;
    explicit Carve(void* p) : base((uintptr_t)p) {}
    // `bytes` bytes at the next multiple of `align`: for records whose type is private to one translation unit
    void* take_bytes(size_t bytes, size_t align)
    {
        const size_t at = (off + align - 1) & ~(align - 1);
        off = at + bytes;
        return base ? (void*)(base + at) : nullptr;
    }
    template <class T> T* take(size_t count, size_t align = alignof(T)) { return (T*)take_bytes(count * sizeof(T), align); }
    size_t bytes() const { return off; }
};

inline size_t up64(size_t v) { return (v + 63) & ~(size_t)63; }      // counts rounded to the 64-entry granule of the blocks

} // namespace clc
#endif
