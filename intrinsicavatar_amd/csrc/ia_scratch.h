// Work areas: ONE layout function per caller-allocated `tmp` / `scratch`, run twice -- with base == nullptr by the ia_*_bytes
// query (measure) and with the caller's pointer by the entry point (carve) -- so that the size and the pointers cannot disagree.
// Plain C++17, no HIP: a host-only program can include it (tests/scratch_harness.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace ia {

class Carver {
public:
    explicit Carver(void* base, size_t bytes = SIZE_MAX) : base_(reinterpret_cast<uintptr_t>(base)), bytes_(bytes) {}

    // the next `count` elements of T at the next ADDRESS (base + offset, not the offset alone) that is a multiple of `align`
    // (a power of two); nullptr when measuring
    template <class T> T* take(size_t count, size_t align = 256)
    {
        const uintptr_t at = (base_ + used_ + align - 1) & ~static_cast<uintptr_t>(align - 1);
        used_ = static_cast<size_t>(at - base_) + count * sizeof(T);
        if (align > max_align_) max_align_ = align;
        return base_ ? reinterpret_cast<T*>(at) : nullptr;
    }

    // offsets, not addresses, where the caller reads a piece through a published offset: round used() up to a multiple of `align`
    void align_to(size_t align) { used_ = (used_ + align - 1) & ~(align - 1); if (align > max_align_) max_align_ = align; }
    // `bytes` that belong to no piece: gaps and tail slack that the hand-written layouts had and that callers' allocations keep
    void skip(size_t bytes) { used_ += bytes; }

    size_t used() const { return used_; }                  // bytes from base to the end of the last piece
    bool fits() const { return used_ <= bytes_; }          // carve mode: the pieces lie inside the caller's `bytes`

    // what a *_bytes query returns after a measuring pass: used() + the worst-case padding in front of the first piece when the
    // entry point asks no more than `base_align` of its pointer (the end of a carve moves by at most max align - base_align:
    // the end address is monotone in the base address and shifts with it by whole multiples of the largest alignment)
    size_t need(size_t base_align) const { return used_ + (max_align_ > base_align ? max_align_ - base_align : 0); }

private:
    uintptr_t base_;
    size_t bytes_, used_ = 0, max_align_ = 1;
};

}  // namespace ia
