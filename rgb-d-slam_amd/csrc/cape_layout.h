// One walk per carve: a layout function lays the arrays of an LDS carve (or of a scratch block in HBM) out as byte offsets, the
// kernel turns the offsets into pointers, and the host sizes the launch from the same walk's `bytes`.  No pointers inside, so the
// host and the device run it alike, and the kernel's carve and the launch's byte count cannot drift apart.
#pragma once
#include <cassert>
#include <cstddef>

#include <hip/hip_runtime.h>

namespace cape {

// a layout's own consistency checks (an alias fits the region it borrows) run on the host, which walks every layout to size its
// launch; the device's walk is the same function, constant-folded
#ifdef __HIP_DEVICE_COMPILE__
#define CAPE_LAYOUT_CHECK(cond) ((void)0)
#else
#define CAPE_LAYOUT_CHECK(cond) assert(cond)
#endif

struct Layout
{
    size_t off = 0;
    // `count` T at the next multiple of `align` bytes; returns their offset
    template <typename T> __host__ __device__ constexpr size_t take(size_t count, size_t align = alignof(T))
    {
        off = (off + align - 1) & ~(align - 1);
        const size_t at = off;
        off += count * sizeof(T);
        return at;
    }
    // `count` T at the same offset as the region [at, end) laid out before, which is dead whenever they are live
    template <typename T> __host__ __device__ constexpr size_t alias(size_t at, size_t count, size_t end) const
    {
        CAPE_LAYOUT_CHECK(at + count * sizeof(T) <= end);
        return at;
    }
    // the size of the whole carve, rounded up to `align`
    __host__ __device__ constexpr size_t end(size_t align = 16) const { return (off + align - 1) & ~(align - 1); }
};

// Typed pointer into a carve.  Offsets are aligned as offsets and added to the extern __shared__ base: an integer cast of an LDS
// pointer loses its address space, and every access through the result becomes a flat_* load that waits for vmcnt and lgkmcnt.
template <typename T> __host__ __device__ __forceinline__ T* carve_at(unsigned char* base, size_t off) { return reinterpret_cast<T*>(base + off); }

} // namespace cape
