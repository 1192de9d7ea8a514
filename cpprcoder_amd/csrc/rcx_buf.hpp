// rcx_buf.hpp -- what both translation units share on the host side: the check of a HIP call and the one owner of a
// device (or pinned host) allocation.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/rcx.h"

// The one place a HIP error becomes a status.  RCX_DEBUG=1 (diagnostic): say which call failed and where, on stderr; the
// status code stays the only thing a caller gets.
inline int rcx_hip_status(hipError_t e, const char* what, const char* file, int line)
{
    if (e == hipSuccess) return RCX_OK;
    if (getenv("RCX_DEBUG")) fprintf(stderr, "rcx: %s failed: %s (%s:%d)\n", what, hipGetErrorString(e), file, line);
    return RCX_E_HIP;
}
#define HIP_TRY(expr)                                                                    \
    do {                                                                                 \
        if (rcx_hip_status((expr), #expr, __FILE__, __LINE__) != RCX_OK) return RCX_E_HIP; \
    } while (0)
// Kernel launches return nothing: what they left is read once behind them, `return LAUNCHED();` or HIP_TRY(hipGetLastError()).
#define LAUNCHED() rcx_hip_status(hipGetLastError(), "a kernel launch", __FILE__, __LINE__)

// `count` elements of hipMalloc (Pinned: hipHostMalloc) memory and nothing else: it is freed with its owner.  Converts to
// T* so that it stands where the pointer stood: kernel arguments, copies, `buf + i`, `if (buf)`.
template <class T, bool Pinned = false>
class DevBuf
{
    T* p_ = nullptr;
    uint64_t count_ = 0;

public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    uint64_t count() const { return count_; }
    uint64_t bytes() const { return count_ * sizeof(T); }
    void release()
    {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        count_ = 0;
    }
    void swap(DevBuf& o)
    {
        T* p = p_; p_ = o.p_; o.p_ = p;
        const uint64_t n = count_; count_ = o.count_; o.count_ = n;
    }
    // Room for `count` elements.  Never shrinks; a growth does NOT keep the contents; after a failed one the buffer is empty.
    int reserve(uint64_t count)
    {
        if (count_ >= count) return RCX_OK;
        release();
        void** const p = reinterpret_cast<void**>(&p_);
        if ((Pinned ? hipHostMalloc(p, count * sizeof(T), hipHostMallocDefault) : hipMalloc(p, count * sizeof(T))) != hipSuccess) {
            p_ = nullptr;
            return RCX_E_NOMEM;
        }
        count_ = count;
        return RCX_OK;
    }
    // ... in steps of `least`, 2 * least, 4 * least, ... for a buffer that follows what a caller feeds it piece by piece
    int reserve_pow2(uint64_t count, uint64_t least)
    {
        if (count_ >= count) return RCX_OK;
        while (least < count) least *= 2;
        return reserve(least);
    }
};
template <class T>
using PinBuf = DevBuf<T, true>;
