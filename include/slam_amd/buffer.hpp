// slam_amd/buffer.hpp -- the one owner of the device and pinned memory an adapter holds, over the C-ABI (slam_mi355x.h:
// slam_malloc / slam_free, slam_host_alloc / slam_host_free), and the adapters' one way to report the library's error.
// Move-only; the destructor frees, so an adapter's destructor deals with its handles, streams and events and nothing else.
// The library's calls keep taking raw pointers (as<T>()).
//
// When a block may be let go -- the one rule.  A block that enqueued work may still read or write is given back only behind
// slam_device_synchronize().  reserve() is the one place that replaces a block in the middle of an adapter's life, and it
// makes that call itself before it frees; release(), alloc() and the destructor free without a wait of their own, for
// owners that have waited (an adapter's destructor waits for what it enqueued before its members go) or whose block was
// never handed to the device.  Which stream used the block does not matter: the wait is for the whole device, as
// slam_free's own is.
// While need <= cap, reserve() is a comparison and nothing else.
#pragma once
#include <cstddef>
#include <cstdio>
#include <utility>

#include "slam_mi355x.h"

namespace slam_amd {
namespace detail {

enum class Kind { Device, Pinned };

template <Kind K>
struct Buffer {
    void  *p = nullptr;
    size_t cap = 0; // bytes

    Buffer() = default;
    Buffer(Buffer &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    Buffer &operator=(Buffer &&o) noexcept
    {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    Buffer(const Buffer &) = delete;
    Buffer &operator=(const Buffer &) = delete;
    ~Buffer() { release(); }

    void release()
    {
        if (p) K == Kind::Device ? slam_free(p) : slam_host_free(p);
        p = nullptr;
        cap = 0;
    }
    bool alloc(size_t bytes) // gives back what it held; empty and false on failure (slam_last_error() has the text)
    {
        release();
        if ((K == Kind::Device ? slam_malloc(&p, bytes) : slam_host_alloc(&p, bytes)) != SLAM_OK) {
            p = nullptr;
            return false;
        }
        cap = bytes;
        return true;
    }
    // No-op while need <= cap; else the block is replaced (contents lost) by one of max(need, alloc_bytes) bytes: the growth
    // rule is the caller's (reserve_quarter, reserve_half)
    bool reserve(size_t need, size_t alloc_bytes = 0)
    {
        if (need <= cap) return true;
        if (p) slam_device_synchronize(); // (the old block may be in use by enqueued work)
        return alloc(need > alloc_bytes ? need : alloc_bytes);
    }
    template <class T>
    T *as() const
    {
        return static_cast<T *>(p);
    }
};
using DeviceBuffer = Buffer<Kind::Device>;
using PinnedBuffer = Buffer<Kind::Pinned>;

// A buffer whose block is an array of T: reads as the T * it replaces (the library's calls still receive the raw pointer)
template <class T, Kind K = Kind::Device>
struct Array : Buffer<K> {
    operator T *() const { return static_cast<T *>(this->p); }
};

// a quarter more than asked: clouds of a sequence differ by a few per cent, and every growth waits for the device
template <Kind K>
inline bool reserve_quarter(Buffer<K> &b, size_t bytes)
{
    return b.reserve(bytes, bytes + bytes / 4);
}
// half more than asked: blocks that follow a growing map
template <Kind K>
inline bool reserve_half(Buffer<K> &b, size_t bytes)
{
    return b.reserve(bytes, bytes + bytes / 2);
}

// "<who>: <the library's last error>" on stderr
inline void warn(const char *who) { std::fprintf(stderr, "%s: %s\n", who, slam_last_error()); }

} // namespace detail
} // namespace slam_amd
