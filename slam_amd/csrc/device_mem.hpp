// device_mem.hpp -- the one owner of the memory a handle holds: a hipMalloc block, a block of the library's pool
// (common.hpp) or pinned host memory.  Move-only; the destructor frees, so a handle's `destroy` is a synchronise and a
// `delete`, and an early return gives back what the call had taken.  Kernels and the structs they read keep raw pointers.
#pragma once
#include <algorithm>
#include <utility>

#include "common.hpp"

namespace slam {

enum class Mem { Device, Pool, Pinned };

template <Mem K>
struct Owned {
    void  *p = nullptr;
    size_t cap = 0; // bytes asked for (the pool may have handed out a larger block)

    Owned() = default;
    Owned(Owned &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    Owned &operator=(Owned &&o) noexcept
    {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { release(); }

    // Who waits: hipFree and hipHostFree wait for the device themselves; pool_free never does -- whoever lets go of a
    // pool block (release, destructor, move-assignment) has made sure that no enqueued work still uses it.
    void release()
    {
        if (p) {
            if (K == Mem::Device) (void)hipFree(p);
            if (K == Mem::Pool) pool_free(p);
            if (K == Mem::Pinned) (void)hipHostFree(p);
        }
        p = nullptr;
        cap = 0;
    }
    int alloc(size_t bytes) // gives back what it held; SLAM_E_NOMEM (error text set) and empty on failure
    {
        release();
        if (!bytes) return SLAM_OK; // nothing asked for: empty
        if (K == Mem::Pool) {
            p = pool_alloc(bytes); // sets the error text itself
        } else {
            const hipError_t e = K == Mem::Device ? hipMalloc(&p, bytes) : hipHostMalloc(&p, bytes, hipHostMallocDefault);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                set_error("no %s memory for %zu bytes (%s)", K == Mem::Device ? "device" : "pinned host", bytes, hipGetErrorString(e));
                p = nullptr;
            }
        }
        if (!p) return SLAM_E_NOMEM;
        cap = bytes;
        return SLAM_OK;
    }
    // No-op while need <= cap; else the block is replaced (contents lost) by one of max(need, alloc_bytes): the growth
    // rule is the caller's.  A pool block in use goes back only after the device has finished what may still read it.
    int reserve(size_t need, size_t alloc_bytes = 0)
    {
        if (need <= cap) return SLAM_OK;
        if (K == Mem::Pool && p) SLAM_HIP(hipDeviceSynchronize());
        return alloc(std::max(need, alloc_bytes));
    }
    template <class T>
    T *as() const
    {
        return static_cast<T *>(p);
    }
};
using DevMem = Owned<Mem::Device>;
using PoolMem = Owned<Mem::Pool>;
using PinnedMem = Owned<Mem::Pinned>;

// An owner whose block is an array of T: reads as the T* it replaces (a launch still receives the raw pointer).
template <class T, Mem K = Mem::Device>
struct OwnedArray : Owned<K> {
    T *get() const { return static_cast<T *>(this->p); }
    operator T *() const { return get(); }
};

// The growth rule of the per-cloud buffers (ccicp, keyframes, ground segmentation): a quarter more than asked -- clouds
// of a sequence differ by a few per cent, and every growth is a free (which waits for the device) and an allocation.
template <Mem K>
inline int reserve_quarter(Owned<K> &b, size_t bytes)
{
    return b.reserve(bytes, bytes + bytes / 4);
}

} // namespace slam
