// Host-side helpers shared by the POA batch and the aligner (C++ API + C ABI).
#pragma once

#include <claraparabricks/genomeworks/utils/allocator.hpp>

#include "diag_env.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>

#define GWAMD_HIP_CHECK(expr)                                                                                  \
    do                                                                                                         \
    {                                                                                                          \
        hipError_t e__ = (expr);                                                                               \
        if (e__ != hipSuccess)                                                                                 \
            throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(e__) + " at " #expr);       \
    } while (0)

namespace gwamd
{
namespace host
{

// Per-thread message of the last failed C ABI call (gwamd_last_error()).
inline std::string& last_error()
{
    thread_local std::string s;
    return s;
}

struct ScopedDevice
{
    int prev = -1;
    explicit ScopedDevice(int dev)
    {
        GWAMD_HIP_CHECK(hipGetDevice(&prev));
        if (prev != dev)
            GWAMD_HIP_CHECK(hipSetDevice(dev));
    }
    ~ScopedDevice()
    {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != prev && prev >= 0)
            (void)hipSetDevice(prev);
    }
};

class PinnedBuf
{
public:
    ~PinnedBuf() { release(); }
    void reserve(size_t bytes, hipStream_t stream)
    {
        if (bytes <= cap_)
            return;
        size_t ncap = std::max(bytes, cap_ * 2);
        void* np    = nullptr;
        GWAMD_HIP_CHECK(hipHostMalloc(&np, ncap, hipHostMallocDefault));
        if (p_)
        {
            // an async H2D copy may still read the old buffer
            GWAMD_HIP_CHECK(hipStreamSynchronize(stream));
            std::memcpy(np, p_, used_);
            (void)hipHostFree(p_);
        }
        p_   = np;
        cap_ = ncap;
    }
    template <typename T>
    T* as() const { return static_cast<T*>(p_); }
    size_t used_ = 0;

private:
    void release()
    {
        if (p_)
            (void)hipHostFree(p_);
        p_ = nullptr;
    }
    void* p_    = nullptr;
    size_t cap_ = 0;
};

using Budget = std::shared_ptr<claraparabricks::genomeworks::DeviceBudget>;

// Device array whose bytes are reserved from the caller's pool (null: no
// pool) for its lifetime; freed and released on every path out of scope.
template <typename T>
class DevBuf
{
public:
    DevBuf() = default;
    DevBuf(size_t n, const Budget& budget) { alloc(n, budget); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept { take(o); }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o)
        {
            free();
            take(o);
        }
        return *this;
    }
    ~DevBuf() { free(); }

    void alloc(size_t n, const Budget& budget)
    {
        free();
        if (n == 0)
            return;
        const int64_t bytes = int64_t(n * sizeof(T));
        if (budget && budget->reserve(bytes, bytes) < 0)
            throw std::runtime_error("Not enough memory left in the device allocator pool: " + std::to_string(bytes) +
                                     " bytes asked, " + std::to_string(budget->capacity() - budget->used()) +
                                     " of " + std::to_string(budget->capacity()) + " left.");
        void* p            = nullptr;
        const hipError_t e = hipMalloc(&p, size_t(bytes));
        if (e != hipSuccess)
        {
            (void)hipGetLastError(); // reported here: the next launch's check must not find it again
            if (budget)
                budget->release(bytes);
            throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(e) + " at hipMalloc of " +
                                     std::to_string(bytes) + " bytes");
        }
        p_      = static_cast<T*>(p);
        n_      = n;
        budget_ = budget;
    }
    void free()
    {
        if (!p_)
            return;
        (void)hipFree(p_);
        if (budget_)
            budget_->release(int64_t(n_ * sizeof(T)));
        p_ = nullptr;
        n_ = 0;
        budget_.reset();
    }
    T* data() const { return p_; }
    size_t size() const { return n_; }

private:
    void take(DevBuf& o)
    {
        p_      = o.p_;
        n_      = o.n_;
        budget_ = std::move(o.budget_);
        o.p_    = nullptr;
        o.n_    = 0;
    }
    T* p_     = nullptr;
    size_t n_ = 0;
    Budget budget_;
};

// Bytes of the caller's pool held for an object's lifetime (null pool: none).
class PoolReservation
{
public:
    PoolReservation() = default;
    PoolReservation(const PoolReservation&) = delete;
    PoolReservation& operator=(const PoolReservation&) = delete;
    ~PoolReservation() { trim(0); }
    // as much of `want` as the pool has left, at least `min_bytes`; negative: not even that (nothing held)
    int64_t reserve(const Budget& budget, int64_t min_bytes, int64_t want)
    {
        trim(0);
        const int64_t got = budget->reserve(min_bytes, want);
        if (got >= 0)
            budget_ = budget, bytes_ = got;
        return got;
    }
    // give back all but `keep` bytes
    void trim(int64_t keep)
    {
        if (budget_ && bytes_ > keep)
            budget_->release(bytes_ - keep), bytes_ = keep;
    }

private:
    Budget budget_;
    int64_t bytes_ = 0;
};

// A non-blocking stream and an event, destroyed with their owner.
class OwnedStream
{
public:
    OwnedStream() { GWAMD_HIP_CHECK(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking)); }
    OwnedStream(OwnedStream&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    OwnedStream& operator=(OwnedStream&&) = delete;
    ~OwnedStream()
    {
        if (s_)
            (void)hipStreamDestroy(s_);
    }
    operator hipStream_t() const { return s_; }

private:
    hipStream_t s_ = nullptr;
};

class OwnedEvent
{
public:
    explicit OwnedEvent(unsigned flags = hipEventDefault) { GWAMD_HIP_CHECK(hipEventCreateWithFlags(&e_, flags)); }
    OwnedEvent(OwnedEvent&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    OwnedEvent& operator=(OwnedEvent&&) = delete;
    ~OwnedEvent()
    {
        if (e_)
            (void)hipEventDestroy(e_);
    }
    operator hipEvent_t() const { return e_; }

private:
    hipEvent_t e_ = nullptr;
};

} // namespace host
} // namespace gwamd
