// What the two cut kernels of cudapolish share (polish_windows.hip on state
// paths, polish_cigar.hip on CIGAR runs): the division by the window length,
// a match state's window and positions, and the stores of the two words it
// defines in its window's record.  Device code: included by the .hip files only.
#pragma once

#include "polish_windows.hpp"

#include <hip/hip_runtime.h>

namespace gwamd
{
namespace polish
{

constexpr uint32_t kOverlapWords = sizeof(OverlapRecord) / sizeof(uint32_t);
constexpr uint32_t kRecordWords  = sizeof(gwamd_window_segment) / sizeof(uint32_t);
static_assert(kRecordWords == 8, "eight words per record");

// n / w == (hi + ((n - hi) >> sh1)) >> sh2 with hi = mulhi(n, magic), for every 32-bit n
struct WindowDivisor
{
    uint32_t magic, sh1, sh2;
};

// Granlund and Montgomery, division of a 32-bit n by the invariant w > 0:
// l = ceil(log2 w), magic = floor(2^32 (2^l - w) / w) + 1
inline WindowDivisor window_divisor(uint32_t w)
{
    uint32_t l = 0;
    while ((uint64_t(1) << l) < w)
        l++;
    WindowDivisor d;
    d.magic = uint32_t(((uint64_t(1) << 32) * ((uint64_t(1) << l) - w)) / w + 1);
    d.sh1   = l < 1 ? l : 1;
    d.sh2   = l < 1 ? 0 : l - 1;
    return d;
}

__device__ inline uint32_t uniform(uint32_t v) { return uint32_t(__builtin_amdgcn_readfirstlane(int(v))); }
__device__ inline int64_t uniform(int64_t v)
{
    return int64_t((uint64_t(uniform(uint32_t(uint64_t(v) >> 32))) << 32) | uniform(uint32_t(v)));
}

__device__ inline uint32_t window_of(uint32_t t, const WindowDivisor& d)
{
    const uint32_t hi = __umulhi(t, d.magic);
    return (hi + ((t - hi) >> d.sh1)) >> d.sh2;
}

// a match or mismatch state: its window and positions
struct Mark
{
    uint32_t k, q, t;
};

// The two words a state defines in its window's record (words 2..5: q_begin,
// q_end, t_begin, t_end).  first_of_path: the state opens its window's run in
// path order; of a Reverse overlap that state has the largest t.
__device__ inline void store_mark(uint32_t* record0, uint32_t k0, const Mark& m, bool first_of_path, bool reverse)
{
    uint32_t* r = record0 + size_t(m.k - k0) * kRecordWords;
    if (first_of_path)
    {
        r[2] = m.q;
        if (reverse)
            r[5] = m.t + 1;
        else
            r[4] = m.t;
    }
    else
    {
        r[3] = m.q + 1;
        if (reverse)
            r[4] = m.t;
        else
            r[5] = m.t + 1;
    }
}

} // namespace polish
} // namespace gwamd
