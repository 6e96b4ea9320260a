// hipCUB wrappers for the mapper kernels (device translation units only):
// exclusive sum and stable radix sort of pairs with their scratch memory
// taken from the caller's pool.
#pragma once

#include "mapper_common.hpp"

#include <hipcub/hipcub.hpp>

namespace gwamd
{
namespace mapper
{

constexpr int kThreads = 256;

inline unsigned blocks_for(uint64_t n, uint64_t cap = uint64_t(1) << 20)
{
    const uint64_t b = (n + kThreads - 1) / kThreads;
    return unsigned(std::max<uint64_t>(1, std::min(b, cap)));
}

inline void check_launch() { GWAMD_HIP_CHECK(hipGetLastError()); }

// out[i] = in[0] + ... + in[i - 1] for i < n
template <typename T>
void exclusive_sum(const T* in, T* out, size_t n, const Budget& budget, hipStream_t stream)
{
    size_t bytes = 0;
    GWAMD_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, n, stream));
    DevBuf<uint8_t> temp(std::max<size_t>(bytes, 1), budget);
    GWAMD_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(temp.data(), bytes, in, out, n, stream));
    GWAMD_HIP_CHECK(hipStreamSynchronize(stream)); // temp is freed on return
}

// stable sort of (key, value) pairs by key bits [0, end_bit)
inline void sort_pairs(const uint64_t* keys_in, uint64_t* keys_out, const uint64_t* vals_in, uint64_t* vals_out,
                       size_t n, int end_bit, const Budget& budget, hipStream_t stream)
{
    size_t bytes = 0;
    GWAMD_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, keys_in, keys_out, vals_in, vals_out, n, 0,
                                                       end_bit, stream));
    DevBuf<uint8_t> temp(std::max<size_t>(bytes, 1), budget);
    GWAMD_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(temp.data(), bytes, keys_in, keys_out, vals_in, vals_out, n, 0,
                                                       end_bit, stream));
    GWAMD_HIP_CHECK(hipStreamSynchronize(stream));
}

template <typename T>
T read_back(const T* d, hipStream_t stream)
{
    T v{};
    GWAMD_HIP_CHECK(hipMemcpyAsync(&v, d, sizeof(T), hipMemcpyDeviceToHost, stream));
    GWAMD_HIP_CHECK(hipStreamSynchronize(stream));
    return v;
}

inline int bit_length(uint64_t v)
{
    int b = 0;
    while (v)
    {
        b++;
        v >>= 1;
    }
    return b;
}

} // namespace mapper
} // namespace gwamd
